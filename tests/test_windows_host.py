"""Host tests of tests/_windows.py: the guard comparison must see a single changed byte anywhere outside the window, report
it with the right coordinates, and ignore the window itself.  NumPy only."""
import numpy as np
import pytest

from _windows import ROWS_AFTER, Window, pattern


def _flip_byte(w, row, col, byte=0):
    """The allocation with one byte of element (row, col) (allocation coordinates) changed."""
    after = w.host0.copy()
    raw = after.view(np.uint8).reshape(w.nrows, w.ld, w.dtype.itemsize)
    raw[row, col, byte] ^= 0x01
    return after


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
def test_layouts(dtype, layout):
    isz = np.dtype(dtype).itemsize
    for cols in (6, 7, 200):
        w = Window(5, cols, dtype, layout)
        assert w.rows_after >= 129 and w.ld > w.col_off + cols - 1 + 1
        if layout == "aligned":
            assert (w.ld * isz) % 16 == 0 and (w.col_off * isz) % 16 == 0 and ((w.rows_before * w.ld + w.col_off) * isz) % 16 == 0
        else:
            assert w.col_off == 1 and w.ld == cols + (3 if cols % 2 == 0 else 4)
            assert w.ld % 2 == 1 and w.ld - w.col_off - cols >= 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pattern_is_finite_and_no_two_neighbours_are_equal(dtype):
    for ld in (9, 16, 1021, 2042):
        p = pattern(140, ld, dtype)
        assert np.isfinite(p).all()
        assert (p[:, 1:] != p[:, :-1]).all() and (p[1:, :] != p[:-1, :]).all()
    assert np.array_equal(pattern(20, 9, dtype, seed=3), pattern(20, 9, dtype, seed=3))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
def test_a_single_changed_byte_in_each_guard_region_is_reported_with_its_coordinates(dtype, layout):
    w = Window(10, 6, dtype, layout)
    rb, co = w.rows_before, w.col_off
    isz = np.dtype(dtype).itemsize
    cases = {
        "rows before": (rb - 1, co + 2),
        "rows after": (rb + w.rows + 128, co + 3),           # where the last row of an overhanging 128-row tile lands
        "left of a row": (rb + 4, co - 1),
        "right of a row": (rb + 4, co + w.cols),
        "last element": (w.nrows - 1, w.ld - 1),
    }
    for name, (r, c) in cases.items():
        for byte in (0, isz - 1):
            hit = w.first_damage(_flip_byte(w, r, c, byte))
            assert hit == (r - rb, c - co), (name, hit)
            with pytest.raises(AssertionError, match=r"\(row %d, col %d\)" % (r - rb, c - co)):
                w.assert_guard_untouched(_flip_byte(w, r, c, byte))
    # the FIRST damaged element is the one reported
    after = _flip_byte(w, rb + 4, co + w.cols)
    after[rb + 7, 0] += 1
    assert w.first_damage(after) == (4, w.cols)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_change_inside_the_window_is_not_reported(dtype):
    w = Window(10, 6, dtype, "unaligned")
    after = w.host0.copy()
    w.inside(after)[...] = -1.0
    assert w.first_damage(after) is None
    w.assert_guard_untouched(after)
    for r, c in ((0, 0), (9, 5), (0, 5), (9, 0)):             # the four corners, one byte each
        assert w.first_damage(_flip_byte(w, w.rows_before + r, w.col_off + c)) is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zero_and_nan_payload_count_as_damage(dtype):
    w = Window(4, 6, dtype, "aligned")
    r, c = w.rows_before + 1, w.col_off + w.cols + 1
    w.host0[r, c] = 0.0
    after = w.host0.copy()
    after[r, c] = -0.0
    assert after[r, c] == w.host0[r, c]                        # equal as numbers
    assert w.first_damage(after) == (1, w.cols + 1)
    w.host0[r, c] = np.nan
    after = _flip_byte(w, r, c, 0)                             # another NaN: same class, another payload
    assert np.isnan(after[r, c]) and w.first_damage(after) == (1, w.cols + 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["aligned", "unaligned", "block"])
def test_input_window_guard_poisons_a_sum_over_ld_instead_of_d(dtype, layout):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((9, 6)).astype(dtype)
    w = Window(9, 6, dtype, layout, "in", data=x, rows_after=2)
    assert np.array_equal(w.initial(), x)
    full = w.host0
    first = w.rows_before * w.ld + w.col_off                   # what the library is handed
    flat = full.reshape(-1)
    right = np.array([flat[first + i * w.ld: first + i * w.ld + 6].sum() for i in range(9)])
    assert np.isfinite(right).all() and np.allclose(right, x.sum(axis=1))
    if layout != "block":                                      # a loader that reads ld elements of a row
        wrong = np.array([flat[first + i * w.ld: first + (i + 1) * w.ld].sum() for i in range(9)])
        assert np.isnan(wrong).all()
    # a loader that reads a row past the last one, or the row before the first
    assert np.isnan(flat[first + 9 * w.ld: first + 9 * w.ld + 6]).all()
    assert np.isnan(flat[first - w.ld: first - w.ld + 6]).all()


def test_an_output_window_keeps_a_whole_tile_of_rows_behind_it():
    with pytest.raises(AssertionError):
        Window(4, 4, np.float32, "aligned", rows_after=128)
    assert Window(4, 4, np.float32, "aligned").rows_after == ROWS_AFTER == 129
