"""CPU checks of tests/_conv_pairs.py: the premises of the multi-pass tests in tests/test_gpu_conv_pairs.py (pass counts, a
sample that touches every pass, single-pass chunking) for every shape and n those tests use."""
import numpy as np
import pytest

import _conv_pairs as P

BUILDS = P.multi_pass_builds()


def test_grid_waves_is_the_launch_cap_of_both_builders():
    """GRID_WAVES restates `blocks > 256 * 8` (4 waves per workgroup) of cnn_t and resnet_t: both lines must still say so."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "scale-mixtures-of-neural-network-gaussian-processes_amd", "csrc")
    for name in ("cnn.hip", "cnn_resnet.hip"):
        with open(os.path.join(csrc, name)) as f:
            assert "if (blocks > 256 * 8) blocks = 256 * 8;" in f.read(), name
    assert P.GRID_WAVES == 256 * 8 * 4


@pytest.mark.parametrize("label,n,sym,n2,min_passes", BUILDS, ids=[b[0] for b in BUILDS])
def test_every_build_is_multi_pass_and_its_sample_covers_every_pass(label, n, sym, n2, min_passes):
    total = P.npairs(n, sym, n2)
    assert P.passes(total) >= min_passes >= 2
    rows, cols = P.sample_rows_cols(n, sym, n2)
    assert len(rows) <= P.MAX_SAMPLE and len(cols) <= P.MAX_SAMPLE
    assert len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
    last = (n if sym else n2) - 1
    assert {0, 1, n - 1} <= set(rows) and {0, 1, last} <= set(cols)
    assert rows.max() < n and cols.max() <= last and rows.min() >= 0 and cols.min() >= 0
    assert P.sampled_passes(rows, cols, sym, n2) == set(range(P.passes(total)))


def test_all_but_the_stated_130_image_case_have_three_passes():
    assert [b[0] for b in BUILDS if b[4] < 3] == ["resnet (32, 32, 3) n=130"]
    assert P.passes(P.npairs(130)) == 2 and P.passes(P.npairs(181)) == 3 and P.passes(P.npairs(222)) == 4
    assert P.passes(P.npairs(150, False, 111)) == 3
    assert P.passes(P.GRID_WAVES) == 1 and P.passes(P.GRID_WAVES + 1) == 2


def test_pass_of_against_brute_force_enumeration():
    pr = 0
    for n in range(222):                                    # the lower triangle, row by row
        for m in range(n + 1):
            assert P.pass_of(n, m, True) == pr // P.GRID_WAVES
            assert P.pass_of(m, n, True) == pr // P.GRID_WAVES       # the mirrored entry is the same pair
            assert P.decode(pr, True) == (n, m)
            pr += 1
    assert pr == P.npairs(222) == 24753
    pr = 0
    for n in range(150):                                    # the 150 x 111 grid, row by row
        for m in range(111):
            assert P.pass_of(n, m, False, 111) == pr // P.GRID_WAVES
            assert P.decode(pr, False, 111) == (n, m)
            pr += 1
    assert pr == P.npairs(150, False, 111) == 16650


@pytest.mark.parametrize("n", sorted({b[1] for b in BUILDS if b[2]}))
def test_chunks_are_single_pass_and_cover_every_row_once(n):
    chunks = P.row_chunks(n, n)
    assert all(0 < (r1 - r0) * n <= P.GRID_WAVES for r0, r1 in chunks)
    assert np.array_equal(np.concatenate([np.arange(r0, r1) for r0, r1 in chunks]), np.arange(n))


def test_cnn_forms_reach_the_kernels_they_name():
    """The table of forms against the restated dispatch of launch_pairs; every form of the dispatch appears."""
    reached = set()
    for shape, dtypes, layers, form in P.CNN_FORMS:
        for dt in dtypes:
            assert form.startswith(P.cnn_form(shape, dt)), (shape, dt, form)
            reached.add((P.cnn_form(shape, dt), dt))
    forms = {"conv_pair_kernel<%d,%s>" % (np_, e) for np_ in (4, 16, 64) for e in ("exact", "ragged")}
    assert {(f, dt) for f in forms for dt in ("f32", "f64")} <= reached
    assert {("conv_pair44_kernel<C=1>", "f64"), ("conv_pair44_kernel<C=3>", "f64"), ("conv_pair32_kernel", "f64")} <= reached


def test_scaled_images_and_leading_dimensions():
    x = P.scaled_images((10, 4, 4, 2), np.float32, 0)
    assert x.dtype == np.float32 and x.shape == (10, 4, 4, 2)
    raw = np.random.default_rng(0).standard_normal((10, 4, 4, 2))
    assert np.allclose(x[9], raw[9] * 1.9, rtol=1e-6) and np.allclose(x[0], raw[0], rtol=1e-6)
    for dt, al in ((np.float32, 4), (np.float64, 2)):
        for cols in (5, 8, 222):
            ld = P.aligned_ld(cols, dt)
            assert ld > cols and ld % al == 0 and ld - cols <= al
