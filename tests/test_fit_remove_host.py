"""Host-side tests of removing points from a fitted posterior (no GPU): the blocked LQ removal of _fit_remove_rules.py against
numpy.linalg.cholesky of the kept block in fp64, the staircase the sweep relies on, FittedPosterior.remove's index
normalisation and its device-free refusals on a stand-in object, and the _lib prototype of smn_fit_remove."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import _fit_append_rules as R
import _fit_remove_rules as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n0, name) for n0 in (130, 260) for name in RR.index_sets(n0)]


def _state(n0, c=3, d=6):
    x, _, y = R.data(n0, c, d, False)
    kdd = R.kernel("mlp", "nngp", x)
    lam = R.frozen_ridge(kdd, R.RIDGE[np.float64])
    st = R.BlockState(kdd, y, lam)
    return kdd, y, lam, st


@pytest.mark.parametrize("b", [32, 64])
@pytest.mark.parametrize("n0,name", CASES)
def test_blocked_removal_equals_the_cholesky_factor_of_the_kept_points(n0, name, b):
    idx = RR.index_sets(n0)[name]
    kdd, y, lam, st = _state(n0)
    keep = np.setdiff1d(np.arange(n0), idx)
    l_ref = np.linalg.cholesky(kdd[np.ix_(keep, keep)] + lam * np.eye(keep.size))        # the SAME lam: the frozen ridge
    b_ref = sla.solve_triangular(l_ref, y[keep], lower=True)
    for what, (l_new, b_new) in (("one pass", RR.blocked_remove(st.L, st.beta, idx, b)),
                                 ("passes of KMAX", RR.remove(st.L, st.beta, idx, b))):
        assert l_new.shape == l_ref.shape and b_new.shape == b_ref.shape
        assert np.abs(l_new - l_ref).max() < 1e-10, what
        assert np.abs(b_new - b_ref).max() < 1e-9, what
        assert (np.diag(l_new) > 0.0).all(), what
        assert not np.triu(l_new, 1).any(), what                                         # exactly 0 above the diagonal
        assert abs(np.sum(b_new ** 2) - np.sum(b_ref ** 2)) <= 1e-10 * np.sum(b_ref ** 2)
        assert abs(np.sum(np.log(np.diag(l_new))) - np.sum(np.log(np.diag(l_ref)))) < 1e-10


@pytest.mark.parametrize("b", [32, 64])
@pytest.mark.parametrize("n0,name", CASES)
def test_the_staircase_block_s_is_zero_right_of_column_s_plus_b_plus_k(n0, name, b):
    idx = RR.index_sets(n0)[name]
    _, _, _, st = _state(n0, c=1)
    seen = []
    RR.blocked_remove(st.L, st.beta, idx, b, staircase=seen)
    assert bool(seen) == (name != "last"), "the suffix path has no block, every other set at least one"
    assert all(v == 0.0 for v in seen), seen


def test_passes_take_kmax_rows_from_the_highest_indices_down():
    idx = list(range(0, 260, 7))
    got = RR.passes(idx)
    assert [len(p) for p in got] == [32, 6] and got[0] == idx[-32:] and got[1] == idx[:6]
    assert RR.passes([4, 9]) == [[4, 9]] and len(RR.index_sets(260)["kmax_plus_1"]) == RR.KMAX + 1


def test_suffix_removal_is_the_leading_block_of_the_factor():
    _, _, _, st = _state(130)
    l_new, b_new = RR.blocked_remove(st.L, st.beta, list(range(120, 130)))
    assert np.array_equal(l_new, st.L[:120, :120]) and np.array_equal(b_new, st.beta[:120])


# ----------------------------------------------------------------------------- index normalisation
def test_index_normalisation():
    from smnngp.posterior import normalise_indices as norm
    assert norm(3, 10).tolist() == [3] and norm(-1, 10).tolist() == [9] and norm(np.int32(4), 10).tolist() == [4]
    assert norm([7, -10, 2], 10).tolist() == [0, 2, 7]
    assert norm(range(3), 10).tolist() == [0, 1, 2]
    assert norm(np.array([5, 1], dtype=np.uint8), 10).tolist() == [1, 5]
    assert norm(np.array([-2, 0], dtype=np.int16), 10).dtype == np.int64
    mask = np.zeros(10, dtype=bool)
    mask[[1, 8]] = True
    assert norm(mask, 10).tolist() == [1, 8]
    assert norm(list(mask), 10).tolist() == [1, 8]
    for bad, word in (([], "empty"), (np.zeros(10, dtype=bool), "empty"), ([10], "index 10 is out of range"),
                      ([-11], "index -11 is out of range"), ([3, 3], "index 3 is given more than once"),
                      ([3, -7], "index 3 is given more than once"), (np.ones(9, dtype=bool), r"shape \(10,\)"),
                      ([1.0, 2.0], "dtype float64"), ([[1, 2]], "shape")):
        with pytest.raises(ValueError, match=word):
            norm(bad, 10)


# ----------------------------------------------------------------------------- refusals before any device call
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s) before the arguments were checked" % name)


def _stand_in(n=10):
    from smnngp import posterior as post_mod
    p = post_mod.FittedPosterior.__new__(post_mod.FittedPosterior)
    p.ctx, p._handle = _NoDevice(), object()
    p.fused, p.num_outputs, p.num_data, p.num_features = True, 1, n, 6
    p.dtype = np.dtype(np.float64)
    p._x_train, p._x_pending = np.zeros((n, 6)), []
    p.close = lambda: None
    return p


def test_remove_checks_its_arguments_before_any_device_call():
    p = _stand_in()
    for bad, word in (([], "empty"), (np.zeros(10, dtype=bool), "empty"), (range(10), "all 10 training points"),
                      (np.ones(10, dtype=bool), "all 10 training points"), ([10], "index 10 is out of range"),
                      (-11, "index -11 is out of range"), ([2, 2], "index 2 is given more than once"),
                      ([-1, 9], "index 9 is given more than once")):
        with pytest.raises(ValueError, match=word):
            p.remove(bad)
    p._handle = None
    with pytest.raises(ValueError, match="closed"):
        p.remove([0])


# ----------------------------------------------------------------------------- the signature table and the header
ARGS = ["smn_fit*", "const int64_t*", "int64_t", "double*", "double*"]
CTYPE = {"smn_fit*": C.c_void_p, "const int64_t*": C.POINTER(C.c_int64), "int64_t": C.c_int64, "double*": C.POINTER(C.c_double)}


def test_the_header_declares_smn_fit_remove_and_names_its_sizes():
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    m = re.search(r"\bint smn_fit_remove\(([^;]*)\);", text)
    assert m, "smn_fit_remove is not declared in include/smnngp.h"
    got = [a.strip().rsplit(" ", 1)[0].replace(" *", "*") for a in m.group(1).replace("\n", " ").split(",")]
    assert got == ARGS
    assert "KMAX = %d" % RR.KMAX in text and "b = %d" % RR.B in text


def test_lib_prototype_matches_the_documented_argument_list():
    from smnngp import _lib
    assert "smn_fit_remove" in _lib.PROTOTYPES
    assert list(_lib.PROTOTYPES["smn_fit_remove"]) == [CTYPE[a] for a in ARGS]
    assert _lib._lib.smn_fit_remove.restype is C.c_int
    from smnngp.posterior import FittedPosterior
    assert callable(FittedPosterior.remove)
