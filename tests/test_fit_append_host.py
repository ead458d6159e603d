"""Host-side tests of appending to a fitted posterior (no GPU): the block-append rules against the one-shot oracle posterior
in fp64, the _lib prototypes of the new entries, and FittedPosterior's device-free argument checks on a stand-in object."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _fit_append_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("net,kind", [("mlp", "nngp"), ("resnet", "ntk")])
@pytest.mark.parametrize("n0,steps", [(40, (1,)), (70, (5, 60, 1)), (33, (1, 1, 1, 17)), (20, (45,))])
def test_block_append_equals_the_one_shot_posterior(n0, steps, net, kind, c):
    n, d = n0 + sum(steps), 6
    x, xt, y = R.data(n, c, d, False)
    ref = R.reference(net, kind, n0, n, c, d, False)
    kdd = ref["kdd"]
    st = R.BlockState(kdd[:n0, :n0], y[:n0], ref["lam"])
    assert st.lam == pytest.approx(1e-3 * np.trace(kdd[:n0, :n0]) / n0, rel=1e-15)
    at = n0
    for k in steps:
        st.append(kdd[at:at + k, :at], kdd[at:at + k, at:at + k], y[at:at + k])
        at += k
        # every intermediate state is the one-shot posterior of the points so far, at the SAME lambda
        part = R.one_shot(kdd[:at, :at], ref["ktd"][:, :at], ref["ktt"], y[:at], ref["lam"])
        mean, cov = st.predict(ref["ktd"][:, :at], ref["ktt"])
        assert _relerr(mean, part["mean"]) < 1e-10 and _relerr(cov, part["cov"]) < 1e-10
    assert st.n == n
    mean, cov = st.predict(ref["ktd"], ref["ktt"])
    assert _relerr(mean, ref["mean"]) < 1e-10 and _relerr(cov, ref["cov"]) < 1e-10
    assert np.allclose(st.quad, ref["quad"], rtol=1e-10, atol=0.0)
    assert abs(st.logdet - ref["logdet"]) <= 1e-10 * abs(ref["logdet"])


def test_the_frozen_ridge_is_not_the_relative_ridge_of_the_grown_set_unless_the_diagonal_is_constant():
    n0, n, d = 30, 50, 6
    x, _, _ = R.data(n, 1, d, False)
    k = R.kernel("mlp", "nngp", x)
    assert abs(R.frozen_ridge(k[:n0, :n0], 1e-3) - R.frozen_ridge(k, 1e-3)) > 1e-6
    kc = R.kernel("mlp", "nngp", R.constant_norm_rows(x))
    assert np.ptp(np.diag(kc)) < 1e-12
    assert R.frozen_ridge(kc[:n0, :n0], 1e-3) == pytest.approx(R.frozen_ridge(kc, 1e-3), rel=1e-12)


def test_an_indefinite_schur_complement_raises_and_leaves_the_rules_state_alone():
    n0, k, d = 25, 4, 6
    x, _, y = R.data(n0 + k, 1, d, False)
    kdd = R.kernel("mlp", "nngp", x)
    st = R.BlockState(kdd[:n0, :n0], y[:n0], 0.0)
    v = np.linalg.solve(st.L, kdd[n0:, :n0].T).T
    before = (st.L.copy(), st.beta.copy(), st.logdet)
    with pytest.raises(np.linalg.LinAlgError):
        st.append(kdd[n0:, :n0], 0.5 * v @ v.T, y[n0:])
    assert np.array_equal(st.L, before[0]) and np.array_equal(st.beta, before[1]) and st.logdet == before[2]


# ----------------------------------------------------------------------------- the signature table and the header
NEW = {
    "smn_fit_reserve": ["smn_fit*", "int64_t"],
    "smn_fit_append": ["smn_fit*", "const void*", "int64_t", "int64_t", "const void*", "double*", "double*", "int*"],
    "smn_fit_append_from_kernel": ["smn_fit*", "const void*", "int64_t", "int64_t", "int64_t", "const void*", "int64_t",
                                   "const void*", "double*", "double*", "int*"],
    "smn_fit_stats": ["smn_fit*", "int64_t*", "double*", "double*", "double*"],
}
CTYPE = {"smn_fit*": C.c_void_p, "const void*": C.c_void_p, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double),
         "int*": C.POINTER(C.c_int), "int64_t*": C.POINTER(C.c_int64)}


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
    assert m, "%s is not declared in include/smnngp.h" % name
    out = []
    for arg in m.group(1).replace("\n", " ").split(","):
        words = arg.strip().rsplit(" ", 1)[0]          # drop the parameter's name
        out.append(words.replace(" *", "*"))
    return out


@pytest.mark.parametrize("name", sorted(NEW))
def test_the_header_declares_the_documented_argument_lists(name):
    assert _header_args(name) == NEW[name]


@pytest.mark.parametrize("name", sorted(NEW))
def test_lib_prototypes_match_the_documented_argument_lists(name):
    from smnngp import _lib
    assert name in _lib.PROTOTYPES
    assert list(_lib.PROTOTYPES[name]) == [CTYPE[a] for a in NEW[name]]
    assert getattr(_lib._lib, name).restype is C.c_int


def test_existing_fit_signatures_are_unchanged():
    assert _header_args("smn_fit_info") == ["smn_fit*", "int64_t*", "int64_t*", "int64_t*", "size_t*"]
    assert _header_args("smn_fit_predict") == ["smn_fit*", "const void*", "int64_t", "int64_t", "void*", "void*", "void*", "int64_t"]


# ----------------------------------------------------------------------------- Python-side validation, no device
class _NoDevice:
    """Any use of the context is a failure: the checks under test must come first."""

    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s) before the arguments were checked" % name)


def _stand_in(fused=True, c=1, n=10, features=6, tail=(5, 4, 3), labels=False):
    from smnngp import posterior as post_mod
    from smnngp.spax.models import MultiSPR
    p = post_mod.FittedPosterior.__new__(post_mod.FittedPosterior)
    p.ctx, p._handle = _NoDevice(), object()
    p.fused, p.num_outputs, p.num_data, p.num_features = fused, c, n, features
    p.dtype = np.dtype(np.float64)
    p._x_train, p._x_pending = np.zeros((n,) + ((features,) if fused else tail)), []
    p.label_targets = MultiSPR.label_targets if labels else None
    p.close = lambda: None                               # (nothing to free)
    return p


def test_append_checks_its_arguments_before_any_device_call():
    p = _stand_in()
    with pytest.raises(ValueError, match="7 features, the training data 6"):
        p.append(np.zeros((3, 7)), np.zeros(3))
    with pytest.raises(ValueError, match="at least one new point"):
        p.append(np.zeros((0, 6)), np.zeros(0))
    with pytest.raises(ValueError, match=r"y must be \[3\] or \[3, 1\]"):
        p.append(np.zeros((3, 6)), np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"y must be \[3\] or \[3, 1\]"):
        p.append(np.zeros((3, 6)), np.zeros(4))
    p3 = _stand_in(c=3)
    with pytest.raises(ValueError, match=r"C = 3 outputs"):
        p3.append(np.zeros((2, 6)), np.zeros(2))
    with pytest.raises(ValueError, match=r"C = 3 outputs"):
        p3.append(np.zeros((2, 6)), np.array([0, 2]))    # integer labels: only a from_labels posterior takes them
    m = _stand_in(fused=False)
    with pytest.raises(ValueError, match=r"rows of shape \(5, 4, 2\)"):
        m.append(np.zeros((2, 5, 4, 2)), np.zeros(2))
    p._handle = None
    with pytest.raises(ValueError, match="closed"):
        p.append(np.zeros((3, 6)), np.zeros(3))
    with pytest.raises(ValueError, match="closed"):
        p.reserve(100)


def test_labels_go_through_the_models_own_rule():
    from smnngp.spax.models import MultiSPR
    p = _stand_in(c=3, labels=True)
    k, y = p._check_append(np.zeros((4, 6)), np.array([0, 2, 1, 2]))
    assert k == 4 and np.array_equal(y, MultiSPR.label_targets([0, 2, 1, 2], 3))
    with pytest.raises(ValueError, match=r"integers in \[0, 3\)"):
        p._check_append(np.zeros((2, 6)), np.array([0, 3]))
    k, y = p._check_append(np.zeros((2, 6)), np.full((2, 3), 0.25))      # explicit targets still pass
    assert np.array_equal(y, np.full((2, 3), 0.25))


def test_reserve_refuses_to_shrink_below_the_data_before_any_device_call():
    p = _stand_in(n=70)
    with pytest.raises(ValueError, match="max_points = 69 is below the 70 training points"):
        p.reserve(69)
