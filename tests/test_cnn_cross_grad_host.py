"""Host-side checks of the conv-NNGP predictive gradients (no GPU): the cross, multi-seed rules the GPU tests compare
smn_kernel_cnn_input_grad_cross against (tests/_cnn_cross_grad_rules.py) agree with central differences of the fp64 reference
kernel, and the predict_grad rules with central differences of the reference posterior; pooled-kernel, conv-ResNet and
foreign-callable posteriors still refuse before any device call; header, ctypes table and library agree on the two new entries.

Bounds.  Central differences with step h = 1e-5 of an fp64 function of size O(1..10) carry h^2 f''' / 6 ~ 1e-10 of truncation
and 2^-53 |f| / h ~ 1e-10 of rounding: the kernel check allows 1e-7 of the largest gradient entry (a hundred times that; it
measures ~1e-9), the posterior check 1e-6 (the solves amplify both by the conditioning of K~, ~1e2 at ridge 0.05)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)

import _cnn_cross_grad_rules as X  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, LW = 1.3, 0.9
TOL_KERNEL, TOL_POST = 1e-7, 1e-6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


# ----------------------------------------------------------------------------- 1. the cross rules against the oracle kernel
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("layers", [0, 2, 3])
@pytest.mark.parametrize("b_std", [0.0, 0.4])
def test_cross_rules_against_central_differences_of_the_oracle_kernel(act, layers, b_std):
    """F(x1) = sum_rj s[r, j] K(x1_r, x2_j) + sum_r gdiag[r] K(x1_r, x1_r) for each of the c mean seeds (s = alpha^T, no
    diagonal) and the variance seed, differentiated at every pixel of x1: 2 x 5 images of 4 x 4 x 2."""
    n1, n2, h, w, cin, c = 2, 5, 4, 4, 2, 2
    rng = np.random.default_rng([layers, int(10 * b_std), act == "erf"])
    x1, x2 = rng.standard_normal((n1, h, w, cin)), rng.standard_normal((n2, h, w, cin))
    alpha, gbar, gdiag = rng.standard_normal((n2, c)), rng.standard_normal((n1, n2)), rng.standard_normal(n1)
    kern = lambda a, b: O.cnn_kernel(a, b, layers, act, W, b_std, LW)   # noqa: E731
    r = X.cross_input_grad(x1, x2, layers, act, W, b_std, LW, alpha=alpha, gbar=gbar, gdiag=gdiag)
    assert r["gmean"].shape == (n1, c, h, w, cin) and r["gvar"].shape == (n1, h, w, cin)
    assert np.all(r["smean"] >= np.abs(r["gmean"]) * (1 - 1e-12)) and np.all(r["svar"] >= np.abs(r["gvar"]) * (1 - 1e-12))

    def values(xx):
        k = kern(xx, x2)
        return np.concatenate([np.sum(k * alpha[:, q][None, :], axis=1) for q in range(c)]
                              + [np.sum(k * gbar, axis=1) + gdiag * np.diag(kern(xx, None))])   # [(c + 1) n1], per row

    step, worst = 1e-5, 0.0
    scale = max(np.max(np.abs(r["gmean"])), np.max(np.abs(r["gvar"])))
    for idx in np.ndindex(n1, h, w, cin):
        up, dn = x1.copy(), x1.copy()
        up[idx] += step; dn[idx] -= step
        fd = ((values(up) - values(dn)) / (2 * step)).reshape(c + 1, n1)[:, idx[0]]      # only row idx[0] moves
        got = np.array([r["gmean"][idx[0], q][idx[1:]] for q in range(c)] + [r["gvar"][idx]])
        worst = max(worst, float(np.max(np.abs(got - fd))) / scale)
    print("cross rules vs oracle %s L%d b_std=%g: worst %.3e of the largest entry (tol %g)" % (act, layers, b_std, worst, TOL_KERNEL))
    assert worst <= TOL_KERNEL


def test_cross_rules_without_a_diagonal_or_without_a_cross_term():
    rng = np.random.default_rng(5)
    x1, x2 = rng.standard_normal((3, 4, 5, 1)), rng.standard_normal((4, 4, 5, 1))
    gbar, gdiag = rng.standard_normal((3, 4)), rng.standard_normal(3)
    both = X.cross_input_grad(x1, x2, 2, "relu", W, 0.2, LW, gbar=gbar, gdiag=gdiag)["gvar"]
    cross = X.cross_input_grad(x1, x2, 2, "relu", W, 0.2, LW, gbar=gbar)["gvar"]
    diag = X.cross_input_grad(x1, x2, 2, "relu", W, 0.2, LW, gdiag=gdiag)["gvar"]
    assert np.allclose(cross + diag, both, rtol=1e-12, atol=1e-14) and np.max(np.abs(diag)) > 0 and np.max(np.abs(cross)) > 0


# ----------------------------------------------------------------------------- 2. the posterior's rules against the oracle
@pytest.mark.parametrize("act,layers,c", [("relu", 2, 1), ("erf", 3, 3)])
def test_predict_grad_rules_against_central_differences_of_the_oracle_posterior(act, layers, c):
    n, t, h, w, cin, ridge, b_std = 12, 3, 4, 4, 2, 0.05, 0.3
    rng = np.random.default_rng(7 + c)
    x, xt, y = rng.standard_normal((n, h, w, cin)), rng.standard_normal((t, h, w, cin)), rng.standard_normal((n, c))
    kern = lambda a, b: O.cnn_kernel(a, b, layers, act, W, b_std, LW)   # noqa: E731
    dmean, dvar, _, _ = X.predict_grad(kern, x, y, xt, ridge, layers, act, W, b_std, LW)
    assert dmean.shape == (t, c, h, w, cin) and dvar.shape == (t, h, w, cin)
    k_dd = kern(x, None)

    def predict(xx):
        mean, cov = O.predict(k_dd, kern(xx, x), kern(xx, None), y, diag_reg=ridge, diag_reg_absolute_scale=True)
        return mean, np.diag(cov)

    step, v = 1e-5, rng.standard_normal(xt.shape)
    (mu, vu), (md, vd) = predict(xt + step * v), predict(xt - step * v)
    fd_m, fd_v = (mu - md) / (2 * step), (vu - vd) / (2 * step)
    got_m, got_v = np.einsum("rkhwc,rhwc->rk", dmean, v), np.einsum("rhwc,rhwc->r", dvar, v)
    err_m = np.max(np.abs(got_m - fd_m)) / np.max(np.abs(fd_m))
    err_v = np.max(np.abs(got_v - fd_v)) / np.max(np.abs(fd_v))
    print("predict_grad rules vs oracle %s L%d c%d: slope of the mean %.3e, of the variance %.3e (tol %g)" % (act, layers, c, err_m,
                                                                                                         err_v, TOL_POST))
    assert err_m <= TOL_POST and err_v <= TOL_POST


# ----------------------------------------------------------------------------- 3. refusals before any device call
class _NoDevice:
    """A context that fails the test on any device call."""

    handle = None

    def __getattr__(self, name):
        raise AssertionError("device call %r before the refusal" % name)


def _bare_posterior(kernel_fn, shape=(5, 6, 6, 1)):
    from smnngp.posterior import FittedPosterior
    post = object.__new__(FittedPosterior)
    post.ctx, post.fused, post._handle, post.kernel_fn, post.mode = _NoDevice(), False, object(), kernel_fn, "nngp"
    post.dtype, post.num_outputs, post.num_data, post.capacity = np.dtype(np.float64), 1, shape[0], 4
    post._x_train, post._x_pending = np.zeros(shape), []
    return post


def test_other_matrix_form_posteriors_still_refuse_before_any_device_call(lib):
    from smnngp import nt_kernels
    x = np.zeros((2, 8, 8, 1))
    for fn in (nt_kernels.get_cnn_pool_kernel(2), nt_kernels.get_conv_resnet_kernel(1, 3), object(), lambda a, b, get: None):
        with pytest.raises(NotImplementedError, match="matrix-form"):
            _bare_posterior(fn, (5, 8, 8, 1)).predict_grad(x)


def test_conv_posterior_checks_its_arguments_before_any_device_call(lib):
    from smnngp import nt_kernels
    fn = nt_kernels.get_cnn_kernel(2)
    with pytest.raises(NotImplementedError, match="1024"):
        _bare_posterior(fn, (5, 40, 40, 1)).predict_grad(np.zeros((2, 40, 40, 1)))
    with pytest.raises(ValueError, match="mean, var or both"):
        _bare_posterior(fn).predict_grad(np.zeros((2, 6, 6, 1)), mean=False, var=False)
    with pytest.raises(ValueError, match="rows of shape"):
        _bare_posterior(fn).predict_grad(np.zeros((2, 6, 5, 1)))
    closed = _bare_posterior(fn)
    closed._handle = None
    with pytest.raises(ValueError, match="closed"):
        closed.predict_grad(np.zeros((2, 6, 6, 1)))


def test_cnn_kernel_fn_input_grad_refusals(lib):
    from smnngp import nt_kernels
    x = np.zeros((2, 8, 8, 1))
    with pytest.raises(NotImplementedError, match="symmetric"):
        nt_kernels.get_cnn_kernel(2).input_grad(x, None, np.zeros((2, 2)))
    for fn in (nt_kernels.get_cnn_pool_kernel(2), nt_kernels.get_conv_resnet_kernel(1, 3)):
        with pytest.raises(NotImplementedError, match="get_cnn_kernel"):
            fn.input_grad(x, x, np.zeros((2, 2)))
    with pytest.raises(NotImplementedError, match="1024"):
        nt_kernels.get_cnn_kernel(2).input_grad(np.zeros((1, 33, 32, 1)), np.zeros((1, 33, 32, 1)), np.zeros((1, 1)))
    with pytest.raises(ValueError, match=r"\[N,H,W,C\]"):
        nt_kernels.get_cnn_kernel(2).input_grad(np.zeros((2, 64)), np.zeros((2, 64)), np.zeros((2, 2)))


# ----------------------------------------------------------------------------- 4. header, ctypes table, exports
def test_header_and_lib_agree_on_the_two_entries(lib):
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    raw = C.CDLL(lib.LIB_PATH)
    for name, arity in (("smn_kernel_cnn_input_grad_cross", 21), ("smn_fit_weights", 7)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, "%s is not declared in include/smnngp.h" % name
        assert name in lib.PROTOTYPES, "_lib does not bind %s" % name
        assert len(m.group(1).split(",")) == arity == len(lib.PROTOTYPES[name]), name
        assert hasattr(raw, name), "libsmnngp.so does not export %s" % name
    assert lib._lib.smn_kernel_cnn_input_grad_cross(None, lib.F64, 0, 1, 1.0, 0.1, 1.0, None, 1, None, 1, 4, 4, 1, None, 0, None, 1,
                                                    None, None, None) == lib.EINVAL
    assert lib._lib.smn_fit_weights(None, None, 1, 1, None, 1, None) == lib.EINVAL
