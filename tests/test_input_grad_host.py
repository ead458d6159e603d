"""CPU-side checks of the predictive gradients: the forward-mode rules of tests/_input_grad_rules.py (what csrc/input_grad.hip
computes) against central differences of the oracle kernels and of oracle.predict, the two new entries in the header and in
_lib, and the host-side refusals of FittedPosterior.predict_grad."""
import os
import re

import numpy as np
import pytest

import _input_grad_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9)
H = 1e-6
RIDGE = 1.0   # relative: cond(K~) <= 1 + N, so the differences of oracle.predict keep u cond / h ~ 2e-9 of rounding error
COMBOS = [(kind, act, get, layers) for kind in ("mlp", "resnet") for act in ("relu", "erf") for get in ("nngp", "ntk")
          for layers in (0, 1, 3)]


def _inputs():
    rng = np.random.default_rng(5)
    return rng.standard_normal((4, 7)), rng.standard_normal((9, 7))


@pytest.mark.parametrize("kind,act,get,layers", COMBOS)
def test_entry_rules_equal_central_differences_of_the_oracle_kernel(kind, act, get, layers):
    """x1 4 x 7 against x2 9 x 7: dK[r, j]/dx1[r, e] by the rules against (K(x1 + h e_re, x2) - K(x1 - h e_re, x2)) / 2h of
    oracle.mlp_kernel / oracle.dense_resnet_kernel, h = 1e-6, to 1e-8 of the largest entry: the differences' own rounding error
    is u |K| / h ~ 2e-10 of it, the truncation error h^2 K''' / 6 below that.  Measured: at most 9.9e-10."""
    x1, x2 = _inputs()
    hyp = dict(num_hiddens=layers, act=act, **HYP)
    got = R.entry_grad(kind, x1, x2, get, **hyp)
    fd = np.zeros_like(got)
    for r in range(x1.shape[0]):
        for e in range(x1.shape[1]):
            up, dn = x1.copy(), x1.copy()
            up[r, e] += H
            dn[r, e] -= H
            fd[r, :, e] = (R.KERNELS[kind](up, x2, get=get, **hyp)[r] - R.KERNELS[kind](dn, x2, get=get, **hyp)[r]) / (2 * H)
    err = np.max(np.abs(got - fd)) / np.max(np.abs(fd))
    print(kind, act, get, layers, "max |rule - fd| / max |fd| = %.3g" % err)
    assert err <= 1e-8
    # the seeded contraction is the same numbers summed
    seed = np.random.default_rng(6).standard_normal((4, 9))
    gx = R.input_grad(kind, x1, x2, seed, get, **hyp)
    assert np.max(np.abs(gx - np.einsum("rj,rje->re", seed, got))) <= 1e-13 * np.max(np.abs(gx))


@pytest.mark.parametrize("kind,act,get,layers", COMBOS)
def test_predict_grad_rules_equal_central_differences_of_oracle_predict(kind, act, get, layers):
    """9 training rows, 4 test rows, d = 7, two outputs, relative ridge RIDGE (the linear kernel of 9 points in 7 dimensions
    is singular without one): dmean and dvar against central differences of oracle.predict's mean and diagonal covariance in
    the test inputs, to 1e-8 of the largest entry of each.  Measured: at most 3.7e-9."""
    xt, x = _inputs()
    y = np.random.default_rng(7).standard_normal((9, 2))
    hyp = dict(num_hiddens=layers, act=act, **HYP)
    dmean, dvar = R.predict_grad(kind, x, y, xt, get, diag_reg=RIDGE, **hyp)
    fm, fv = np.zeros_like(dmean), np.zeros_like(dvar)
    for r in range(xt.shape[0]):
        for e in range(xt.shape[1]):
            up, dn = xt.copy(), xt.copy()
            up[r, e] += H
            dn[r, e] -= H
            mu, vu = R.predict_mean_var(kind, x, y, up, get, diag_reg=RIDGE, **hyp)
            md, vd = R.predict_mean_var(kind, x, y, dn, get, diag_reg=RIDGE, **hyp)
            fm[r, :, e] = (mu[r] - md[r]) / (2 * H)
            fv[r, e] = (vu[r] - vd[r]) / (2 * H)
    em = np.max(np.abs(dmean - fm)) / np.max(np.abs(fm))
    ev = np.max(np.abs(dvar - fv)) / np.max(np.abs(fv))
    print(kind, act, get, layers, "dmean %.3g  dvar %.3g" % (em, ev))
    assert em <= 1e-8 and ev <= 1e-8


@pytest.mark.parametrize("kind,act,get", [("mlp", "relu", "nngp"), ("resnet", "relu", "ntk"), ("mlp", "erf", "ntk")])
def test_guarded_rules_are_finite_at_the_singular_points(kind, act, get):
    """A row of x1 bit-equal to a row of x2, and an all-zero row with b_std = 0, in both dtypes."""
    x1, x2 = _inputs()
    x1[1] = x2[3]
    x1[2] = 0.0
    for dtype in (np.float64, np.float32):
        for b in (0.4, 0.0):
            f1, f2, dd = R.factors(kind, x1, x2, get, num_hiddens=2, act=act, w_std=1.3, b_std=b, last_w_std=0.9, dtype=dtype)
            assert f1.dtype == dtype and np.isfinite(f1).all() and np.isfinite(f2).all() and np.isfinite(dd).all()


def test_the_float32_rules_stay_near_the_float64_rules():
    """The yardstick of the device tests exists: the same rules in float32 lie within 1e-5 of the float64 ones."""
    x1, x2 = _inputs()
    seed = np.random.default_rng(8).standard_normal((4, 9))
    for kind, act, get, layers in COMBOS:
        hyp = dict(num_hiddens=layers, act=act, **HYP)
        g64 = R.input_grad(kind, x1, x2, seed, get, **hyp)
        g32 = R.input_grad(kind, x1, x2, seed, get, dtype=np.float32, **hyp)
        assert g32.dtype == np.float32
        assert np.max(np.abs(g32 - g64)) <= 1e-5 * np.max(np.abs(g64))


def test_the_new_entries_are_bound_with_the_header_arity():
    from smnngp import _lib
    text = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    for name, arity in (("smn_kernel_mlp_input_grad", 19), ("smn_fit_predict_grad", 6)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, "%s is not declared in include/smnngp.h" % name
        assert name in _lib.PROTOTYPES, "_lib does not bind %s" % name
        assert len(m.group(1).split(",")) == arity == len(_lib.PROTOTYPES[name]), name


class _NoDevice:
    """A context that fails the test on any device call."""

    handle = None

    def __getattr__(self, name):
        raise AssertionError("device call %r before the refusal" % name)


def _bare_posterior(fused, handle):
    from smnngp.posterior import FittedPosterior
    post = object.__new__(FittedPosterior)
    post.ctx, post.fused, post._handle = _NoDevice(), fused, handle
    post.dtype, post.num_outputs, post.num_features = np.dtype(np.float64), 1, 3
    return post


def test_predict_grad_refuses_matrix_form_and_closed_posteriors_before_any_device_call():
    x = np.zeros((2, 3))
    with pytest.raises(NotImplementedError, match="matrix-form"):
        _bare_posterior(False, object()).predict_grad(x)
    with pytest.raises(ValueError, match="closed"):
        _bare_posterior(True, None).predict_grad(x)
    with pytest.raises(ValueError, match="mean, var or both"):
        _bare_posterior(True, object()).predict_grad(x, mean=False, var=False)


def test_kernel_fn_input_grad_refuses_the_symmetric_form_and_a_bad_get():
    from smnngp import nt_kernels
    fn = nt_kernels.get_mlp_kernel(1, act="relu", w_std=1.3, b_std=0.4, last_w_std=0.9)
    with pytest.raises(NotImplementedError, match="symmetric"):
        fn.input_grad(np.zeros((2, 3)), None, np.zeros((2, 2)))
    with pytest.raises(ValueError, match="get must be"):
        fn.input_grad(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 2)), get="both")
