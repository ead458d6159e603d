"""Host checks of the finite-time gradient-descent rules (tests/_gd_rules.py) and of the Python surface around them.

The rules are the contract of predict_fn(t=...); here they are tied to what the repository already trusts: the t = infinity
posteriors of the oracle, the matrix exponential of scipy, and the exact t = 0 state.  No GPU.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import _gd_rules as R
from oracle import nngp_oracle as O

HYP = dict(num_hiddens=2, act="relu", w_std=1.3, b_std=0.4, last_w_std=0.9)
CASES = [(40, 7, 5, 2, 1e-2), (130, 9, 6, 1, 1e-3), (257, 33, 12, 3, 1e-4)]


def _data(n, t, d, c):
    rng = np.random.default_rng(n)
    xa = rng.standard_normal((n + t, d))
    y = rng.standard_normal((n, c))
    return xa, y


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("n,t,d,c,diag_reg", CASES)
def test_long_time_limit_is_the_oracle_posterior(n, t, d, c, diag_reg):
    xa, y = _data(n, t, d, c)
    k, th = R.joint_kernels("mlp", xa, ("nngp", "ntk"), **HYP)
    ref_m, ref_c = O.predict(k[:n, :n], k[n:, :n], k[n:, n:], y, diag_reg=diag_reg)
    ntk_m, ntk_c = O.predict_ntk(k[:n, :n], k[n:, :n], k[n:, n:], th[:n, :n], th[n:, :n], y, diag_reg=diag_reg)
    m, cv = R.gd_predict(k, None, n, y, [1e15, np.inf], diag_reg)
    mt, ct = R.gd_predict(k, th, n, y, [1e15, np.inf], diag_reg)
    for j in range(2):
        errs = (_rel(m[j], ref_m), _rel(cv[j], ref_c), _rel(mt[j], ntk_m), _rel(ct[j], ntk_c))
        print("gd host limit N=%d diag_reg=%g t=%s: %s" % (n, diag_reg, ("1e15", "inf")[j], " ".join("%.1e" % e for e in errs)))
        assert max(errs) <= 1e-11


def test_absolute_ridge_limit():
    n, t, d, c, diag_reg = CASES[0]
    xa, y = _data(n, t, d, c)
    k, _ = R.joint_kernels("mlp", xa, "nngp", **HYP)
    ref_m, ref_c = O.predict(k[:n, :n], k[n:, :n], k[n:, n:], y, diag_reg=diag_reg, diag_reg_absolute_scale=True)
    m, cv = R.gd_predict(k, None, n, y, np.inf, diag_reg, absolute=True)
    assert _rel(m[0], ref_m) <= 1e-11 and _rel(cv[0], ref_c) <= 1e-11


@pytest.mark.parametrize("get", ["nngp", "ntk"])
def test_time_zero_is_the_prior(get):
    n, t, d, c, diag_reg = CASES[0]
    xa, y = _data(n, t, d, c)
    k, th = R.joint_kernels("mlp", xa, ("nngp", "ntk"), **HYP)
    m, cv = R.gd_predict(k, th if get == "ntk" else None, n, y, 0.0, diag_reg)
    assert np.array_equal(m[0], np.zeros((t, c))) and np.array_equal(cv[0], k[n:, n:])


@pytest.mark.parametrize("n,t,d,c,diag_reg", CASES)
@pytest.mark.parametrize("get", ["nngp", "ntk"])
def test_mean_is_the_matrix_exponential_solution(get, n, t, d, c, diag_reg):
    xa, y = _data(n, t, d, c)
    k, th = R.joint_kernels("mlp", xa, ("nngp", "ntk"), **HYP)
    g = th if get == "ntk" else k
    gt = R.regularised(g[:n, :n], diag_reg)
    s = 50.0 / (n * c)
    ref = g[n:, :n] @ np.linalg.solve(gt, (np.eye(n) - sla.expm(-s * gt)) @ y)
    m, _ = R.gd_predict(k, th if get == "ntk" else None, n, y, 50.0, diag_reg)
    err = _rel(m[0], ref)
    print("gd host expm %s N=%d: %.1e" % (get, n, err))
    assert err <= 1e-12


def test_learning_rate_scales_time():
    n, t, d, c, diag_reg = CASES[0]
    xa, y = _data(n, t, d, c)
    k, _ = R.joint_kernels("mlp", xa, "nngp", **HYP)
    a = R.gd_predict(k, None, n, y, [1.0, 50.0], diag_reg, learning_rate=3.0)
    b = R.gd_predict(k, None, n, y, [3.0, 150.0], diag_reg)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_other_kernels_and_float32_evaluate():
    rng = np.random.default_rng(3)
    xa = rng.standard_normal((24 + 5, 6, 6, 2))
    y = rng.standard_normal((24, 1))
    k, th = R.joint_kernels("cnn", xa, "nngp", dtype=np.float32, **HYP)
    assert th is None and k.dtype == np.float32
    m, cv = R.gd_predict(k, None, 24, y, [0.0, 1.0, np.inf], 1e-2, dtype=np.float32)
    assert m.shape == (3, 5, 1) and cv.shape == (3, 5, 5) and m.dtype == np.float32 and np.isfinite(cv).all()
    k2, th2 = R.joint_kernels("dense_resnet", xa.reshape(29, -1), ("nngp", "ntk"), **HYP)
    assert k2.shape == th2.shape == (29, 29)
    with pytest.raises(ValueError):
        R.joint_kernels("cnn", xa, "ntk", **HYP)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


def test_max_learning_rate_formula(lib):
    from smnngp import spectral
    lam = np.array([0.25, 1.5, 7.0])
    assert spectral.max_learning_rate(lam, 12) == 2.0 * 12 / (7.0 + 1e-12)
    assert spectral.max_learning_rate(lam, 12, momentum=0.9, eps=0.5) == 2.0 * 1.9 * 12 / 7.5
    assert spectral.__all__ == ["eigh_pd", "max_learning_rate"]


def test_new_entries_are_bound(lib):
    assert len(lib.PROTOTYPES["smn_eigh_pd"]) == 11 and len(lib.PROTOTYPES["smn_predict_gd"]) == 19
    assert hasattr(lib._lib, "smn_eigh_pd") and hasattr(lib._lib, "smn_predict_gd")
    import inspect

    from smnngp import predict
    sig = inspect.signature(predict.gradient_descent_mse_ensemble)
    assert list(sig.parameters)[-1] == "learning_rate" and sig.parameters["learning_rate"].default == 1.0
    assert predict.PredictResult.evals is None
