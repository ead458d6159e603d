"""Regression on the pivoted-Cholesky factor, host side: the NumPy rules of tests/_lowrank_rules.py against themselves and
against the exact model, and every refusal of the Python surface that needs no device.

  1. the rules' Woodbury form against their dense form (K^ + D formed and solved), both corrections, eps from 1e-1 to 1e-6:
     1e-8 relative for quad and logdet at every eps and for mean and var at eps >= 1e-2 (norm-wise: the largest error over
     the largest reference entry) -- the bound the device's f64 results are held to.  Below 1e-2 the DENSE predictions are the
     weaker side: q^T K^^-1 Y cancels the 1 / eps part of K^^-1 Y, so a dense solve loses digits as cond(K^) ~ 1 / eps grows,
     and mean and var are held to 1e-8 (1e-2 / eps) there.
  2. at rank = N the factor is the whole matrix (resid = 0, both corrections coincide): the rules against the exact
     log-marginal likelihood and posterior of K + lam I from the reference kernels, to 1e-8 relative.
  3. LowRankSPR / lowrank.woodbury_fit: ValueError / NotImplementedError / TypeError before any device call."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _lowrank_rules as LR
import _pchol_rules as PR
from oracle import nngp_oracle as O

HP = dict(w_std=1.3, b_std=0.2, last_w_std=0.9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * np.exp(0.5 * rng.standard_normal((n, 1)))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def problem():
    n, t, d = 300, 23, 5
    xa = data(n + t, d)
    K = np.asarray(O.mlp_kernel(xa, None, num_hiddens=2, act="relu", **HP), dtype=np.float64)
    rng = np.random.default_rng(3)
    y = np.stack([np.sin(xa[:n, 0]) + 0.1 * rng.standard_normal(n), rng.standard_normal(n)], axis=1)
    K.setflags(write=False)
    return SimpleNamespace(n=n, t=t, K=K, y=y)


@pytest.mark.parametrize("fitc", [True, False], ids=["fitc", "none"])
@pytest.mark.parametrize("m", [1, 17, 40])
def test_woodbury_form_equals_dense_form(problem, m, fitc):
    n, K = problem.n, problem.K
    r = PR.pivoted_cholesky(K[:n, :n], m)
    assert r.rank == m
    R = r.L[r.pivots]
    kzt, ktt = K[r.pivots][:, n:], np.diag(K)[n:]
    for eps in (1e-1, 1e-2, 1e-4, 1e-6):
        a = LR.woodbury(r.L, r.resid, eps, fitc, problem.y, R, kzt, ktt)
        b = LR.dense(r.L, r.resid, eps, fitc, problem.y, R, kzt, ktt)
        assert rel(a.quad, b.quad) <= 1e-8, (m, fitc, eps)
        for name in ("mean", "var"):
            assert rel(getattr(a, name), getattr(b, name)) <= 1e-8 * max(1.0, 1e-2 / eps), (name, m, fitc, eps)
        assert abs(a.logdet - b.logdet) <= 1e-8 * abs(b.logdet), (m, fitc, eps)
        assert np.all(a.var > 0.0)


def test_float32_split_gram_is_a_perturbation_of_the_fp64_one(problem):
    """The yardstick itself: the float32-split Gram differs from the fp64 one by rounding, not by construction."""
    n, K = problem.n, problem.K
    r = PR.pivoted_cholesky(K[:n, :n], 17, dtype=np.float32)
    w = 1.0 / LR.weights(r.resid, 1e-2, True, n)
    G32, B32, s32 = LR.gram(r.L, w, problem.y, np.float32, split=128)
    G64, B64, s64 = LR.gram(r.L, w, problem.y.astype(np.float32), np.float64)
    assert np.array_equal(G32, G32.T)
    assert 0.0 < rel(G32, G64) < 1e-5 and rel(B32, B64) < 1e-12 and rel(s32, s64) < 1e-12


@pytest.mark.parametrize("lam", [1e-1, 1e-3])
def test_full_rank_is_the_exact_model(lam):
    n, t, d = 65, 9, 5
    xa = data(n + t, d, seed=5)
    K = np.asarray(O.mlp_kernel(xa, None, num_hiddens=2, act="relu", **HP), dtype=np.float64)
    y = np.sin(xa[:n, 0]) + 0.3 * xa[:n, 1]
    r = PR.pivoted_cholesky(K[:n, :n], n)
    assert r.rank == n and np.all(r.resid == 0.0)
    R = r.L[r.pivots]
    for fitc in (True, False):
        a = LR.woodbury(r.L, r.resid, lam, fitc, y, R, K[r.pivots][:, n:], np.diag(K)[n:])
        cov = K[:n, :n] + lam * np.eye(n)
        gp, tp = O.mvn_logpdf(y, cov), O.mvt_logpdf(y, 1.7 * cov, 4.0)
        assert abs(LR.gp_logpdf(a.quad[0], a.logdet, n) - gp) <= 1e-8 * abs(gp)
        assert abs(LR.tp_logpdf(a.quad[0], a.logdet, n, 4.0, 1.7) - tp) <= 1e-8 * abs(tp)
        mean, pc = O.predict(K[:n, :n], K[n:, :n], K[n:, n:], y, diag_reg=lam, diag_reg_absolute_scale=True)
        assert rel(a.mean, mean) <= 1e-8 and rel(a.var, np.diag(pc)) <= 1e-8


def test_limits_match_the_header():
    from smnngp import _lib
    src = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    assert int(re.search(r"#define SMN_LOWRANK_MAX_RANK (\d+)", src).group(1)) == _lib.LOWRANK_MAX_RANK == 4096
    assert int(re.search(r"#define SMN_LOWRANK_SPLIT (\d+)", src).group(1)) == _lib.LOWRANK_SPLIT


# ---------------------------------------------------------------- refusals without a device
def _model_args():
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.5, 1.0)
    return kernel, GaussianLikelihood(), np.zeros((10, 3)), np.zeros(10), 0.0, 1.0


@pytest.mark.parametrize("kw", [dict(rank=0), dict(rank=11), dict(rank=-3), dict(rank=2.5), dict(rank=True), dict(rank=4097),
                                dict(rank=3, correction="sor"), dict(rank=3, correction=None), dict(rank=3, tol=-1.0),
                                dict(rank=3, tol=float("nan"))],
                         ids=lambda kw: "-".join("%s=%s" % it for it in kw.items()))
def test_bad_rank_correction_tol_raise_value_error(kw):
    from smnngp.spax.models import LowRankSPR
    with pytest.raises(ValueError):
        LowRankSPR(*_model_args(), **kw)


def test_bad_data_and_unsupported_pieces_are_refused_before_the_device():
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import LowRankSPR
    kernel, lik, x, y, ym, ys = _model_args()
    with pytest.raises(ValueError):
        LowRankSPR(kernel, lik, x, np.zeros(9), ym, ys, rank=3)
    with pytest.raises(ValueError):
        LowRankSPR(kernel, lik, np.zeros(10), y, ym, ys, rank=3)
    with pytest.raises(TypeError):
        LowRankSPR(kernel, lik, x, y, ym, ys)                          # rank is required
    scaled = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, w_std=w, b_std=b, last_w_std=l), input_scales=np.ones(3))
    with pytest.raises(NotImplementedError):
        LowRankSPR(scaled, lik, x, y, ym, ys, rank=3)
    with pytest.raises(NotImplementedError):
        LowRankSPR(kernel, object(), x, y, ym, ys, rank=3)             # a likelihood without lml_params
    bare = LowRankSPR.__new__(LowRankSPR)                              # the methods that do not exist touch nothing
    for call in (bare.loss_and_grad, bare.loo_loss, bare.loo_predict, bare.loo_loss_and_grad, bare.posterior,
                 lambda: bare.sample_posterior(0, x, 2), lambda: bare.predict(x, cov="full")):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        bare.predict(x, chunk=0)


def test_woodbury_fit_checks_its_arguments_before_the_device():
    from smnngp import lowrank
    res = lowrank.PivotedCholesky(np.arange(3), SimpleNamespace(shape=(10, 3)), np.zeros(10), np.ones(4), 3)
    y = np.zeros(10)
    with pytest.raises(TypeError):
        lowrank.woodbury_fit(object(), y, 1e-3)
    for bad_y in (np.zeros(9), np.zeros((10, 49)), np.zeros((10, 0)), np.zeros((2, 5, 1))):
        with pytest.raises(ValueError):
            lowrank.woodbury_fit(res, bad_y, 1e-3)
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lowrank.woodbury_fit(res, y, lam)
    with pytest.raises(ValueError):
        lowrank.woodbury_fit(res, y, 1e-3, fitc="yes")
    empty = lowrank.PivotedCholesky(np.arange(0), SimpleNamespace(shape=(10, 0)), np.zeros(10), np.ones(1), 0)
    with pytest.raises(ValueError):
        lowrank.woodbury_fit(empty, y, 1e-3)
    big = lowrank.PivotedCholesky(np.arange(5000), SimpleNamespace(shape=(6000, 5000)), np.zeros(6000), np.ones(5001), 5000)
    with pytest.raises(NotImplementedError):
        lowrank.woodbury_fit(big, np.zeros(6000), 1e-3)
