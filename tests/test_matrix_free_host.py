"""Matrix-free exact GP, host side: the NumPy restatement of the block PCG (tests/_pcg_rules.py) against a dense solve on the
reference kernels, the three conditions the GPU tests lean on, and every refusal of the Python surface that needs no device.

  1. the restated PCG against numpy.linalg.solve, with and without the preconditioner, several right-hand sides, a zero
     column and a warm start;
  2. on the reference kernel with n = 130 / 300 / 1000, d = 7, eps = 1e-2, tol = 1e-8: a rank-n preconditioner converges in one
     iteration; rank 32 needs at most half the unpreconditioned iterations; the iteration counts at 4 tol, tol and tol / 4 are
     ordered (the window the device's count must fall into);
  3. lowrank.kernel_matmul / lowrank.pcg_solve / IterativeSPR: ValueError / NotImplementedError / TypeError before any device
     call."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _pchol_rules as PR
import _pcg_rules as CG
from oracle import nngp_oracle as O

HP = dict(w_std=1.3, b_std=0.2, last_w_std=0.9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * np.exp(0.5 * rng.standard_normal((n, 1)))


def problem(n, d=7, eps=1e-2, c=3, seed=0):
    x = data(n, d, seed)
    K = np.asarray(O.mlp_kernel(x, None, num_hiddens=2, act="relu", **HP), dtype=np.float64)
    lam = eps * np.trace(K) / n
    rng = np.random.default_rng(seed + 11)
    b = np.stack([np.sin(x[:, 0])] + [rng.standard_normal(n) for _ in range(c - 1)], axis=1)
    return SimpleNamespace(n=n, x=x, K=K, lam=lam, b=b)


@pytest.fixture(scope="module", params=[130, 300, 1000])
def prob(request):
    return problem(request.param)


def test_restated_pcg_matches_a_dense_solve(prob):
    K, lam, b, n = prob.K, prob.lam, prob.b, prob.n
    ref = np.linalg.solve(K + lam * np.eye(n), b)
    L = PR.pivoted_cholesky(K, 32).L
    for fac in (None, L):
        r = CG.pcg(K, b, lam, fac, tol=1e-10, max_iter=2000)
        assert r.info == 0 and (r.resid <= 2e-10).all()
        for k in range(b.shape[1]):
            bound = np.linalg.norm(b[:, k] - (K @ r.x[:, k] + lam * r.x[:, k])) / lam + 1e-12 * np.linalg.norm(ref[:, k])
            assert np.linalg.norm(r.x[:, k] - ref[:, k]) <= bound
        assert r.history.shape == (r.iters + 1, b.shape[1]) and (r.history[0] == 1.0).all()
        assert r.iters == r.col_iters.max()


def test_zero_column_warm_start_and_max_iter(prob):
    K, lam, n = prob.K, prob.lam, prob.n
    b = prob.b.copy()
    b[:, 1] = 0.0
    r = CG.pcg(K, b, lam, None, tol=1e-8)
    assert r.info == 0 and (r.x[:, 1] == 0.0).all() and r.col_iters[1] == 0 and r.resid[1] == 0.0
    again = CG.pcg(K, b, lam, None, tol=1e-6, x0=r.x)
    assert again.iters == 0 and again.info == 0 and np.array_equal(again.x, r.x)
    short = CG.pcg(K, b, lam, None, tol=1e-8, max_iter=2)
    assert short.info == 1 and short.iters == 2 and np.isfinite(short.x).all()


def test_the_three_conditions_of_the_gpu_tests(prob):
    K, lam, b, n = prob.K, prob.lam, prob.b, prob.n
    tol = 1e-8
    plain = CG.pcg(K, b, lam, None, tol=tol, max_iter=5000)
    full = CG.pcg(K, b, lam, PR.pivoted_cholesky(K, n).L, tol=tol)
    r32 = CG.pcg(K, b, lam, PR.pivoted_cholesky(K, 32).L, tol=tol, max_iter=5000)
    assert plain.info == full.info == r32.info == 0
    assert full.iters == 1, full.iters
    assert 2 * r32.iters <= plain.iters, (r32.iters, plain.iters)
    lo = CG.pcg(K, b, lam, None, tol=4 * tol, max_iter=5000)
    hi = CG.pcg(K, b, lam, None, tol=tol / 4, max_iter=5000)
    assert (lo.col_iters <= plain.col_iters).all() and (plain.col_iters <= hi.col_iters).all()
    assert lo.iters >= 1 and hi.info == 0


def test_float32_yardstick_is_a_perturbation():
    p = problem(130)
    r32 = CG.pcg(p.K, p.b, p.lam, None, tol=1e-4, round_to=np.float32, max_iter=1000)
    # the true residual leaves the recurrence's by at most iters u cond(K~) <= 1000 * 2^-24 * (1 + 1 / eps) = 6e-3
    assert r32.info == 0 and (r32.resid <= 1e-4 + 6e-3).all()


def test_limits_match_the_header():
    from smnngp import _lib
    src = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    assert int(re.search(r"#define SMN_MATMUL_SPLIT (\d+)", src).group(1)) == _lib.MATMUL_SPLIT
    assert _lib.MATMUL_SPLIT % 128 == 0
    assert int(re.search(r"#define SMN_MATMUL_PASS (\d+)", src).group(1)) == _lib.MATMUL_PASS
    assert 16 <= _lib.MATMUL_PASS <= 64 and _lib.PCG_MAX_COLS == 48


# ---------------------------------------------------------------- refusals without a device
def _kfn():
    from smnngp import nt_kernels
    return nt_kernels.get_mlp_kernel(2, act="relu", w_std=1.0, b_std=0.5, last_w_std=1.0)


def test_kernel_matmul_checks_its_arguments_before_the_device():
    from smnngp import lowrank, nt_kernels
    k = _kfn()
    x, v = np.zeros((10, 3)), np.zeros((10, 2))
    with pytest.raises(NotImplementedError):
        lowrank.kernel_matmul(nt_kernels.get_cnn_kernel(1), np.zeros((4, 3, 3, 1)), None, np.zeros(4))
    with pytest.raises(NotImplementedError):
        lowrank.kernel_matmul(lambda a, b: None, x, None, v)
    for bad_v in (np.zeros(9), np.zeros((9, 2)), np.zeros((10, 0)), np.zeros((10, 2, 1))):
        with pytest.raises(ValueError):
            lowrank.kernel_matmul(k, x, None, bad_v)
    with pytest.raises(ValueError):
        lowrank.kernel_matmul(k, x, np.zeros((7, 4)), np.zeros(7))            # feature dimensions differ
    with pytest.raises(ValueError):
        lowrank.kernel_matmul(k, x, np.zeros((7, 3)), np.zeros(10))           # v has the rows of x2
    with pytest.raises(ValueError):
        lowrank.kernel_matmul(k, x, np.zeros((7, 3)), np.zeros(7), shift=0.5)  # shift: the symmetric form only
    for shift in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lowrank.kernel_matmul(k, x, None, v, shift=shift)
    with pytest.raises(ValueError):
        lowrank.kernel_matmul(k, np.zeros(10), None, np.zeros(10))


def test_pcg_solve_checks_its_arguments_before_the_device():
    from smnngp import lowrank, nt_kernels
    k = _kfn()
    x, b = np.zeros((10, 3)), np.ones(10)
    with pytest.raises(NotImplementedError):
        lowrank.pcg_solve(nt_kernels.get_cnn_kernel(1), np.zeros((10, 3, 3, 1)), b, 1e-2)
    with pytest.raises(TypeError):
        lowrank.pcg_solve(k, x, b, 1e-2, precond=object())
    res = lowrank.PivotedCholesky(np.arange(3), SimpleNamespace(shape=(9, 3)), np.zeros(9), np.ones(4), 3)
    with pytest.raises(ValueError):
        lowrank.pcg_solve(k, x, b, 1e-2, precond=res)                         # factor rows != N
    big = lowrank.PivotedCholesky(np.arange(5000), SimpleNamespace(shape=(6000, 5000)), np.zeros(6000), np.ones(5001), 5000)
    with pytest.raises(NotImplementedError):
        lowrank.pcg_solve(k, np.zeros((6000, 3)), np.ones(6000), 1e-2, precond=big)
    for bad_b in (np.zeros(9), np.zeros((10, 0)), np.zeros((2, 5, 1))):
        with pytest.raises(ValueError):
            lowrank.pcg_solve(k, x, bad_b, 1e-2)
    with pytest.raises(NotImplementedError):
        lowrank.pcg_solve(k, x, np.zeros((10, 49)), 1e-2)
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lowrank.pcg_solve(k, x, b, lam)
    for tol in (0.0, 1.0, -1e-3, float("nan")):
        with pytest.raises(ValueError):
            lowrank.pcg_solve(k, x, b, 1e-2, tol=tol)
    with pytest.raises(ValueError):
        lowrank.pcg_solve(k, x, b, 1e-2, max_iter=0)
    with pytest.raises(ValueError):
        lowrank.pcg_solve(k, x, b, 1e-2, x0=np.zeros((10, 2)))


def _model_args():
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.5, 1.0)
    return kernel, GaussianLikelihood(), np.zeros((10, 3)), np.zeros(10), 0.0, 1.0


@pytest.mark.parametrize("kw", [dict(rank=-1), dict(rank=2.5), dict(rank=True), dict(rank=4097), dict(tol=0.0), dict(tol=1.0),
                                dict(tol=float("nan")), dict(max_iter=0), dict(max_iter=1.5)],
                         ids=lambda kw: "-".join("%s=%s" % it for it in kw.items()))
def test_iterative_spr_bad_arguments_raise_value_error(kw):
    from smnngp.spax.models import IterativeSPR
    with pytest.raises(ValueError):
        IterativeSPR(*_model_args(), **kw)


def test_iterative_spr_refusals_touch_no_device():
    from smnngp.spax.models import IterativeSPR
    kernel, lik, x, y, ym, ys = _model_args()
    with pytest.raises(ValueError):
        IterativeSPR(kernel, lik, x, np.zeros(9), ym, ys)
    with pytest.raises(ValueError):
        IterativeSPR(kernel, lik, np.zeros(10), y, ym, ys)
    with pytest.raises(NotImplementedError):
        IterativeSPR(kernel, object(), x, y, ym, ys)                   # a likelihood without lml_params
    with pytest.raises(TypeError):
        IterativeSPR.from_model(object())
    bare = IterativeSPR.__new__(IterativeSPR)                          # the methods that do not exist touch nothing
    for call in (bare.loss, bare.loss_and_grad, bare.loo_loss, bare.loo_predict, bare.loo_loss_and_grad, bare.posterior,
                 lambda: bare.sample_posterior(0, x, 2)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "LowRankSPR" in str(e.value) and "SPR" in str(e.value)
    for kw in (dict(chunk=0), dict(var_block=0), dict(var_block=49)):
        with pytest.raises(ValueError):
            bare.predict(x, **kw)
