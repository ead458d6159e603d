"""CPU-side checks of the posterior draws: the NumPy restatement of the chi-square mixing variate follows its law, the C ABI
declares, exports and binds the two new entries, the models carry the new methods, and every precondition the GPU tests of
tests/test_gpu_draws.py lean on holds for their cases (checked here, on the oracle, so that a GPU failure is the device's)."""
import os
import re

import numpy as np
import pytest

import _draws_rules as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAW_SYMBOLS = ("smn_rng_chi2", "smn_mvn_draws")


# ------------------------------------------------------------------------------------------- 1. the chi-square variate
@pytest.mark.parametrize("df", D.STAT_DFS)
def test_restated_chi2_follows_its_law(df):
    """S = 16384 draws: Kolmogorov-Smirnov D < 1.95 / sqrt(S), lag-1 correlation of the probability transform
    < 5 / sqrt(S) (the bounds of test_variates_follow_their_distribution_and_are_uncorrelated)."""
    s = D.STAT_DRAWS
    g = D.chi2(D.STAT_SEED, df, s)
    assert g.shape == (s,) and np.all(np.isfinite(g)) and np.all(g > 0)
    d, lag1 = D.chi2_statistics(g, df)
    print("chi2 df %g: KS D sqrt(S) = %.3f, lag-1 sqrt(S) = %.3f" % (df, d * np.sqrt(s), lag1 * np.sqrt(s)))
    assert d < 1.95 / np.sqrt(s)
    assert lag1 < 5 / np.sqrt(s)


def test_the_rules_product_is_the_dense_product():
    rng = np.random.default_rng(0)
    t, c, s = 7, 3, 5
    mean, lo, z, r = rng.standard_normal((t, c)), rng.standard_normal((t, t)), rng.standard_normal((t, c, s)), rng.random(s) + 0.5
    lo_nan = np.where(np.tri(t, dtype=bool), lo, np.nan)          # the strict upper triangle is never used
    got = D.draws(mean, lo_nan, z, r)
    for i in range(s):
        assert np.allclose(got[i], mean + r[i] * np.tril(lo) @ z[:, :, i], rtol=1e-13, atol=1e-13)
    assert np.all(D.error_bound(mean, lo_nan, z, r, np.float32) > 0)
    assert np.array_equal(D.scale_r(0.0, 3.0, np.ones(4)), np.ones(4))
    assert np.allclose(D.scale_r(4.0, 0.5, np.array([2.0])), 1.0)


# ------------------------------------------------------------------------------------------- 2. exports and methods
def test_header_declares_and_the_binding_binds_the_draw_entries():
    import ctypes

    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smnngp.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in DRAW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, "include/smnngp.h does not declare %s" % name
        assert name in _lib.PROTOTYPES, "_lib does not bind %s" % name
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name]), name
        assert hasattr(raw, name), "libsmnngp.so does not export %s" % name


def test_models_have_the_methods_and_the_gaussian_parameters_need_no_device():
    import __graft_entry__ as g
    g.build()
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    for cls in (SPR, MultiSPR):
        for name in ("predict", "predictive_params", "sample_posterior"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
        model = cls.__new__(cls)                  # no data, no context: the Gaussian answer reads the likelihood alone
        model.likelihood = GaussianLikelihood()
        assert model.predictive_params() == (None, 1.0)


# ------------------------------------------------------------------------------ the GPU tests' preconditions, on the CPU
@pytest.mark.parametrize("name", sorted(D.CASES))
def test_reference_draws_stay_inside_the_moment_cap(name):
    """GPU test 6c: the rules with NumPy's own normals on the oracle posterior miss at most 5 % of the entries."""
    mean, cov = D.oracle_posterior(name)
    cov = D.ridged(cov, D.MOMENT_JITTER)
    t, c = mean.shape
    z = np.random.default_rng(D.MOMENT_SEED).standard_normal((t, c, D.MOMENT_DRAWS))
    f = D.draws(mean, np.linalg.cholesky(cov), z, np.ones(D.MOMENT_DRAWS))
    total, miss = D.moment_misses(f, mean, cov)
    print("%s: %d of %d entries outside 5 sd / sqrt(S)" % (name, miss, total))
    assert miss <= 0.05 * total


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_covariance_at_the_training_points_without_ridge_does_not_factor(name):
    """GPU test 6e: test points = training points, eps tiny, no ridge: NumPy's Cholesky of the oracle covariance fails."""
    _, cov = D.oracle_posterior(name, hyp=dict(D.HYP, eps=D.TINY_EPS), at_training_points=True)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(cov)


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_fp32_cases_are_not_marginal(name):
    """GPU test 7: the smallest eigenvalue of cov + jitter tr/T I is above 100 T 2^-24 max diag."""
    _, cov = D.oracle_posterior(name, f32=True)
    t = cov.shape[0]
    lam = np.linalg.eigvalsh(D.ridged(cov, D.F32_JITTER))[0]
    floor = 100 * t * 2.0 ** -24 * np.max(np.diag(cov))
    print("%s: smallest eigenvalue %.3g, floor %.3g" % (name, lam, floor))
    assert lam > floor
