"""NumPy fp64 restatement of the posterior-draw entries (shared by test_draws_host.py and test_gpu_draws.py; not a test
module), written from include/smnngp.h:

    out[s,t,c] = mean[t,c] + r_s sum_{k<=t} L[t,k] xi[k,c,s]          r_s = sqrt(shape df / g_s),  g_s ~ chi2(df)

and the chi-square mixing variate g_s of (seed, s): chi2(df) = 2 Gamma(df / 2) by Marsaglia & Tsang on the Philox block
ctr = (s, 0, 0, 0xC0000000 | k), key = (seed low word, seed high word), try k = 0 .. 31.
"""
import functools
import math

import numpy as np

from oracle import nngp_oracle as O

from _svsp_rules import philox4x32_10

STAT_SEED = 20240229
STAT_DFS = (1.5, 4.0, 9.3, 76.0, 40004.0)      # 1.5 runs the boost branch
STAT_DRAWS = 16384

CHI2_STREAM = 0xC0000000
CHI2_TRIES = 32


def _unit(r):
    return (r + 0.5) * 2.0 ** -32


def chi2_variate(seed, s, df):
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    a = 0.5 * df
    boost = a < 1.0
    d = (a + 1.0 if boost else a) - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    for k in range(CHI2_TRIES):
        r = philox4x32_10((s, 0, 0, CHI2_STREAM | k), key)
        x = math.sqrt(-2.0 * math.log(_unit(r[0]))) * math.cos(2.0 * math.pi * _unit(r[1]))
        t = 1.0 + c * x
        if t <= 0.0:
            continue
        v = t * t * t
        if math.log(_unit(r[2])) < 0.5 * x * x + d - d * v + d * math.log(v):
            g = 2.0 * d * v
            return g * _unit(r[3]) ** (1.0 / a) if boost else g
    return df


@functools.lru_cache(maxsize=None)
def _chi2_cached(seed, df, num):
    out = np.array([chi2_variate(seed, s, df) for s in range(num)])
    out.setflags(write=False)
    return out


def chi2(seed, df, num):
    """The first `num` mixing variates of (seed, df), fp64 (computed once per process; read-only)."""
    return _chi2_cached(int(seed), float(df), int(num))


def chi2_statistics(g, df):
    """(Kolmogorov-Smirnov D against chi2(df), |lag-1 correlation| of the probability transform)."""
    from scipy import stats
    g = np.asarray(g, dtype=np.float64)
    dist = stats.chi2(df)
    d = stats.kstest(g, dist.cdf).statistic
    u = dist.cdf(g)
    a, b = u[:-1] - u[:-1].mean(), u[1:] - u[1:].mean()
    return float(d), abs(float(a @ b / np.sqrt((a @ a) * (b @ b))))


def scale_r(df, shape, g, dtype=np.float64):
    """r_s: 1 for df <= 0, else sqrt(shape df / g_s) formed in fp64 and rounded to dtype once; returned as fp64."""
    g = np.asarray(g, dtype=np.float64)
    if not df > 0:
        return np.ones(g.shape[0])
    return np.sqrt(shape * df / g).astype(dtype).astype(np.float64)


def draws(mean, L, Z, r):
    """mean [T,C], L [T,T] (lower triangle used), Z [T,C,S], r [S] -> [S,T,C], fp64."""
    mean, L, Z, r = (np.asarray(v, dtype=np.float64) for v in (mean, L, Z, r))
    return mean[None] + r[:, None, None] * np.einsum("tk,kcs->stc", np.tril(L), Z)


def error_bound(mean, L, Z, r, dtype):
    """(T + 8) u (|mean[t,c]| + r_s sum_k |L[t,k]| |Z[k,c,s]|), u the unit roundoff of dtype: the inner-product bound
    gamma_{T+8} in any summation order, with room for the rounding of r_s, the multiply and the add."""
    mean, L, Z, r = (np.asarray(v, dtype=np.float64) for v in (mean, L, Z, r))
    u = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    mag = np.abs(mean)[None] + r[:, None, None] * np.einsum("tk,kcs->stc", np.abs(np.tril(L)), np.abs(Z))
    return (L.shape[0] + 8) * u * mag


# ---------------------------------------------------------------- the model-level cases of the GPU tests
HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)      # tests/test_gpu_cnn_grad.py
LAYERS, ACT = 2, "relu"
CASES = {"spr": dict(family="mlp", n=40, t=12, c=1, shape=(5,)),
         "multi": dict(family="cnn", n=24, t=9, c=3, shape=(6, 6, 2))}
MOMENT_DRAWS, MOMENT_JITTER, MOMENT_SEED = 4096, 1e-8, 11
F32_JITTER = 1e-3
TINY_EPS = 1e-20      # the ridge of the case that must not factor


@functools.lru_cache(maxsize=None)
def case_data(name, f32=False):
    """(x [N,...], y [N,C], x_test [T,...]) of a case, fp64 values (rounded to fp32 first when f32); test points are
    drawn separately from the training points."""
    cs = CASES[name]
    rng = np.random.default_rng(len(name) + 100 * cs["n"])
    x = rng.standard_normal((cs["n"],) + cs["shape"])
    y = rng.standard_normal((cs["n"], cs["c"]))
    xt = rng.standard_normal((cs["t"],) + cs["shape"])
    if f32:
        x, y, xt = (v.astype(np.float32).astype(np.float64) for v in (x, y, xt))
    return x, y, xt


def oracle_kernel(name, x1, x2=None, hyp=HYP):
    kfn = O.mlp_kernel if CASES[name]["family"] == "mlp" else O.cnn_kernel
    return kfn(x1, x2, num_hiddens=LAYERS, act=ACT, w_std=hyp["w_std"], b_std=hyp["b_std"], last_w_std=hyp["last_w_std"])


def oracle_posterior(name, f32=False, hyp=HYP, at_training_points=False):
    """mean [T,C], cov [T,T] of NNGPKernel.predict (relative ridge eps) from the oracle kernels, fp64."""
    x, y, xt = case_data(name, f32)
    if at_training_points:
        xt = x
    return O.predict(oracle_kernel(name, x, None, hyp), oracle_kernel(name, xt, x, hyp), oracle_kernel(name, xt, None, hyp), y,
                     diag_reg=hyp["eps"])


def oracle_predictive_params(name, f32=False, hyp=HYP):
    """(df_post, shape) of the Student-t head: df_post = 2a + N C, shape = (2a + quad) / df_post * b/a with
    quad = tr(Y^T ((b/a) K + 1e-6 I)^-1 Y), K without eps (spax/likelihoods.py:52-65 in dimension N C)."""
    import scipy.linalg as sla
    x, y, _ = case_data(name, f32)
    n, c = y.shape
    df, scale = 2.0 * hyp["alpha"], hyp["beta"] / hyp["alpha"]
    khat = scale * oracle_kernel(name, x, None, hyp) + 1e-6 * np.eye(n)
    quad = float(np.sum(y * sla.cho_solve(sla.cho_factor(khat, lower=True), y)))
    df_post = df + n * c
    return df_post, (df + quad) / df_post * scale


def ridged(cov, jitter):
    cov = np.asarray(cov, dtype=np.float64)
    t = cov.shape[0]
    return cov + jitter * np.trace(cov) / t * np.eye(t)


def moment_misses(f, mean, cov):
    """f [S,T,C] Gaussian draws; mean [T,C], cov [T,T] (ridged) their law -> (entries checked, entries whose sample mean
    or per-output sample covariance is further than 5 sd / sqrt(S) from it).  sd: sqrt(cov_tt) for a mean, sqrt(cov_ii
    cov_jj + cov_ij^2) for a covariance entry (the Gaussian formulas)."""
    f = np.asarray(f, dtype=np.float64)
    s, t, c = f.shape
    dg = np.diag(cov)
    miss = int(np.sum(np.abs(f.mean(axis=0) - mean) > 5.0 * np.sqrt(dg)[:, None] / np.sqrt(s)))
    total = t * c
    sd = np.sqrt(np.outer(dg, dg) + cov * cov)
    for k in range(c):
        sc = np.cov(f[:, :, k], rowvar=False).reshape(t, t)
        miss += int(np.sum(np.abs(sc - cov) > 5.0 * sd / np.sqrt(s)))
        total += t * t
    return total, miss
