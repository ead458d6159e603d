"""The gradient of the low-rank model's log-marginal likelihood at FIXED pivots (csrc/lowrank_grad.hip), restated in NumPy
(test infrastructure; not a test module).  Two independent forms:

formula(...)   the closed form the device evaluates.  With P the pivots, Z = X[P], L [n, m], R = L[P], d_i = fitc max(resid_i, 0)
               + lam, W = diag(1 / d), A = I + L^T W L = C C^T, beta = A^-1 L^T W Y, alpha = W (Y - L beta), h_i = |C^-1 L_i^T|^2,
               kappa_i = w_i - w_i^2 h_i, g_i = coef |alpha_i|^2 - c kappa_i, mu_i = fitc [resid_i > 0]:
                   U = [coef alpha beta^T - c W L A^-1 - diag(mu g) L] R^-1
                   T = R^-T [coef beta beta^T - c (I - A^-1) - L^T diag(mu g) L] R^-1
                   terms_theta = 2 sum U_ia dK(x_i, z_a) - sum T_ab dK(z_a, z_b) + sum mu_i g_i dK(x_i, x_i),  terms_eps = sum g_i
               with dK / d(w_std, b_std, last_w_std) from the forward-mode rules of tests/_grad_probe_rules.py (entry_tangents).
               dtype=np.float32 is the same-precision yardstick run: L, U, K0 = X Z^T / d and the tangents as float32 holds them,
               the two Grams by float32 splits in summation order `order` (tests/_lowrank_rules.gram), everything m x m and every
               sum that crosses elements in fp64.
dense_fd(...)  forms K^(theta) = K_nP K_PP^-1 K_Pn + diag(mu (k - q)) + lam I from the oracle's kernel at the same pivots and the
               same mask mu, evaluates the log-pdf and takes central differences in fp64.  Shares nothing with formula() but the
               oracle kernel's name.
"""
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla
from scipy.special import gammaln

import _grad_probe_rules as GP
import _lowrank_rules as LR
from oracle import nngp_oracle as O

NAMES = ("w_std", "b_std", "last_w_std", "eps")


def oracle_kernel(net, act, layers, w_std, b_std, last_w_std, x):
    fn = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel}[net]
    return fn(np.asarray(x, dtype=np.float64), None, layers, act, w_std, b_std, last_w_std)


def tangents(net, act, layers, w_std, b_std, last_w_std, x, piv, T=np.float64):
    """(dKx [3, n, m], dKd [3, n]) in T: d K(x_i, z_a) and d K(x_i, x_i) / d(w_std, b_std, last_w_std); K0 = X X^T / d in T."""
    xs = np.asarray(x, dtype=np.float64).astype(T)
    n, d = xs.shape
    k0 = (xs @ xs.T) / T(d)
    q = np.diagonal(k0).copy()
    piv = np.asarray(piv, dtype=np.int64)
    m = piv.shape[0]
    i, j = np.repeat(np.arange(n), m), np.tile(piv, n)
    dkx = GP.entry_tangents(net, act, layers, w_std, b_std, last_w_std, k0, q, i, j, T).reshape(3, n, m)
    r = np.arange(n)
    dkd = GP.entry_tangents(net, act, layers, w_std, b_std, last_w_std, k0, q, r, r, T)
    return dkx.astype(np.float64), dkd.astype(np.float64)


def head(quad, logdet, n, c, df, scale):
    """(log-pdf, coef) of c target columns that share one covariance: Gaussian (df <= 0) or the joint multivariate t in
    dimension n c with shape scale K^ (quad: the sum over the columns)."""
    if df <= 0.0:
        return -0.5 * quad - 0.5 * n * c * np.log(2.0 * np.pi) - 0.5 * c * logdet, 1.0
    t = 0.5 * (df + n * c)
    lp = (-t * np.log1p(quad / scale / df) - 0.5 * n * c * np.log(df * np.pi) + gammaln(t) - gammaln(0.5 * df)
          - 0.5 * (c * logdet + n * c * np.log(scale)))
    return lp, (df + n * c) / ((df + quad / scale) * scale)


def formula(L, resid, piv, lam, fitc, y, coef, kern, dtype=np.float64, split=512, order=0, parts=None):
    """terms [4] and S [4] (the sum of the absolute contracted products of each term); kern = (net, act, layers, w_std, b_std,
    last_w_std, x).  parts: tangents(...) of the same dtype when the caller already has them."""
    dt = np.dtype(dtype).type
    Ls = np.asarray(L, dtype=np.float64).astype(dt).astype(np.float64)
    Y = LR._cols(y).astype(dt).astype(np.float64)
    n, m = Ls.shape
    c = Y.shape[1]
    piv = np.asarray(piv, dtype=np.int64)
    d = LR.weights(resid, lam, fitc, n)
    w = 1.0 / d
    mu = (np.asarray(resid) > 0.0).astype(np.float64) if fitc else np.zeros(n)
    R = np.tril(Ls[piv])
    G, B, _ = LR.gram(Ls, w, Y, dt, split, order)
    A = np.eye(m) + G
    C = sla.cholesky(A, lower=True)
    beta = sla.cho_solve((C, True), B)
    alpha = w[:, None] * (Y - Ls @ beta)
    h = np.sum(sla.solve_triangular(C, Ls.T, lower=True) ** 2, axis=0)
    kappa = w - w * w * h
    g = coef * np.sum(alpha * alpha, axis=1) - c * kappa
    mg = mu * g
    Ainv = sla.cho_solve((C, True), np.eye(m))
    V = coef * alpha @ beta.T - c * (w[:, None] * Ls) @ Ainv - mg[:, None] * Ls
    U = sla.solve_triangular(R.T, V.T, lower=False).T
    U = U.astype(dt).astype(np.float64)
    G2 = LR.gram(Ls, mg, np.zeros((n, 1)), dt, split, order)[0]
    Bk = coef * beta @ beta.T - c * (np.eye(m) - Ainv) - G2
    Tm = sla.solve_triangular(R.T, sla.solve_triangular(R.T, Bk, lower=False).T, lower=False)
    Tm = Tm.astype(dt).astype(np.float64)
    dkx, dkd = tangents(*kern, piv, T=dt) if parts is None else parts
    terms, S = np.zeros(4), np.zeros(4)
    for t in range(3):
        px, pz, pd = 2.0 * U * dkx[t], Tm * dkx[t][piv], mg * dkd[t]
        terms[t] = px.sum() - pz.sum() + pd.sum()
        S[t] = np.abs(px).sum() + np.abs(pz).sum() + np.abs(pd).sum()
    terms[3], S[3] = g.sum(), np.abs(g).sum()
    return terms, S


def yardstick32(L, resid, piv, lam, fitc, y, coef, kern, split=512):
    """(ref [4], S [4], yard [4]): the fp64 run on the float32-stored inputs, its S, and the largest error of the float32 run over
    the four summation orders, floored at u32 S."""
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    kern64 = kern[:6] + (f32(kern[6]),)
    ref, S = formula(f32(L), resid, piv, lam, fitc, f32(LR._cols(y)), coef, kern64)
    parts = tangents(*kern, piv, T=np.float32)
    yard = np.zeros(4)
    for order in range(LR.ORDERS):
        run, _ = formula(L, resid, piv, lam, fitc, y, coef, kern, dtype=np.float32, split=split, order=order, parts=parts)
        yard = np.maximum(yard, np.abs(run - ref))
    return ref, S, np.maximum(yard, 2.0 ** -24 * S)


# ---------------------------------------------------------------------------------------------------------------- dense form
def dense_cov(kern, piv, mu, lam):
    """K^ at fixed pivots and a fixed mask mu from the oracle's kernel."""
    K = oracle_kernel(*kern)
    piv = np.asarray(piv, dtype=np.int64)
    Knp = K[:, piv]
    cf = sla.cho_factor(K[np.ix_(piv, piv)], lower=True)
    Q = Knp @ sla.cho_solve(cf, Knp.T)
    return Q + np.diag(mu * (np.diagonal(K) - np.diagonal(Q))) + lam * np.eye(K.shape[0])


def dense_logpdf(kern, piv, mu, lam, y, df, scale):
    Y = LR._cols(y)
    n, c = Y.shape
    cf = sla.cho_factor(dense_cov(kern, piv, mu, lam), lower=True)
    quad = float(np.sum(Y * sla.cho_solve(cf, Y)))
    return head(quad, 2.0 * float(np.log(np.diag(cf[0])).sum()), n, c, df, scale)


def _bump(kern, lam, t, step):
    if t == 3:
        return kern, lam + step
    k = list(kern)
    k[3 + t] = k[3 + t] + step
    return tuple(k), lam


def dense_fd(kern, piv, mu, lam, y, df, scale, h=1e-5):
    """(terms [4] = 2 d logpdf / d(w_std, b_std, last_w_std, lam) by central differences with relative step h, S [4] =
    sum |G_ij dK^_ij| with G = coef alpha alpha^T - c K^^-1 and dK^ by the same differences, coef)."""
    Y = LR._cols(y)
    c = Y.shape[1]
    _, coef = dense_logpdf(kern, piv, mu, lam, y, df, scale)
    cov = dense_cov(kern, piv, mu, lam)
    kinv = np.linalg.inv(cov)
    al = kinv @ Y
    G = coef * al @ al.T - c * kinv
    terms, S = np.zeros(4), np.zeros(4)
    for t in range(4):
        v = lam if t == 3 else kern[3 + t]
        step = h * abs(v) if v != 0.0 else h
        up, dn = _bump(kern, lam, t, step), _bump(kern, lam, t, -step)
        terms[t] = 2.0 * (dense_logpdf(up[0], piv, mu, up[1], y, df, scale)[0]
                          - dense_logpdf(dn[0], piv, mu, dn[1], y, df, scale)[0]) / (2.0 * step)
        dcov = (dense_cov(up[0], piv, mu, up[1]) - dense_cov(dn[0], piv, mu, dn[1])) / (2.0 * step)
        S[t] = np.abs(G * dcov).sum()
    return terms, S, coef


def case(n, d, m, seed, net="mlp", act="relu", layers=2, w_std=1.3, b_std=0.4, last_w_std=0.9, c=1):
    """Fixed-seed inputs and the fp64 factor of the oracle's kernel at its greedy pivots (tests/_pchol_rules)."""
    import _pchol_rules as PR
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) * np.exp(0.3 * rng.standard_normal((n, 1)))
    y = np.sin(x[:, :1] * np.arange(1, c + 1)[None, :]) + 0.3 * rng.standard_normal((n, c))
    kern = (net, act, layers, w_std, b_std, last_w_std, x)
    r = PR.pivoted_cholesky(oracle_kernel(*kern), m)
    return SimpleNamespace(x=x, y=y, kern=kern, L=r.L[:, :r.rank], resid=r.resid, piv=r.pivots[:r.rank], rank=r.rank)
