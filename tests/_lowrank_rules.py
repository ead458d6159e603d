"""Regression on a rank-M factor (csrc/lowrank.hip), restated in fp64 NumPy (test infrastructure).

The model covariance is K^ = L L^T + D, D = diag(d), d_i = fitc max(resid_i, 0) + lam, with L [N, M] a pivoted-Cholesky factor,
R = L[pivots] (lower triangular, K(Z, Z) = R R^T) and, at test points, kzt [M, T] = K(Z, x*), ktt [T] = K(x*, x*).

dense(...)     forms K^ and solves with it: quad_k = y_k^T K^^-1 y_k, logdet = log|K^|, and the DTC / FITC predictive
               phi = R^-1 kzt,  q = L phi [N, T],  mean = q^T K^^-1 Y,  var = ktt - diag(q^T K^^-1 q).
woodbury(...)  the device's steps: W = D^-1, G = L^T W L, B = L^T W Y, s_k = sum w y_k^2, A = I + G = C C^T,
               quad_k = s_k - |C^-1 B_k|^2, logdet = log|A| + sum log d, beta = A^-1 B, mean = phi^T beta,
               var = ktt - |phi|^2 + |C^-1 phi|^2.
               dtype=np.float32 is the same-precision yardstick of the device's f32 results: L, Y, kzt, ktt as float32 holds
               them, G accumulated in float32 over splits of `split` rows (the weight rounded to float32, w l rounded, a float32
               product per split) and the splits added in fp64; B, s and the whole M x M side in fp64, as on the device; mean and
               var rounded to float32 as the device stores them.
               Float32 has many admissible orders for the sums inside a split, and the error of ONE of them is a random number
               that can come out near zero; order = 0 .. ORDERS - 1 selects one of four (one product per split; the rows of a
               split reversed; the rows dealt into 7 interleaved passes; four rows at a time, accumulated in sequence, as a
               16x16x4 MFMA steps through them).  yardstick() is the largest error over the four."""
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla


def weights(resid, lam, fitc, n):
    """d [N]: the diagonal of D."""
    r = np.zeros(n) if (resid is None or not fitc) else np.maximum(np.asarray(resid, dtype=np.float64), 0.0)
    return r + float(lam)


def _cols(y):
    y = np.asarray(y, dtype=np.float64)
    return y[:, None] if y.ndim == 1 else y


def dense(L, resid, lam, fitc, y, R=None, kzt=None, ktt=None):
    L, Y = np.asarray(L, dtype=np.float64), _cols(y)
    n = L.shape[0]
    d = weights(resid, lam, fitc, n)
    cf = sla.cho_factor(L @ L.T + np.diag(d), lower=True)
    out = SimpleNamespace(quad=np.einsum("ik,ik->k", Y, sla.cho_solve(cf, Y)), logdet=2.0 * float(np.log(np.diag(cf[0])).sum()),
                          mean=None, var=None)
    if kzt is not None:
        phi = sla.solve_triangular(np.asarray(R, dtype=np.float64), np.asarray(kzt, dtype=np.float64), lower=True)
        q = L @ phi
        sq = sla.cho_solve(cf, q)
        out.mean = q.T @ sla.cho_solve(cf, Y)
        out.var = np.asarray(ktt, dtype=np.float64) - np.einsum("it,it->t", q, sq)
    return out


ORDERS = 4


def _split_product(a, b, order):
    """a^T b in float32 for one split, in summation order `order`."""
    if order == 0:
        return a.T @ b
    if order == 1:
        return a[::-1].T @ b[::-1]
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    if order == 2:
        for p in range(7):
            acc = acc + a[p::7].T @ b[p::7]
        return acc
    for j in range(0, a.shape[0], 4):
        acc = acc + a[j:j + 4].T @ b[j:j + 4]
    return acc


def gram(L, w, y, dtype=np.float64, split=512, order=0):
    """(G, B, s) in fp64 from L and Y as `dtype` holds them; float32: G by float32 splits, see the module docstring."""
    dt = np.dtype(dtype)
    Ls = np.asarray(L, dtype=np.float64).astype(dt)
    Ys = _cols(y).astype(dt).astype(np.float64)
    n = Ls.shape[0]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    L64 = Ls.astype(np.float64)
    if dt == np.float64:
        G = (L64 * w[:, None]).T @ L64
    else:
        G = np.zeros((Ls.shape[1],) * 2)
        for a in range(0, n, split):
            blk = Ls[a:a + split]
            G += _split_product(w[a:a + split].astype(dt)[:, None] * blk, blk, order).astype(np.float64)
        G = np.tril(G) + np.tril(G, -1).T
    return G, L64.T @ (w[:, None] * Ys), np.einsum("i,ik,ik->k", w, Ys, Ys)


def woodbury(L, resid, lam, fitc, y, R=None, kzt=None, ktt=None, dtype=np.float64, split=512, order=0):
    dt = np.dtype(dtype)
    n, m = np.shape(L)
    d = weights(resid, lam, fitc, n)
    G, B, s = gram(L, 1.0 / d, y, dt, split, order)
    A = np.eye(m) + G
    C = sla.cholesky(A, lower=True)
    Z = sla.solve_triangular(C, B, lower=True)
    out = SimpleNamespace(quad=s - np.einsum("jk,jk->k", Z, Z), logdet=2.0 * float(np.log(np.diag(C)).sum()) + float(np.log(d).sum()),
                          beta=sla.solve_triangular(C.T, Z, lower=False), C=C, G=G, mean=None, var=None)
    if kzt is not None:
        k = np.asarray(kzt, dtype=np.float64).astype(dt).astype(np.float64)
        phi = sla.solve_triangular(np.asarray(R, dtype=np.float64), k, lower=True)
        psi = sla.solve_triangular(C, phi, lower=True)
        out.mean = (phi.T @ out.beta).astype(dt).astype(np.float64)
        out.var = (np.asarray(ktt, dtype=np.float64).astype(dt).astype(np.float64) - np.einsum("it,it->t", phi, phi)
                   + np.einsum("it,it->t", psi, psi)).astype(dt).astype(np.float64)
    return out


def yardstick(L, resid, lam, fitc, y, R, kzt, ktt, split, quantities):
    """{name: the largest error, over the four float32 orders, of quantity `name` of the float32 run against the fp64 run on the
    same stored inputs}; quantities: {name: function of a woodbury() result}."""
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    ref = woodbury(f32(L), resid, lam, fitc, f32(_cols(y)), R, f32(kzt), f32(ktt))
    out = {k: 0.0 for k in quantities}
    for order in range(ORDERS):
        run = woodbury(L, resid, lam, fitc, y, R, kzt, ktt, dtype=np.float32, split=split, order=order)
        for k, f in quantities.items():
            out[k] = max(out[k], float(np.abs(np.asarray(f(run)) - np.asarray(f(ref))).max()))
    return out


def gp_logpdf(quad, logdet, n):
    return -0.5 * quad - 0.5 * n * np.log(2.0 * np.pi) - 0.5 * logdet


def tp_logpdf(quad, logdet, n, df, scale):
    """Zero-mean multivariate t with shape matrix scale * cov, from quad = y^T cov^-1 y and logdet = log|cov|."""
    from scipy.special import gammaln
    t = 0.5 * (df + n)
    return (-t * np.log1p(quad / scale / df) - 0.5 * n * np.log(df * np.pi) + gammaln(t) - gammaln(0.5 * df)
            - 0.5 * (logdet + n * np.log(scale)))
