"""Block preconditioned conjugate gradients on (K + lam I) X = B in NumPy fp64: the rule smn_pcg_solve follows, restated (a
helper, not a test module).

c independent recurrences, one alpha and one beta per column; a column stops when |r_k| <= tol |b_k| (recurrence residual) and
is frozen from then on; a zero b_k has x_k = 0 at iteration 0.  The preconditioner is M = L L^T + lam I by the Woodbury identity,
M^-1 r = (r - L (lam I + L^T L)^-1 L^T r) / lam.  `round_to` (np.float32) rounds K and the operand of every K-apply to that type:
the same-precision yardstick of the fp32 device solve, whose vectors and inner products stay fp64 as the device's do.
info: 0 every column stopped on tol, 1 max_iter reached, 2 breakdown (p^T K~ p <= 0 or a scalar that is not finite)."""
from types import SimpleNamespace

import numpy as np


def preconditioner(L, lam):
    """r -> M^-1 r for M = L L^T + lam I (L None or with no columns: r / lam)."""
    if L is None or L.shape[1] == 0:
        return lambda r: r / lam
    L = np.asarray(L, np.float64)
    C = np.linalg.cholesky(lam * np.eye(L.shape[1]) + L.T @ L)

    def apply(r):
        s = np.linalg.solve(C.T, np.linalg.solve(C, L.T @ r))
        return (r - L @ s) / lam
    return apply


def pcg(K, b, lam, L=None, tol=1e-6, max_iter=1000, x0=None, round_to=None):
    K = np.asarray(K, np.float64)
    b = np.asarray(b, np.float64)
    b = b.reshape(-1, 1) if b.ndim == 1 else b
    n, c = b.shape
    if round_to is not None:
        K = K.astype(round_to).astype(np.float64)
    kapply = (lambda v: K @ v) if round_to is None else (lambda v: K @ v.astype(round_to).astype(np.float64))
    minv = preconditioner(L, lam)
    x = np.zeros((n, c)) if x0 is None else np.array(x0, np.float64).reshape(n, c)
    bnorm = np.sqrt((b * b).sum(0))
    nz = bnorm > 0
    x[:, ~nz] = 0.0
    r = np.where(nz, b - (kapply(x) + lam * x), 0.0) if x0 is not None else b.copy()
    rnorm = np.sqrt((r * r).sum(0))
    hist = [np.where(nz, rnorm / np.where(nz, bnorm, 1.0), 0.0)]
    active = nz & ~(rnorm <= tol * bnorm)
    col_iters = np.zeros(c, dtype=np.int64)
    it, info = 0, 0
    z = minv(r)
    p = z.copy()
    rz = (r * z).sum(0)
    while active.any() and it < max_iter:
        it += 1
        a = np.flatnonzero(active)
        w = np.zeros((n, c))
        w[:, a] = kapply(p[:, a]) + lam * p[:, a]
        pw = (p * w).sum(0)
        alpha = np.zeros(c)
        with np.errstate(all="ignore"):
            alpha[a] = rz[a] / pw[a]
        if not (pw[a] > 0).all() or not np.isfinite(alpha[a]).all():
            info = 2
            break
        x[:, a] += alpha[a] * p[:, a]
        r[:, a] -= alpha[a] * w[:, a]
        rnorm = np.sqrt((r * r).sum(0))
        hist.append(np.where(nz, rnorm / np.where(nz, bnorm, 1.0), 0.0))
        done = active & (rnorm <= tol * bnorm)
        col_iters[done] = it
        active &= ~done
        if not active.any() or it == max_iter:
            break
        a = np.flatnonzero(active)
        z = minv(r)
        rz_new = (r * z).sum(0)
        beta = np.zeros(c)
        beta[a] = rz_new[a] / rz[a]
        rz = rz_new
        p[:, a] = z[:, a] + beta[a] * p[:, a]
    col_iters[active] = it
    if info == 2:
        return SimpleNamespace(x=np.full((n, c), np.nan), iters=it, col_iters=col_iters, resid=np.full(c, np.nan),
                               history=np.array(hist), info=2)
    true = b - (kapply(x) + lam * x)
    resid = np.where(nz, np.sqrt((true * true).sum(0)) / np.where(nz, bnorm, 1.0), 0.0)
    return SimpleNamespace(x=x, iters=it, col_iters=col_iters, resid=resid, history=np.array(hist),
                           info=1 if active.any() else 0)
