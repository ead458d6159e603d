"""The greedy pivoted Cholesky of csrc/pchol.hip, restated in NumPy on a stored matrix (test infrastructure).

State: L [N, M] in the storage dtype, resid [N] in fp64, r_i = K_ii - sum_t L_it^2.  Step j with pivot p:
    l_i = (K_ip - sum_{t<j} L_it L_pt) / sqrt(r_p)   (fp64),   L_ij = l_i rounded to the storage dtype,   r_i <- r_i - L_ij^2
    L_pj = sqrt(r_p), r_p = 0;  a row whose residual is exactly 0 gets L_ij = 0 and stays at 0.
Next pivot: argmax r_i, ties to the lowest index (numpy.argmax returns the first maximum).  Trace: sum_i max(r_i, 0).
Stop before step j when trace_j <= tol * trace_0 or max_i r_i <= noise_floor(j): 4 (j + 1) eps max_i K_ii (eps of the storage
dtype), which does not depend on N.

dtype=np.float32 runs the same steps with K and L rounded to float32 (sums and residuals stay fp64, as on the device): the
same-precision yardstick of the device's f32 results.  pivots=[...] forces the pivot order (then neither stopping rule applies,
and a forced pivot whose residual is not positive ends the run)."""
from types import SimpleNamespace

import numpy as np


def noise_floor(j, dtype, dmax):
    """The residual below which step j does not run: the rounding noise of a residual computed from j stored columns."""
    return 4.0 * (j + 1) * float(np.finfo(np.dtype(dtype)).eps) * max(float(dmax), 0.0)


def pivoted_cholesky(K, max_rank, tol=0.0, dtype=np.float64, pivots=None, keep_resid=False):
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    assert K.shape == (n, n) and 1 <= max_rank <= n and tol >= 0.0
    dt = np.dtype(dtype)
    Ks = K.astype(dt).astype(np.float64)            # the matrix as the storage dtype holds it
    L = np.zeros((n, max_rank), dtype=np.float64)   # values as stored (every entry is representable in dt)
    resid = np.diag(Ks).copy()
    dmax = resid.max()
    trace = [float(np.maximum(resid, 0.0).sum())]
    piv, hist, gaps = [], [], []
    for j in range(max_rank):
        if keep_resid:
            hist.append(resid.copy())
        if pivots is None:
            p = int(np.argmax(resid))
            if not resid[p] > noise_floor(j, dt, dmax) or trace[-1] <= tol * trace[0]:
                break
            top = np.sort(resid)[-2:]
            gaps.append(float(top[-1] - top[0]) if n > 1 else np.inf)
        else:
            if j >= len(pivots):
                break
            p = int(pivots[j])
            if not resid[p] > 0.0:
                break
        rp = resid[p]
        l = (Ks[:, p] - L[:, :j] @ L[p, :j]) / np.sqrt(rp)
        l[resid == 0.0] = 0.0
        l[p] = np.sqrt(rp)
        l = l.astype(dt).astype(np.float64)
        L[:, j] = l
        new = resid - l * l
        new[resid == 0.0] = 0.0
        new[p] = 0.0
        resid = new
        piv.append(p)
        trace.append(float(np.maximum(resid, 0.0).sum()))
    rank = len(piv)
    L[:, rank:] = 0.0
    return SimpleNamespace(pivots=np.asarray(piv, dtype=np.int64), L=L[:, :rank], resid=resid, trace=np.asarray(trace),
                           rank=rank, resid_hist=hist, gaps=np.asarray(gaps), dmax=float(dmax))


def conditional_residuals(K, pivots):
    """r^(j) = diag(K) - diag(K[:, P_j] K[P_j, P_j]^-1 K[P_j, :]) for P_j = pivots[:j], j = 0 .. len(pivots), in fp64 through the
    rules with the pivot order forced: [len(pivots) + 1, N] (the run ends early, with fewer rows, at a non-positive pivot)."""
    r = pivoted_cholesky(K, max(1, len(pivots)), pivots=list(pivots), keep_resid=True)
    return np.asarray(r.resid_hist[:r.rank] + [r.resid])
