"""NumPy fp64 rules for removing training points from a fitted posterior (FittedPosterior.remove, smn_fit_remove).

The state holds L (n x n, lower), L L^T = K~ = K(X, X) + lam I, and beta = L^-1 Y.  With J the removed rows, R the kept ones in
their order and H = L[R, :], H H^T = K~_RR and Y_R = H beta: any orthogonal Q with H Q = [L' 0] (L' lower, positive diagonal)
gives the factor of the kept points at the SAME lam and beta' = L'^-1 Y_R as the first n - k entries of Q^T beta.  `blocked_remove`
restates how the device forms Q: the window starts at j1 = min J rounded down to the block size b; there new row i ends at column
i + r(i), r(i) <= k the removed rows above it; block s (new rows [s, s + b)) is non-zero in columns [s, s + b + k) only, the LQ
factorisation of that block gives Q_s (sign flips folded in), Q_s goes to those columns of every row below and of the beta rows,
and the k columns behind the block carry into the next step.  More than KMAX rows go in passes of KMAX from the highest indices
down (`passes`).  Tolerances, data and kernels are those of _fit_append_rules.py, imported unchanged by the tests."""
import numpy as np

B, KMAX = 64, 32   # the device's block size and rows per pass (csrc/fit_remove.hip)


def normalise(idx, n):
    return sorted(int(i) % n for i in idx)


def passes(idx, kmax=KMAX):
    """The sorted index set as the device's passes: chunks of at most kmax from the highest indices down (indices of what is
    still to go do not move)."""
    idx = sorted(idx)
    out = []
    while idx:
        out.append(idx[-kmax:])
        idx = idx[:-kmax]
    return out


def blocked_remove(L, beta, idx, b=B, staircase=None):
    """(L', beta') after removing the rows idx (distinct, in [0, n)) from (L [n, n] lower, beta [n, c]) in ONE pass of the blocked
    LQ sweep.  staircase: a list that receives, per block, the largest |entry| right of column s + b + k of its rows (the rules
    say it is exactly 0).  Removing exactly the last k rows is the leading block of the factor, untouched."""
    n, k = L.shape[0], len(idx)
    gone = sorted(idx)
    keep = np.setdiff1d(np.arange(n), gone)
    m = n - k
    if gone == list(range(m, n)):                              # the suffix path: no arithmetic touches L
        return np.tril(L)[:m, :m].copy(), beta[:m].copy()
    h = np.vstack([np.tril(L)[keep], beta.T])                 # gather: the kept rows, then the beta rows
    w0 = gone[0] // b * b
    for s in range(w0, m, b):
        e, hi = min(s + b, m), min(min(s + b, m) + k, n)
        if staircase is not None:
            staircase.append(float(np.abs(h[s:e, hi:]).max()) if hi < n else 0.0)
        q, r = np.linalg.qr(h[s:e, s:hi].T, mode="complete")   # block^T = q r  =>  block q = r^T, lower trapezoidal
        sign = np.where(np.diag(r) < 0.0, -1.0, 1.0)
        q[:, :e - s] *= sign                                   # the sign fix: diag L' > 0
        h[s:, s:hi] = h[s:, s:hi] @ q                          # the block itself, every row below, the beta rows
        h[s:e, s:hi] = np.tril(h[s:e, s:hi])                   # exact zeros where the block became zero
    return h[:m, :m], h[m:, :m].T


def remove(L, beta, idx, b=B, kmax=KMAX):
    """`blocked_remove` pass by pass, as the device goes."""
    for chunk in passes(idx, kmax):
        L, beta = blocked_remove(L, beta, chunk, b)
    return L, beta


def index_sets(n0):
    """The index sets of the removal tests at n0 training points (name -> list)."""
    sets = {
        "first": [0],
        "last": [n0 - 1],
        "straddle_tile": [127, 128],
        "spread": sorted({0, 5, 129, n0 - 1}),                               # (three rows at n0 = 130)
        "every_7th": list(range(0, n0, 7)),
        "kmax_plus_1": list(range(3, 3 + 3 * (KMAX + 1), 3)),            # one row more than a pass takes
    }
    if n0 == 130:
        sets["to_127"] = [1, 64, 128]                                     # the last tile row becomes all padding
    return sets
