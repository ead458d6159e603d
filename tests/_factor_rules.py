"""Componentwise backward-error rules for smn_cholesky / smn_trsm (shared by test_factor_host.py and test_gpu_factor.py;
not a test module).  NumPy / SciPy only.  Every rule takes the arrays a factorisation returned, in their dtype, and does its
own arithmetic in fp64; u is the unit roundoff of that dtype (2^-24 or 2^-53).

    rho_factor  max_{i>=j} |A - L L^T|_ij / (u (|L||L^T|)_ij)                 leading n_factor block
    rho_rows    max        |B - W L^T| / (u |W||L^T|)                          appended rows, W = B L^-T
    rho_schur   max_{i>=j} |S - (C - W W^T)| / (u (|C| + |W||W^T|))            trailing block
    rho_trsm    max        |B - op(L) X| / (u |op(L)||X|)

Each is at most n_factor + 1 for ANY order of summation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
Thm 10.3 for the factor, Thm 8.5 for the substitutions, (3.5) for the inner products of the Schur block), and none depends on
the condition number.  A zero denominator counts as 0 under a zero numerator and as inf otherwise; a NaN counts as inf.

Above SAMPLE_ABOVE rows the rules evaluate one row of every 16-row group against all columns (sample_rows).

The reference of every GPU case is the same rule on LAPACK's result in the same precision on the same matrix
(lapack_factor: potrf, trsm, and the dtype product for the Schur block); references are computed once per process and
handed out read-only.
"""
import functools
import math

import numpy as np
import scipy.linalg as sla

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
SAMPLE_ABOVE = 2500
REF_FACTOR = 8.0          # rho_gpu <= REF_FACTOR * rho_lapack: blocked algorithms of different block shapes, MFMA accumulation
                          # that need not round as LAPACK's FMAs do, and LAPACK's own rho varying about 7-fold across cases
TILE = 128

# ----------------------------------------------------------------------------- cases
# (n_factor, m): default context
SHAPES_A = [(1, 0), (16, 0), (17, 3), (127, 0), (129, 1), (128, 0), (256, 128), (384, 0), (640, 128), (391, 37), (1025, 0),
            (1300, 77), (2305, 0), (1152, 0), (1024, 128), (4480, 0), (5120, 0)]
# (name, environment of the context, (n_factor, m), dtypes): schedules the default context takes only from n = 8192 on, or never
F32, F64 = np.float32, np.float64
SCHEDULES = [
    ("lookahead512", {"SMN_CHAIN_MIN_N": "1", "SMN_SUPER": "512"}, (1664, 128), (F32, F64)),
    ("lookahead512_wide", {"SMN_CHAIN_MIN_N": "1", "SMN_SUPER": "512", "SMN_SUPER_WIDE_ROWS": "1024"}, (1664, 128), (F32, F64)),
    ("lookahead_width_change", {"SMN_CHAIN_MIN_N": "1", "SMN_SUPER": "512", "SMN_SUPER_WIDE_ROWS": "1024"}, (2432, 128), (F32, F64)),
    ("super256", {"SMN_SUPER": "256"}, (640, 0), (F32, F64)),
    ("trail_kernel", {"SMN_SUPER": "2048", "SMN_CHAIN_CUS": "0"}, (5888, 0), (F32,)),
    ("panel_leaf0", {"SMN_PANEL_LEAF": "0"}, (1152, 128), (F32, F64)),
]
SHIFT_SHAPES = [(391, 37), (640, 128)]
SHIFT_COUNTS = [0, 1, 127, 300, None]                           # None: n_factor
SHIFT_KINDS = {"jitter": (0.5, 0.0), "ridge": (0.0, 0.25), "both": (0.5, 0.25)}
TRSM_SHAPES = [(1, 1), (129, 3), (333, 45), (1300, 130)]
# 1-based failing pivot p in (n_factor, m)
PIVOT_CASES = [(1, 300, 0), (16, 300, 0), (17, 300, 0), (128, 300, 0), (129, 300, 0), (257, 300, 0), (391, 391, 0),
               (1025, 1152, 128)]
PIVOT_LOOKAHEAD = (513, 1664, 128)
# one NaN at (i, j), i > j (0-based) in (n_factor, m): inside one sub-panel; across a super-panel edge (1024)
NAN_CASES = [(100, 37, 300, 0), (1100, 1000, 1152, 128)]


def unit(x):
    return U[np.dtype(x.dtype)]


@functools.lru_cache(maxsize=None)
def spd(n, seed, cond=1e3):
    """The suite's _spd: Q diag(geomspace(1, cond)) Q^T, fp64, read-only."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * np.geomspace(1.0, cond, n)) @ q.T
    a.setflags(write=False)
    return a


def upper_pattern(n):
    """What the tests upload strictly above the diagonal: negative, never zero, exact in fp32, different in every row and
    column of a tile."""
    i, j = np.triu_indices(n, 1)
    return i, j, -(((i * 31 + j * 17) % 1021) + 0.5)


def with_upper_pattern(a):
    a = np.array(a)
    i, j, v = upper_pattern(a.shape[0])
    a[i, j] = v.astype(a.dtype)
    return a


def upper_intact(a, got):
    i, j = np.triu_indices(a.shape[0], 1)
    return bool(np.array_equal(a[i, j], got[i, j]))


def matrix(n_factor, m, dtype):
    """The matrix of shape case (n_factor, m) as uploaded: lower triangle of _spd(cond=1e3) rounded to dtype, the pattern above."""
    n = n_factor + m
    return with_upper_pattern(spd(n, 1000 + n_factor + m).astype(dtype))


def shift_matrix(n_factor, m, n_shift, dtype):
    """Case E: the diagonal entries from n_shift on are 100 times larger (still positive definite: a positive diagonal was
    added), so a trace taken over more than the first n_shift entries moves the shift far outside the bound."""
    n = n_factor + m
    a = np.array(spd(n, 2000 + n_factor + m))
    idx = np.arange(n_shift, n)
    a[idx, idx] *= 100.0
    return with_upper_pattern(a.astype(dtype))


def shifted(a, n_shift, jitter_abs, ridge_rel, trace_over=None, also=()):
    """jitter_abs + ridge_rel tr/n added to the first n_shift diagonal entries of the dtype matrix `a`, in fp64, rounded to
    dtype once; the trace over the first n_shift entries.  trace_over / also: the damaged variants of the host tests (trace
    and division over another count; further diagonal entries shifted too)."""
    out = a.astype(np.float64)
    if n_shift > 0 and (jitter_abs != 0.0 or ridge_rel != 0.0):
        t = n_shift if trace_over is None else trace_over
        sh = jitter_abs + ridge_rel * math.fsum(np.diag(out)[:t]) / t
        idx = np.concatenate([np.arange(n_shift), np.asarray(also, dtype=np.int64)])
        out[idx, idx] += sh
    return out.astype(a.dtype)


def pivot_matrix(p, n_factor, m, dtype):
    """Case D: a_pp (1-based p) lowered by 1.5 max_i a_ii.  The leading minor of order p - 1 is untouched (positive definite).
    The pivot of order p is a_pp minus a non-negative quadratic form, so it started at most max_i a_ii and ends at or below
    -0.5 max_i a_ii: half the largest diagonal entry below zero, far from rounding.  (Lowering a_pp by 0.5 max_i a_ii alone
    leaves the early pivots of these matrices positive -- their diagonal is nearly constant -- and LAPACK then fails later.)"""
    n = n_factor + m
    a = np.array(spd(n, 3000 + n)).astype(dtype)
    a[p - 1, p - 1] = a[p - 1, p - 1] - dtype(1.5) * a.diagonal().max()
    return with_upper_pattern(a)


def nan_matrix(i, j, n_factor, m, dtype):
    n = n_factor + m
    a = with_upper_pattern(np.array(spd(n, 3000 + n)).astype(dtype))
    a[i, j] = np.nan
    return a


def trsm_case(n, nrhs, dtype):
    rng = np.random.default_rng(4000 + n + nrhs)
    l = with_upper_pattern(np.linalg.cholesky(spd(n, 4000 + n)).astype(dtype))      # (strictly upper: not part of L)
    b = rng.standard_normal((n, nrhs)).astype(dtype)
    return l, b


def trail_kernel_min_n(num_cu=256, super_panel=2048, outer=256, max_k=512):
    """Smallest n (multiple of 128, no appended rows, no look-ahead) whose first near update goes to trail_kernel: launch_update
    takes it for fp32 when tag == 1, the shape is a trapezoid or triangle without the XCD map (a trapezoid never has one),
    K <= kPersistMaxK (K = the outer panel's 256 columns) and nt > 2 * num_cu.  The first near update follows outer panel
    [0, 256): tiles_n = (super_panel - 256) / 128 columns, tiles_m = (n - 256) / 128 rows,
    nt = tiles_n (tiles_n + 1) / 2 + (tiles_m - tiles_n) tiles_n."""
    assert outer <= max_k
    n = super_panel
    while True:
        tn, tm = (super_panel - outer) // TILE, (n - outer) // TILE
        if tn * (tn + 1) // 2 + (tm - tn) * tn > 2 * num_cu:
            return n
        n += TILE


# ----------------------------------------------------------------------------- sampling
def sample_rows(n_total):
    """All rows up to SAMPLE_ABOVE; above, one row of every group of 16, its offset inside the group rotating with the group
    index (a last, short group gives its last row): every 16-row MFMA block row of every tile is hit, at n^3 / 8 flops."""
    if n_total <= SAMPLE_ABOVE:
        return np.arange(n_total)
    g = np.arange((n_total + 15) // 16)
    return np.minimum(16 * g + g % 16, n_total - 1)


# ----------------------------------------------------------------------------- rules
def _ratio_max(num, den, mask=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0.0, num / den, np.where(num == 0.0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    if mask is not None:
        r = np.where(mask, r, 0.0)
    return float(r.max()) if r.size else 0.0


def split(f, n_factor):
    """(L, W, S) views of a factored buffer [n_total, n_total]."""
    return f[:n_factor, :n_factor], f[n_factor:, :n_factor], f[n_factor:, n_factor:]


def _rows(a, rows):
    return sample_rows(a.shape[0]) if rows is None else np.asarray(rows)


def rho_factor(a, lhat, diag_allow=0.0, rows=None):
    """a: the matrix as uploaded (its lower triangle is read; it may be the whole [n_total, n_total] matrix, whose size decides
    the sampling), lhat [n_factor, n_factor] (lower triangle read).  diag_allow is subtracted from the diagonal ratios (case E:
    one more rounding of a_ii).  rows: evaluate these rows (of the whole matrix) instead of the sample."""
    n = lhat.shape[0]
    u = unit(lhat)
    l = np.tril(lhat).astype(np.float64)
    rows = _rows(a, rows)
    rows = rows[rows < n]
    lr = l[rows]
    num = np.abs(a[rows, :n].astype(np.float64) - lr @ l.T)
    den = u * (np.abs(lr) @ np.abs(l).T)
    cols = np.arange(n)[None, :]
    if diag_allow:
        k = np.arange(rows.size)
        num[k, rows] = np.maximum(num[k, rows] - diag_allow * den[k, rows], 0.0)
    return _ratio_max(num, den, cols <= rows[:, None])


def rho_rows(a, lhat, what, rows=None):
    n = lhat.shape[0]
    u = unit(what)
    l = np.tril(lhat).astype(np.float64)
    rows = _rows(a, rows)
    rows = rows[rows >= n] - n
    w = what[rows].astype(np.float64)
    num = np.abs(a[n + rows, :n].astype(np.float64) - w @ l.T)
    den = u * (np.abs(w) @ np.abs(l).T)
    return _ratio_max(num, den)


# The Schur rule measures ONE product W W^T against the value a factorisation formed from the same W.  Evaluated in fp64 on
# fp64 data it repeats the very arithmetic under test (LAPACK's reference then measures exactly 0, whatever its error), so
# for fp64 data the product is evaluated in the 64-bit-mantissa long double where the platform has one.  (The factor and rows
# rules stay in fp64 as everywhere: potrf and trsm do not sum in the order of the evaluating matrix product, so there the
# evaluation's own rounding is independent noise of a few units on both sides of the comparison.)
WIDE = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64


def rho_schur(a, what, shat, rows=None):
    m, n = what.shape
    u = unit(shat)
    ev = WIDE if shat.dtype == np.float64 else np.float64
    rows = _rows(a, rows)
    rows = rows[rows >= n] - n
    w = what.astype(ev)
    c = a[n + rows, n:].astype(ev)
    num = np.abs(shat[rows].astype(ev) - (c - w[rows] @ w.T)).astype(np.float64)
    den = u * (np.abs(c) + np.abs(w[rows]) @ np.abs(w).T).astype(np.float64)
    return _ratio_max(num, den, np.arange(m)[None, :] <= rows[:, None])


def rho_trsm(l, b, xhat, trans):
    u = unit(xhat)
    op = np.tril(l).astype(np.float64)
    if trans:
        op = op.T
    x = xhat.astype(np.float64)
    return _ratio_max(np.abs(b.astype(np.float64) - op @ x), u * (np.abs(op) @ np.abs(x)))


def residuals(a, f, n_factor, diag_allow=0.0, rows=None):
    """{'factor', 'rows', 'schur'} of a factored buffer f against the uploaded matrix a (rows, schur only with appended rows)."""
    lh, wh, sh = split(f, n_factor)
    out = {"factor": rho_factor(a, lh, diag_allow, rows)}
    if f.shape[0] > n_factor:
        out["rows"] = rho_rows(a, lh, wh, rows)
        out["schur"] = rho_schur(a, wh, sh, rows)
    return out


def logdet_self(lhat):
    """(2 sum log L_ii, sum |2 log L_ii|) in fp64 from the stored diagonal."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 2.0 * np.log(np.diagonal(lhat).astype(np.float64))
    return math.fsum(t), math.fsum(np.abs(t))


def logdet_bound(lhat):
    """fp64 logs of the stored diagonal, each within a few ulp, and n fp64 additions in any order."""
    return (lhat.shape[0] + 8) * 2.0 ** -53 * logdet_self(lhat)[1]


def logdet_ok(logdet, lhat):
    return bool(abs(logdet - logdet_self(lhat)[0]) <= logdet_bound(lhat))


def info_ok(info, logdet, p):
    """A failing pivot p (1-based): exactly p, and no log-determinant."""
    return info == p and math.isnan(logdet)


def within(got, n_factor, ref=None):
    """The bounds of one case: every rho at most n_factor + 1 (derived) and, given the reference's, at most REF_FACTOR times it."""
    for k, v in got.items():
        if not v <= n_factor + 1:
            return False
        if ref is not None and not v <= REF_FACTOR * ref[k]:
            return False
    return True


# ----------------------------------------------------------------------------- LAPACK in the matrix's own precision
def lapack_factor(a, n_factor):
    """(buffer laid out as smn_cholesky leaves it, info): potrf of the leading block, trsm for the appended rows, the Schur block
    by the dtype product -- all in a's dtype.  The strict upper triangle is a's."""
    potrf = sla.lapack.spotrf if a.dtype == np.float32 else sla.lapack.dpotrf
    n = n_factor
    f = np.array(a)
    c, info = potrf(a[:n, :n], lower=1, clean=1)
    il = np.tril_indices(n)
    f[:n, :n][il] = c[il]
    if info == 0 and a.shape[0] > n:
        w = np.ascontiguousarray(sla.solve_triangular(c, a[n:, :n].T, lower=True, check_finite=False).T)
        s = a[n:, n:] - w @ w.T
        assert w.dtype == a.dtype and s.dtype == a.dtype
        f[n:, :n] = w
        im = np.tril_indices(a.shape[0] - n)
        f[n:, n:][im] = s[im]
    return f, int(info)


def lapack_first_bad_pivot(a, n_factor):
    """1-based index of the first pivot LAPACK could not take, 0 if none: potrf's info where it gives one, else the first
    diagonal entry of its factor that is not finite.  (Reference LAPACK's potrf2 tests the pivot with `ajj <= 0 or isnan(ajj)`;
    an optimised potrf may test `ajj <= 0` alone, carry a NaN pivot through and return info = 0 -- the NaN pivot is then in
    the factor it returns, at the same place.)"""
    f, info = lapack_factor(a, n_factor)
    if info:
        return info
    bad = ~np.isfinite(np.diagonal(f)[:n_factor])
    return int(np.argmax(bad)) + 1 if bad.any() else 0


def lapack_trsm(l, b, trans):
    x = sla.solve_triangular(l, b, lower=True, trans=1 if trans else 0, check_finite=False)
    assert x.dtype == b.dtype
    return x


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(n_factor, m, dtype):
    """(a, LAPACK's buffer, the reference residuals) of shape case (n_factor, m): once per process, read-only.  The reference
    residuals are LAPACK's, or the chain emulation's for the shapes of CHAIN_SHAPES."""
    a = matrix(n_factor, m, dtype)
    f, info = lapack_factor(a, n_factor)
    assert info == 0
    _frozen(a, f)
    if (n_factor, m, dtype) in CHAIN_SHAPES:
        return a, f, chain_residuals(a, f, n_factor)
    return a, f, residuals(a, f, n_factor)


@functools.lru_cache(maxsize=None)
def shift_reference(n_factor, m, n_shift, kind, dtype):
    """(a as uploaded, a shifted on the host, LAPACK's buffer of the shifted matrix, the reference residuals: the chain
    emulation's on the shifted matrix)."""
    jitter, ridge = SHIFT_KINDS[kind]
    a = shift_matrix(n_factor, m, n_shift, dtype)
    a_sh = shifted(a, n_shift, jitter, ridge)
    f, info = lapack_factor(a_sh, n_factor)
    assert info == 0
    _frozen(a, a_sh, f)
    return a, a_sh, f, chain_residuals(a_sh, f, n_factor)


@functools.lru_cache(maxsize=None)
def trsm_reference(n, nrhs, trans, dtype):
    l, b = trsm_case(n, nrhs, dtype)
    x = lapack_trsm(l, b, trans)
    _frozen(l, b, x)
    return l, b, x, rho_trsm(l, b, x, trans)


# ----------------------------------------------------------------------------- the library's summation order
# update_kernel (cholesky.hip) starts its accumulator at -C and runs the K loop on top of it ("acc starts at -C so the C read is
# in flight together with the first operand loads"), and C goes back to memory in the same precision between launches.  Whatever
# the blocking, entry (i, j) is therefore formed as ONE chain in the order of k,
#       c_0 = a_ij,   c_k = fl(c_{k-1} - l_ik l_jk),   l_ij = fl(c_j / l_jj)    (sqrt on the diagonal; no division in the Schur block)
# so every step rounds at the size of the running c -- of a_ij itself while the subtracted part is small -- where LAPACK's
# kernels sum the products by themselves, in several short chains, and subtract once.  Both are within the derived bound; the
# chain's error grows like sqrt(k) u |c|, and on a matrix whose diagonal dwarfs its off-diagonal part (case E) or from a few
# thousand columns on it is more than 8 times LAPACK's.  For the cases listed in CHAIN_SHAPES and for every case E the
# reference is therefore this emulation of the chain, not LAPACK: measured on the GPU, LAPACK's rho | the library's were
# 3.9 | 37.4 (4480,0) fp64, 3.6 | 45.8 (5120,0) fp64, 3.0 | 27.3 (2432,128) fp64, 4.9 | 58.8 (5888,0) fp32, and 4.2 | 57.8 on
# (640,128) fp32 with the diagonal 100 times larger and no shift at all (profiles/r14_factor_residuals.txt).
#
# The emulation is independent of the library: plain NumPy in the matrix's own dtype, row by row of a subsample of CHAIN_ROWS
# of the rule's rows, every other row of the factor taken from LAPACK.  The residual of entry (i, j) is the rounding committed
# while forming l_ij from the l_jk used, so a row's residuals do not depend on how the other rows were obtained.  Two
# simplifications, both short of what is modelled: NumPy rounds the product before it subtracts where the MFMA fuses (at most
# u |l_ik l_jk| more per step, beside the u |c| the order costs), and the sums inside a 128-column sub-panel (the 16-column
# leaves) and trail_kernel's K <= 512 (which starts from zero) are taken as part of the same chain.
CHAIN_ROWS = 64
# (129,1) fp32 is here for another reason: its Schur block is ONE entry, and LAPACK's single dot product happens to land 0.078 u
# from the exact value (the library 0.82 u, the chain 0.61 u): eight times a lucky rounding is no bound.
CHAIN_SHAPES = {(4480, 0, F64), (5120, 0, F64), (2432, 128, F64), (5888, 0, F32), (129, 1, F32)}


def chain_rows(n_total):
    rows = sample_rows(n_total)
    return rows[::-1][::max(1, rows.size // CHAIN_ROWS)][::-1]           # (counted from the last row: the longest chains)


def emulate_chain(a, f_base, n_factor, rows):
    """f_base (LAPACK's buffer of a) with the given rows recomputed by the chain above, in a's dtype."""
    rows = np.asarray(rows)                                              # ascending
    g = np.array(f_base)
    c = np.array(a[rows])                                                # working rows; columns above the diagonal are carried along, unused
    where = {int(r): k for k, r in enumerate(rows)}
    with np.errstate(all="ignore"):
        for k in range(n_factor):
            if k in where:
                c[where[k], k] = np.sqrt(c[where[k], k])
                g[k, k] = c[where[k], k]
            i0 = int(np.searchsorted(rows, k, side="right"))             # the working rows below row k
            if i0 == rows.size:
                break
            c[i0:, k] /= g[k, k]
            g[rows[i0:], k] = c[i0:, k]
            c[i0:, k + 1:] -= np.outer(c[i0:, k], g[k + 1:, k])          # dtype arithmetic throughout
    for k, r in enumerate(rows):
        if r >= n_factor:
            g[r, n_factor:r + 1] = c[k, n_factor:r + 1]
    return g


def chain_residuals(a, f_base, n_factor):
    rows = chain_rows(a.shape[0])
    return residuals(a, emulate_chain(a, f_base, n_factor, rows), n_factor, rows=rows)


# ----------------------------------------------------------------------------- damage (host tests)
def drop_product(f, i, j, k):
    """Entry (i, j), i > j > k, of the factor as a K loop that stopped before step k leaves it: the product l_ik l_jk is never
    subtracted."""
    g = np.array(f)
    g[i, j] = g[i, j] + g[i, k] * g[j, k] / g[j, j]
    return g


def drop_last_kstep(f, r0, c0):
    """Rows [r0, r0 + 16) of tile columns [c0, c0 + 128), c0 + 128 <= r0: the last MFMA K step (columns c0 - 4 .. c0 - 1) of
    their update never ran."""
    g = np.array(f)
    rows, cols, ks = slice(r0, r0 + 16), slice(c0, c0 + TILE), slice(c0 - 4, c0)
    g[rows, cols] = g[rows, cols] + (g[rows, ks] @ g[cols, ks].T) / np.diagonal(g)[cols][None, :]
    return g


def logdet_without_subpanel(lhat, p):
    """logdet with the atomicAdd of sub-panel p (columns [128 p, 128 p + 128)) lost."""
    with np.errstate(divide="ignore"):
        t = 2.0 * np.log(np.diagonal(lhat).astype(np.float64))
    return math.fsum(t) - math.fsum(t[TILE * p:TILE * (p + 1)])
