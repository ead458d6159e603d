"""Greedy pivoted Cholesky of a kernel matrix that is never formed: K(X, X) ~ L L^T with L [N, M], from the kernel's diagonal
and M of its rows (csrc/pchol.hip).  The pivots are the conditional-variance choice of M inducing points, L is the Nystroem
factor of those points, and the trace of what is left out is known after every step, so a rank can be chosen by tolerance.

    res = pivoted_cholesky(kernel_fn, x, max_rank, tol=0.0, route="auto", pivots=None)
    res.pivots, res.factor, res.resid, res.trace, res.rank, res.approx(rows, cols)
    greedy_variance_points(kernel_fn, x, m)  ->  pivots
    fit = woodbury_fit(res, y, lam, fitc)        regression on the factor (csrc/lowrank.hip): fit.quad, fit.logdet, fit.info,
    fit.readout(kzt, ktt) -> mean, var           K^ = L L^T + diag(fitc max(resid, 0) + lam) by the Woodbury identity
    terms = woodbury_grad(fit, kernel_fn, x, coef)   sum G dK^/d(w_std, b_std, last_w_std, lam) at FIXED pivots (csrc/lowrank_grad.hip)
    out = kernel_matmul(kernel_fn, x1, x2, v, shift=0.0)     K(x1, x2) V (+ shift V) without K (csrc/kernel_matmul.hip)
    sol = pcg_solve(kernel_fn, x, b, lam, precond=res)       (K + lam I) X = B by preconditioned CG (csrc/pcg.hip): a PcgResult

pivots=<distinct indices>: step j is taken at pivots[j] instead of the arg-max (both routes).  The loop still stops before step j
when resid[pivots[j]] is not above the floor below, so a later pivot that duplicates an earlier pivot's row ends the factor there.
A factor built at the pivots a greedy call returned, at the same hyper-parameters, carries that call's bits.

Routes
  "fused"   MLP / dense-ResNet kernel functions with NNGP covariance: one call (smn_pchol_mlp) queues every step; the kernel
            rows are made inside the step kernel from x, which is streamed once per step.
  "matrix"  the host loop over smn_pchol_begin / smn_pchol_step: the diagonal from the kernel function, one row
            kernel_fn(x[p:p+1], x) per step.  The conv kernel functions (all three), MLP-family functions under
            with_cov("ntk"), and any other callable kernel_fn(x1, x2) that also has diag(x).
  "auto"    the fused route where it exists.

Both stop before step j when trace_j <= tol * trace_0, or when the largest residual is not above 4 (j + 1) eps max_i K_ii (eps: the
unit roundoff of the storage dtype): the rounding noise of a residual computed from j stored columns -- the matrix has run out
of numerical rank.  The floor grows with the columns made, not with N.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeviceArray, as_device, default_context
from .nt_kernels import CnnKernelFn, KernelFn

__all__ = ["pivoted_cholesky", "greedy_variance_points", "PivotedCholesky", "woodbury_fit", "WoodburyFit", "woodbury_grad",
           "kernel_diag", "kernel_cross", "kernel_matmul", "pcg_solve", "PcgResult"]

_DIAG_BLOCK = 256   # rows per symmetric build when an MLP-family diagonal is taken from diagonal blocks (matrix route)


class PivotedCholesky:
    """pivots: np.int64 [rank]; factor: device array [N, rank] in the dtype of x; resid: np.float64 [N], K_ii - sum_t L_it^2;
    trace: np.float64 [rank + 1], the trace of the residual before each step and after the last; rank: columns made."""

    def __init__(self, pivots, factor, resid, trace, rank):
        self.pivots, self.factor, self.resid, self.trace, self.rank = pivots, factor, resid, trace, int(rank)
        self._host = None

    def approx(self, rows=None, cols=None):
        """(L L^T)[rows][:, cols] on the host in fp64 (None: every row / column); for tests and figures."""
        if self._host is None:
            self._host = np.asarray(self.factor.raw_numpy(), dtype=np.float64).reshape(self.factor.shape)
        a = self._host if rows is None else self._host[np.asarray(rows, dtype=np.int64)]
        b = self._host if cols is None else self._host[np.asarray(cols, dtype=np.int64)]
        return a @ b.T


def _num_rows(x):
    shape = tuple(x.shape) if isinstance(x, DeviceArray) else np.shape(x)
    if len(shape) < 2 or shape[0] < 1:
        raise ValueError("x must be [N, ...] with N >= 1, got shape %s" % (shape,))
    return int(shape[0])


def _pick_route(kernel_fn, route):
    if route not in ("auto", "fused", "matrix"):
        raise ValueError("route must be 'auto', 'fused' or 'matrix', got %r" % (route,))
    fusable = isinstance(kernel_fn, KernelFn) and kernel_fn.cov == "nngp"
    if route == "fused" and not fusable:
        raise NotImplementedError("route='fused' exists for get_mlp_kernel / get_dense_resnet_kernel with NNGP covariance; %s%s goes "
                                  "through route='matrix'" % (type(kernel_fn).__name__,
                                                              " under with_cov('ntk')" if isinstance(kernel_fn, KernelFn) else ""))
    if route == "auto":
        route = "fused" if fusable else "matrix"
    if route == "matrix" and not isinstance(kernel_fn, (KernelFn, CnnKernelFn)):
        if not callable(kernel_fn) or not callable(getattr(kernel_fn, "diag", None)):
            raise TypeError("route='matrix' needs a callable kernel_fn(x1, x2) that also has diag(x)")
    return route


def _check_pivots(pivots, n):
    """pivots as np.int64 [m]: distinct indices in [0, n)."""
    p = np.asarray(pivots)
    if p.ndim != 1 or p.shape[0] < 1 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError("pivots must be a non-empty 1-D integer array, got shape %s dtype %s" % (p.shape, p.dtype))
    p = np.ascontiguousarray(p, dtype=np.int64)
    if p.min() < 0 or p.max() >= n:
        raise ValueError("pivots must lie in [0, N = %d)" % n)
    if np.unique(p).shape[0] != p.shape[0]:
        raise ValueError("pivots must be distinct")
    return p


def _check(kernel_fn, x, max_rank, tol, route, pivots=None):
    """Everything that can be refused without a device: returns (N, max_rank, tol, route[, pivots])."""
    n = _num_rows(x)
    if pivots is not None:
        pivots = _check_pivots(pivots, n)
        if max_rank is not None and int(max_rank) != pivots.shape[0]:
            raise ValueError("max_rank = %d does not equal len(pivots) = %d" % (int(max_rank), pivots.shape[0]))
        max_rank = pivots.shape[0]
    elif max_rank is None:
        raise ValueError("max_rank is needed when no pivots are given")
    max_rank = int(max_rank)
    if max_rank < 1 or max_rank > n:
        raise ValueError("max_rank must lie in [1, N = %d], got %d" % (n, max_rank))
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError("tol must be >= 0, got %r" % (tol,))
    route = _pick_route(kernel_fn, route)
    return (n, max_rank, tol, route) if pivots is None else (n, max_rank, tol, route, pivots)


def _compact(ctx, factor, rank):
    """factor [N, max_rank] -> [N, rank] (two device transposes: the library has no strided device copy)."""
    n, m = factor.shape
    if rank == m:
        return factor
    out = ctx.empty((n, rank), factor.dtype)
    if rank > 0:
        t = ctx.empty((rank, n), factor.dtype)
        ctx.call("smn_transpose", factor.dcode, t.ptr, n, factor.ptr, m, n, rank)
        ctx.call("smn_transpose", factor.dcode, out.ptr, rank, t.ptr, n, rank, n)
    return out


def _fused(kernel_fn, x, n, max_rank, tol, given=None):
    xs = kernel_fn.scaled(x)
    ctx = xs.ctx
    d = xs.shape[1]
    factor = ctx.empty((n, max_rank), xs.dtype)
    resid = ctx.empty((n,), np.float64)
    pivots = np.zeros(max_rank, dtype=np.int64)
    trace = np.zeros(max_rank + 1, dtype=np.float64)
    rank = C.c_int64(0)
    if given is None:
        ctx.call("smn_pchol_mlp", xs.dcode, kernel_fn.net, kernel_fn.act, kernel_fn.num_hiddens, kernel_fn.w_std, kernel_fn.b_std,
                 kernel_fn.last_w_std, xs.ptr, n, d, d, max_rank, tol, factor.ptr, max_rank, resid.ptr,
                 pivots.ctypes.data_as(C.POINTER(C.c_int64)), trace.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rank))
    else:
        pivots = given
        ctx.call("smn_pchol_mlp_at", xs.dcode, kernel_fn.net, kernel_fn.act, kernel_fn.num_hiddens, kernel_fn.w_std, kernel_fn.b_std,
                 kernel_fn.last_w_std, xs.ptr, n, d, d, pivots.ctypes.data_as(C.POINTER(C.c_int64)), max_rank, tol, factor.ptr,
                 max_rank, resid.ptr, trace.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rank))
    r = int(rank.value)
    return PivotedCholesky(pivots[:r].copy(), _compact(ctx, factor, r), resid.raw_numpy(), trace[:r + 1].copy(), r)


def _row_view(xd, p):
    """x[p:p+1] of a device array as a view (no copy); keeps the buffer alive."""
    row_elems = int(np.prod(xd.shape[1:]))
    v = DeviceArray(xd.ctx, (1,) + tuple(xd.shape[1:]), xd.dtype,
                    ptr=C.c_void_p(xd.ptr.value + int(p) * row_elems * xd.dtype.itemsize), owner=False)
    v._base = xd
    return v


def _rows_view(xd, a, b):
    row_elems = int(np.prod(xd.shape[1:]))
    v = DeviceArray(xd.ctx, (b - a,) + tuple(xd.shape[1:]), xd.dtype,
                    ptr=C.c_void_p(xd.ptr.value + int(a) * row_elems * xd.dtype.itemsize), owner=False)
    v._base = xd
    return v


def kernel_diag(kernel_fn, xd, x=None):
    """K(x_i, x_i) [N] as a device array in the dtype of xd, without the other pairs.  The conv kernel functions have their own
    diag; an MLP-family diagonal is read off the symmetric builds of diagonal blocks, O(N B d) with B = _DIAG_BLOCK; any other
    callable is asked for diag(x) (x: the array as the caller handed it in, xd by default)."""
    ctx, n, dt = xd.ctx, xd.shape[0], xd.dtype
    if isinstance(kernel_fn, CnnKernelFn):
        return kernel_fn.diag(xd)
    if isinstance(kernel_fn, KernelFn):
        dh = np.empty(n, dtype=dt)
        for a in range(0, n, _DIAG_BLOCK):
            b = min(n, a + _DIAG_BLOCK)
            dh[a:b] = kernel_fn(_rows_view(xd, a, b), None, get=kernel_fn.cov).diagonal()
        return ctx.to_device(dh)
    return as_device(np.asarray(kernel_fn.diag(xd if x is None else x)).reshape(-1), ctx, dtype=dt)


def kernel_cross(kernel_fn, a, b):
    """K(a, b) [na, nb] as a plain device array in the dtype of a: the covariance mode of an MLP-family kernel function, the
    NNGP kernel of a conv one, whatever any other callable returns."""
    if isinstance(kernel_fn, KernelFn):
        return kernel_fn(a, b, get=kernel_fn.cov)
    if isinstance(kernel_fn, CnnKernelFn):
        return kernel_fn(a, b)
    return as_device(kernel_fn(a, b), a.ctx, dtype=a.dtype)


def _matrix(kernel_fn, x, n, max_rank, tol, given=None):
    native = isinstance(kernel_fn, (KernelFn, CnnKernelFn))
    ctx = getattr(kernel_fn, "ctx", None) or (x.ctx if isinstance(x, DeviceArray) else default_context())
    xd = as_device(x, ctx)
    if isinstance(kernel_fn, KernelFn) and len(xd.shape) != 2:
        xd = ctx.to_device(xd.numpy().reshape(n, -1))
    dt = xd.dtype
    diag = kernel_diag(kernel_fn, xd, x)
    if isinstance(kernel_fn, CnnKernelFn):
        row = lambda p: kernel_fn(_row_view(xd, p), xd)
    elif isinstance(kernel_fn, KernelFn):
        row = lambda p: kernel_fn(_row_view(xd, p), xd, get=kernel_fn.cov)
    else:
        row = lambda p: as_device(kernel_fn(_row_view(xd, p), xd), ctx, dtype=dt)
    if tuple(diag.shape) != (n,) or diag.dtype != dt:
        raise ValueError("diag(x) must be [N] in the dtype of x, got %s %s" % (diag.shape, diag.dtype))
    factor = ctx.empty((n, max_rank), dt)
    ctx.call("smn_memset", factor.ptr, 0, factor.nbytes)
    resid = ctx.empty((n,), np.float64)
    piv, rmax, tr = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    ctx.call("smn_pchol_begin", xd.dcode, n, diag.ptr, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
    floor1 = 4.0 * float(np.finfo(dt).eps) * max(rmax.value, 0.0)      # the floor of step j is (j + 1) times this
    pivots, trace = [], [tr.value]
    rp = C.c_double(0.0)
    for j in range(max_rank):
        if given is not None:                        # the prescribed pivot and its residual stand in for the arg-max
            piv.value = int(given[j])
            ctx.call("smn_memcpy_d2h", C.byref(rp), C.c_void_p(resid.ptr.value + 8 * piv.value), 8)
            rmax.value = rp.value
        if not rmax.value > (j + 1) * floor1 or trace[-1] <= tol * trace[0]:
            break
        k = row(piv.value)
        if not native and (k.size != n):
            raise ValueError("kernel_fn(x[p:p+1], x) must have N entries, got shape %s" % (k.shape,))
        p = piv.value
        ctx.call("smn_pchol_step", xd.dcode, n, j, p, k.ptr, factor.ptr, max_rank, resid.ptr, C.byref(piv), C.byref(rmax),
                 C.byref(tr))
        pivots.append(p)
        trace.append(tr.value)
    r = len(pivots)
    return PivotedCholesky(np.asarray(pivots, dtype=np.int64), _compact(ctx, factor, r), resid.raw_numpy(),
                           np.asarray(trace, dtype=np.float64), r)


def pivoted_cholesky(kernel_fn, x, max_rank=None, tol=0.0, route="auto", pivots=None):
    """The partial Cholesky factorisation of K(x, x) with greedy pivoting (largest residual variance, ties to the lowest
    index), up to max_rank <= N columns; x a host or a device array.  Input scales of an MLP-family kernel function are
    applied first.  pivots: an integer array of distinct indices in [0, N) to take, in order, instead of the greedy choice
    (max_rank may then be omitted, or must equal len(pivots)).  See the module docstring for the routes and the stopping rule."""
    if pivots is None:
        n, max_rank, tol, route = _check(kernel_fn, x, max_rank, tol, route)
        return (_fused if route == "fused" else _matrix)(kernel_fn, x, n, max_rank, tol)
    n, max_rank, tol, route, pivots = _check(kernel_fn, x, max_rank, tol, route, pivots)
    return (_fused if route == "fused" else _matrix)(kernel_fn, x, n, max_rank, tol, pivots)


def greedy_variance_points(kernel_fn, x, m):
    """Indices of (up to) m rows of x chosen greedily by largest conditional variance: the pivots of pivoted_cholesky."""
    return pivoted_cholesky(kernel_fn, x, m).pivots


class WoodburyFit:
    """What smn_lowrank_fit leaves: quad [c] = y_k^T K^^-1 y_k, logdet = log|K^|, info (0, or the failing pivot of I + G; quad
    and logdet are then NaN), and on the device the fp64 factor C of I + L^T W L, beta = (I + G)^-1 L^T W Y and R = L[pivots, :]."""

    def __init__(self, res, lam, fitc, quad, logdet, info, c_fac, beta, r_fac, y_dev=None):
        self.res, self.lam, self.fitc, self.y_dev = res, float(lam), bool(fitc), y_dev   # y_dev: the targets as the fit read them
        self.quad, self.logdet, self.info = quad, float(logdet), int(info)
        self.c_fac, self.beta, self.r_fac = c_fac, beta, r_fac

    def readout(self, kzt, ktt):
        """(mean [t, c], var [t]) device arrays in the factor's dtype from kzt [rank, t] = K(Z, x*), Z = x[res.pivots], and
        ktt [t] = K(x*, x*): smn_lowrank_readout.  A point carries the same bits alone or inside a larger chunk."""
        f = self.res.factor
        ctx, m = f.ctx, self.res.rank
        kzt, ktt = as_device(kzt, ctx, dtype=f.dtype), as_device(ktt, ctx, dtype=f.dtype)
        if len(kzt.shape) != 2 or kzt.shape[0] != m or tuple(ktt.shape) != (kzt.shape[1],):
            raise ValueError("kzt must be [rank = %d, t] and ktt [t], got %s and %s" % (m, kzt.shape, ktt.shape))
        t, c = kzt.shape[1], self.beta.shape[1]
        mean, var = ctx.empty((t, c), f.dtype), ctx.empty((t,), f.dtype)
        ctx.call("smn_lowrank_readout", f.dcode, kzt.ptr, t, ktt.ptr, t, m, self.r_fac.ptr, m, self.c_fac.ptr, self.beta.ptr, c,
                 mean.ptr, var.ptr)
        return mean, var


def _check_fit(res, y, lam, fitc):
    """Everything woodbury_fit can refuse without a device: returns (y [n, c] float64, lam)."""
    if not isinstance(res, PivotedCholesky):
        raise TypeError("res must be a PivotedCholesky (pivoted_cholesky's result), got %s" % type(res).__name__)
    if res.rank < 1:
        raise ValueError("the factor has rank 0: nothing to regress on")
    if res.rank > _lib.LOWRANK_MAX_RANK:
        raise NotImplementedError("rank %d is above the limit of %d columns (SMN_LOWRANK_MAX_RANK)" % (res.rank, _lib.LOWRANK_MAX_RANK))
    n = int(res.factor.shape[0])
    y = np.asarray(y, dtype=np.float64)
    y = y.reshape(n, 1) if y.ndim == 1 and y.shape[0] == n else y
    if y.ndim != 2 or y.shape[0] != n or not 1 <= y.shape[1] <= 48:
        raise ValueError("y must be [N = %d] or [N, C] with 1 <= C <= 48, got shape %s" % (n, np.shape(y)))
    lam = float(lam)
    if not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError("lam must be a positive finite number, got %r" % (lam,))
    if fitc not in (0, 1, False, True):
        raise ValueError("fitc must be a bool, got %r" % (fitc,))
    return y, lam


def woodbury_fit(res, y, lam, fitc=True):
    """The regression quantities of K^ = L L^T + diag(d), d_i = fitc max(resid_i, 0) + lam, for a PivotedCholesky `res` and
    targets y [N] or [N, C <= 48]: a WoodburyFit.  fitc=True is the FITC approximation on the greedy inducing points, False is
    SoR / DTC.  O(N rank^2) work and O(N rank) memory; the rank x rank side runs in fp64 for both dtypes.  An fp32 factor
    under fitc with a small lam loses digits in quad: the pivot rows have resid = 0, hence weight 1 / lam, and
    s - |C^-1 B|^2 cancels (2.8e-2 relative at lam = 1e-6; README, "Low-rank regression")."""
    y, lam = _check_fit(res, y, lam, fitc)
    f = res.factor
    ctx, (n, m), c = f.ctx, f.shape, y.shape[1]
    yd = ctx.to_device(np.ascontiguousarray(y, dtype=f.dtype))
    resid = ctx.to_device(np.ascontiguousarray(res.resid, dtype=np.float64)) if fitc else None
    c_fac, beta = ctx.empty((m, m), np.float64), ctx.empty((m, c), np.float64)
    quad = np.zeros(c, dtype=np.float64)
    logdet, info = C.c_double(0.0), C.c_int(0)
    ctx.call("smn_lowrank_fit", f.dcode, f.ptr, n, m, m, None if resid is None else resid.ptr, lam, 1 if fitc else 0, yd.ptr, c, c,
             c_fac.ptr, beta.ptr, quad.ctypes.data_as(C.POINTER(C.c_double)), C.byref(logdet), C.byref(info))
    if getattr(res, "_r_fac", None) is None:     # R = L[pivots, :] in fp64: rank row copies, once per factor
        r = np.empty((m, m), dtype=f.dtype)
        isz = f.dtype.itemsize
        for j, p in enumerate(res.pivots):
            ctx.call("smn_memcpy_d2h", r[j].ctypes.data_as(C.c_void_p), C.c_void_p(f.ptr.value + int(p) * m * isz), m * isz)
        res._r_fac = ctx.to_device(np.tril(r).astype(np.float64))
    return WoodburyFit(res, lam, fitc, quad, logdet.value, info.value, c_fac, beta, res._r_fac, yd)


def _check_grad(fit, kernel_fn, x, coef):
    """Everything woodbury_grad can refuse without a device: returns coef."""
    if not isinstance(fit, WoodburyFit):
        raise TypeError("fit must be a WoodburyFit (woodbury_fit's result), got %s" % type(fit).__name__)
    if isinstance(kernel_fn, KernelFn) and kernel_fn.cov != "nngp":
        raise NotImplementedError("woodbury_grad has no form for with_cov(%r): SMN_NET_NTK is not supported" % (kernel_fn.cov,))
    if not isinstance(kernel_fn, KernelFn):
        raise NotImplementedError("woodbury_grad exists for get_mlp_kernel / get_dense_resnet_kernel with NNGP covariance, not for %s"
                                  % type(kernel_fn).__name__)
    if getattr(kernel_fn, "input_scales", None) is not None:
        raise NotImplementedError("woodbury_grad does not support input scales")
    n = int(fit.res.factor.shape[0])
    shape = tuple(x.shape) if isinstance(x, DeviceArray) else np.shape(x)
    if len(shape) != 2 or shape[0] != n:
        raise ValueError("x must be [N = %d, d], got shape %s" % (n, shape))
    coef = float(coef)
    if not np.isfinite(coef):
        raise ValueError("coef must be finite, got %r" % (coef,))
    return coef


def woodbury_grad(fit, kernel_fn, x, coef):
    """terms [4] = sum_ij G_ij dK^_ij / d(w_std, b_std, last_w_std, lam) with G = coef alpha alpha^T - C K^^-1 (the convention of
    smn_lml_grad_terms: d logpdf / d theta = terms / 2), for a WoodburyFit whose factor was built on x by kernel_fn at the pivots
    fit.res.pivots.  The pivots are held FIXED: the derivative of the selection is not part of it.  One smn_lowrank_grad call,
    O(N rank^2 + N rank d) work and O(N rank) memory.  MLP / dense-ResNet kernel functions with NNGP covariance; NaN when the fit
    failed (fit.info != 0)."""
    coef = _check_grad(fit, kernel_fn, x, coef)
    if fit.info != 0:
        return np.full(4, np.nan)
    res = fit.res
    f = res.factor
    ctx, (n, m) = f.ctx, f.shape
    xd = as_device(x, ctx, dtype=f.dtype)
    d, c = xd.shape[1], fit.beta.shape[1]
    resid = ctx.to_device(np.ascontiguousarray(res.resid, dtype=np.float64)) if fit.fitc else None
    piv = np.ascontiguousarray(res.pivots, dtype=np.int64)
    terms = np.zeros(4, dtype=np.float64)
    ctx.call("smn_lowrank_grad", f.dcode, kernel_fn.net, kernel_fn.act, kernel_fn.num_hiddens, kernel_fn.w_std, kernel_fn.b_std,
             kernel_fn.last_w_std, xd.ptr, n, d, d, piv.ctypes.data_as(C.POINTER(C.c_int64)), f.ptr, m, m,
             None if resid is None else resid.ptr, fit.lam, 1 if fit.fitc else 0, fit.y_dev.ptr, c, c, fit.c_fac.ptr, fit.beta.ptr,
             fit.r_fac.ptr, m, coef, terms.ctypes.data_as(C.POINTER(C.c_double)))
    return terms


def _check_matrix_free(kernel_fn):
    """kernel_matmul / pcg_solve exist for the MLP family alone; refused before any device call."""
    if not isinstance(kernel_fn, KernelFn):
        raise NotImplementedError("the matrix-free product exists for get_mlp_kernel / get_dense_resnet_kernel (NNGP or with_cov('ntk')), "
                                  "not for %s: a matrix-free conv kernel costs P times more per pair" % type(kernel_fn).__name__)


def _shape2(a, what):
    shape = tuple(a.shape) if isinstance(a, DeviceArray) else np.shape(a)
    if len(shape) < 2 or shape[0] < 1 or int(np.prod(shape[1:])) < 1:
        raise ValueError("%s must be [N, d] with N, d >= 1, got shape %s" % (what, shape))
    return int(shape[0]), int(np.prod(shape[1:]))


def _check_matmul(kernel_fn, x1, x2, v, shift):
    """Everything kernel_matmul can refuse without a device: returns (n1, n2, t, shift)."""
    _check_matrix_free(kernel_fn)
    n1, d = _shape2(x1, "x1")
    n2 = n1
    if x2 is not None:
        n2, d2 = _shape2(x2, "x2")
        if d2 != d:
            raise ValueError("x1 and x2 feature dimensions differ: %d vs %d" % (d, d2))
    vs = tuple(v.shape) if isinstance(v, DeviceArray) else np.shape(v)
    if len(vs) == 1:
        vs = (vs[0], 1)
    if len(vs) != 2 or vs[0] != n2 or vs[1] < 1:
        raise ValueError("v must be [%d] or [%d, t] with t >= 1, got shape %s" % (n2, n2, vs))
    shift = float(shift)
    if not np.isfinite(shift):
        raise ValueError("shift must be finite, got %r" % (shift,))
    if x2 is not None and shift != 0.0:
        raise ValueError("shift belongs to the symmetric form (x2=None), got shift = %r with x2 given" % (shift,))
    return n1, n2, int(vs[1]), shift


def kernel_matmul(kernel_fn, x1, x2, v, shift=0.0):
    """K(x1, x2) V as a device fp64 array [n1, t], K never stored (smn_kernel_mlp_matmul): the covariance mode of an MLP /
    dense-ResNet kernel function (with_cov("ntk"): Theta), input scales applied first.  x2=None is the symmetric form on the
    exact diagonal, K(x1, x1) V + shift V with the shift added in fp64.  v [n2] or [n2, t] is taken in the dtype of x1.  Cost:
    ceil(t / 16) builds of the n1 x n2 rectangle; memory O((n1 + n2) (d + t))."""
    n1, n2, t, shift = _check_matmul(kernel_fn, x1, x2, v, shift)
    a = kernel_fn.scaled(x1)
    ctx = a.ctx
    b = None if x2 is None or x2 is x1 else kernel_fn.scaled(x2, ctx, dtype=a.dtype)
    if x2 is x1:
        n2 = n1
    vd = as_device(v, ctx, dtype=a.dtype)
    out = ctx.empty((n1, t), np.float64)
    net = kernel_fn.params[0]
    ctx.call("smn_kernel_mlp_matmul", a.dcode, net, kernel_fn.act, kernel_fn.num_hiddens, kernel_fn.w_std, kernel_fn.b_std,
             kernel_fn.last_w_std, a.ptr, n1, a.shape[1], None if b is None else b.ptr, n2, a.shape[1], a.shape[1], shift, vd.ptr, t, t,
             out.ptr, t)
    return out


class PcgResult:
    """x: device fp64 [N, C]; iters: iterations run; col_iters: np.int32 [C], the iteration at which each column stopped; resid:
    np.float64 [C], the TRUE relative residuals |b - (K + lam I) x| / |b| of the returned solution; history: np.float64
    [iters + 1, C], the recurrence's relative residual per iteration; info: 0 converged, 1 max_iter reached, 2 breakdown (x and
    resid are NaN); converged: info == 0."""

    def __init__(self, x, iters, col_iters, resid, history, info):
        self.x, self.iters, self.col_iters, self.resid, self.history, self.info = x, int(iters), col_iters, resid, history, int(info)
        self.converged = self.info == 0


def _check_pcg(kernel_fn, x, b, lam, precond, tol, max_iter, x0):
    """Everything pcg_solve can refuse without a device: returns (n, b [n, c] float64, lam, tol, max_iter, x0 or None)."""
    _check_matrix_free(kernel_fn)
    n, _ = _shape2(x, "x")
    if precond is not None:
        if not isinstance(precond, PivotedCholesky):
            raise TypeError("precond must be a PivotedCholesky (pivoted_cholesky's result) or None, got %s" % type(precond).__name__)
        if precond.rank > _lib.LOWRANK_MAX_RANK:
            raise NotImplementedError("rank %d is above the limit of %d columns (SMN_LOWRANK_MAX_RANK)" % (precond.rank, _lib.LOWRANK_MAX_RANK))
        if precond.rank > 0 and int(precond.factor.shape[0]) != n:
            raise ValueError("the preconditioner's factor has %d rows, x has %d" % (int(precond.factor.shape[0]), n))
    if isinstance(b, DeviceArray):
        b = b.numpy()
    b = np.asarray(b, dtype=np.float64)
    b = b.reshape(n, 1) if b.ndim == 1 and b.shape[0] == n else b
    if b.ndim != 2 or b.shape[0] != n or b.shape[1] < 1:
        raise ValueError("b must be [N = %d] or [N, C] with C >= 1, got shape %s" % (n, np.shape(b)))
    if b.shape[1] > _lib.PCG_MAX_COLS:
        raise NotImplementedError("%d right-hand sides are above the limit of %d per solve" % (b.shape[1], _lib.PCG_MAX_COLS))
    lam, tol = float(lam), float(tol)
    if not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError("lam must be a positive finite number, got %r" % (lam,))
    if not 0.0 < tol < 1.0:
        raise ValueError("tol must lie in (0, 1), got %r" % (tol,))
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1, got %d" % max_iter)
    if x0 is not None:
        if isinstance(x0, DeviceArray):
            x0 = x0.numpy()
        x0 = np.asarray(x0, dtype=np.float64).reshape(n, -1)
        if x0.shape != b.shape:
            raise ValueError("x0 must have the shape of b %s, got %s" % (b.shape, x0.shape))
    return n, b, lam, tol, max_iter, x0


def pcg_solve(kernel_fn, x, b, lam, precond=None, tol=1e-6, max_iter=1000, x0=None):
    """(K(x, x) + lam I) X = B by block preconditioned conjugate gradients with K applied matrix-free (smn_pcg_solve): a
    PcgResult.  b [N] or [N, C <= 48]; precond a PivotedCholesky of the same kernel on x (any route produced it; M = L L^T +
    lam I) or None (M = lam I); x0 the start (zeros by default).  Each column is its own CG recurrence and stops at
    |r| <= tol |b|; all vectors and inner products are fp64.  Cost per iteration: one kernel_matmul with the active columns."""
    n, b, lam, tol, max_iter, x0 = _check_pcg(kernel_fn, x, b, lam, precond, tol, max_iter, x0)
    xs = kernel_fn.scaled(x)
    ctx, d, c = xs.ctx, xs.shape[1], b.shape[1]
    bd = ctx.to_device(np.ascontiguousarray(b))
    sol = ctx.to_device(np.ascontiguousarray(x0)) if x0 is not None else ctx.empty((n, c), np.float64)
    f = precond.factor if precond is not None and precond.rank > 0 else None
    if f is not None and f.dtype != xs.dtype:
        f = as_device(f, ctx, dtype=xs.dtype)
    m = 0 if f is None else int(f.shape[1])
    iters, info = C.c_int(0), C.c_int(0)
    col_iters = np.zeros(c, dtype=np.int32)
    resid = np.zeros(c, dtype=np.float64)
    hist = np.zeros((max_iter + 1, c), dtype=np.float64)
    net = kernel_fn.params[0]
    ctx.call("smn_pcg_solve", xs.dcode, net, kernel_fn.act, kernel_fn.num_hiddens, kernel_fn.w_std, kernel_fn.b_std,
             kernel_fn.last_w_std, xs.ptr, n, d, d, lam, None if f is None else f.ptr, m, max(m, 1), bd.ptr, c, c, tol, max_iter,
             1 if x0 is not None else 0, sol.ptr, c, C.byref(iters), col_iters.ctypes.data_as(C.POINTER(C.c_int)),
             resid.ctypes.data_as(C.POINTER(C.c_double)), hist.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))
    return PcgResult(sol, iters.value, col_iters, resid, hist[:iters.value + 1].copy(), info.value)
