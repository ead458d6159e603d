"""Fit once, predict many: a fitted exact-GP posterior that lives on the device (csrc/fit.hip, the smn_fit_* entries).

`SPR.posterior()` / `MultiSPR.posterior()` factor K~ = K_dd + eps tr(K_dd)/N I once -- the posterior of the models' own
`predict` -- and return a FittedPosterior that answers `predict`, `test_nll`, `sample`, `classify` for test sets of any size at
O(N^2 T) per call instead of O(N^3).  The object is a snapshot: the hyper-parameters, the ridge, the likelihood's (df, scale)
and the Student-t quadratic form are those of the moment it was made; moving the model's variables afterwards does not reach
it.  `gradient_descent_mse_ensemble(..., cache=True)` serves its t = None posterior from one of these.

MLP / dense-ResNet kernel functions (under NNGPKernel or NTKKernel) take the fused entries: the cross kernel K(x_chunk, X) is
built straight into the state.  The conv kernels and any other callable take the matrix form: K_dd once at creation, then per
chunk of test points kernel_fn(x_chunk, x_train), the prior variances (smn_kernel_conv_diag for the conv kernels) and, for
cov="full", kernel_fn(x_chunk, None).

The training set can grow: `post.append(x, y)` adds observations at O(N^2 k) without refitting, under the ridge the state
froze when it was made (`post.ridge`, absolute for every later point), and `post.reserve(max_points)` makes room up front.
The fused form hands the new inputs to smn_fit_append; the matrix form builds kernel_fn(x_chunk, x_train) and the lower
kernel_fn(x_chunk, None) per chunk of `capacity` points for smn_fit_append_from_kernel and keeps x_train as the concatenation.

And it can shrink: `post.remove(indices)` takes observations out at O(N^2 k), again without refitting and under the same frozen
ridge (smn_fit_remove: an orthogonal re-triangularisation of the kept rows of L, no kernel is evaluated) -- a sliding window
over a stream is `remove(range(k))` + `append`, and removing the points just appended undoes the append bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeviceArray, as_device
from .nt_kernels import CnnKernelFn, KernelFn

__all__ = ["FittedPosterior", "chunks", "normalise_indices"]


def chunks(T, capacity):
    """[(start, rows)] covering T test rows in order, at most `capacity` rows each: the chunking of smn_fit_predict."""
    T, capacity = int(T), int(capacity)
    if T < 0 or capacity < 1:
        raise ValueError("chunks: T must be >= 0 and capacity >= 1, got T = %d, capacity = %d" % (T, capacity))
    return [(s, min(capacity, T - s)) for s in range(0, T, capacity)]


def _rows(arr, start, rows):
    """Rows [start, start + rows) of a host array or of a plain row-major DeviceArray (a view: no copy)."""
    if not isinstance(arr, DeviceArray):
        return arr[start:start + rows]
    per_row = int(np.prod(arr.shape[1:])) if len(arr.shape) > 1 else 1
    view = DeviceArray(arr.ctx, (rows,) + tuple(arr.shape[1:]), arr.dtype,
                       ptr=C.c_void_p(arr.ptr.value + start * per_row * arr.dtype.itemsize), owner=False)
    view._base = arr if arr._base is None else arr._base
    return view


def _as2d(arr):
    """[N, ...] -> [N, features] of a plain row-major DeviceArray, as a view (what KernelFn does by a host round trip)."""
    if len(arr.shape) == 2:
        return arr
    view = DeviceArray(arr.ctx, (arr.shape[0], int(np.prod(arr.shape[1:])) if len(arr.shape) > 1 else 1), arr.dtype, ptr=arr.ptr,
                       owner=False)
    view._base = arr if arr._base is None else arr._base
    return view


def normalise_indices(indices, n):
    """`indices` (an int, a sequence / array of ints, or a boolean mask of length n; negative values count from the end) as a
    sorted int64 array of distinct values in [0, n).  ValueError: empty, out of range, duplicates after normalisation, a mask
    of another length, anything that is not integral."""
    n = int(n)
    arr = np.asarray(indices)
    if arr.dtype == np.bool_:
        if arr.shape != (n,):
            raise ValueError("a boolean mask must have shape (%d,), the training points; got %s" % (n, arr.shape))
        arr = np.flatnonzero(arr)
    else:
        arr = np.atleast_1d(arr)
        if arr.ndim != 1 or not (arr.size == 0 or np.issubdtype(arr.dtype, np.integer)):
            raise ValueError("indices must be an int, a 1-d sequence of ints or a boolean mask, got dtype %s, shape %s"
                             % (arr.dtype, arr.shape))
    if arr.size == 0:
        raise ValueError("remove needs at least one point: the selection is empty")
    arr = arr.astype(np.int64)
    bad = arr[(arr < -n) | (arr >= n)]
    if bad.size:
        raise ValueError("index %d is out of range for %d training points" % (int(bad[0]), n))
    arr = np.sort(np.where(arr < 0, arr + n, arr))
    dup = arr[1:][arr[1:] == arr[:-1]]
    if dup.size:
        raise ValueError("index %d is given more than once" % int(dup[0]))
    return arr


def _at(arr, elems):
    return C.c_void_p(arr.ptr.value + int(elems) * arr.dtype.itemsize)


class FittedPosterior:
    """See the module docstring.  Attributes: quad [C] (y_k^T K~^-1 y_k), logdet (log det K~), info (0, or the failing pivot
    of a matrix that is not positive definite: every prediction is then NaN), num_data, num_outputs, capacity, nbytes (device
    memory the state owns), hyper (the snapshot: w_std, b_std, last_w_std, eps, df, scale), ridge (lambda = ridge_abs +
    ridge_rel tr(K_dd) / n as the device applied it at creation: the absolute ridge of every point appended later), max_points
    (training points the state has room for; a multiple of 128)."""

    def __init__(self, kernel_fn, x, y, *, ridge_rel=0.0, ridge_abs=0.0, capacity=2048, mode="nngp", ctx=None, reserve=None):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be at least 1, got %d" % capacity)
        if mode not in ("nngp", "ntk"):
            raise ValueError("mode must be 'nngp' or 'ntk', got %r" % (mode,))
        if reserve is not None and int(reserve) < int(x.shape[0]):
            raise ValueError("reserve = %d is below the %d training points" % (int(reserve), int(x.shape[0])))
        self.ctx = ctx or getattr(kernel_fn, "ctx", None) or getattr(x, "ctx", None) or _lib.default_context()
        self._handle = None
        self.kernel_fn, self.mode, self.capacity = kernel_fn, mode, capacity
        self._x_train, self._x_pending = x, []
        self._y_first, self._y_parts = y, None
        self._quad_model, self._student_quad, self._student_stale = None, None, False
        self.label_targets = None
        self.dtype = np.dtype(x.dtype)
        self.num_data = int(x.shape[0])
        self.num_outputs = int(y.shape[1]) if len(y.shape) > 1 else 1
        self.fused = isinstance(kernel_fn, KernelFn)
        self.multi = False
        self.y_mean, self.y_std = 0.0, 1.0
        self.df, self.scale, self.student_quad = 0.0, 1.0, None
        self.hyper = {"eps": float(ridge_rel)}
        for name in ("w_std", "b_std", "last_w_std"):
            if hasattr(kernel_fn, name):
                self.hyper[name] = float(getattr(kernel_fn, name))
        n, c, code = self.num_data, self.num_outputs, _lib.dtype_code(self.dtype)
        quad, logdet, info, handle = (C.c_double * c)(), C.c_double(), C.c_int(), C.c_void_p()
        if self.fused:
            x2 = _as2d(x)
            self.num_features = int(x2.shape[1])
            x2 = self._scaled(x2)          # input scales: the state is fitted on s o x (x_train stays what was handed in)
            net, act, depth, w, b, lw = kernel_fn.with_cov(mode).params      # "ntk": net carries SMN_NET_NTK
            self.ctx.call("smn_fit_create", code, net, act, depth, w, b, lw, x2.ptr, n, self.num_features, self.num_features,
                          y.ptr, c, float(ridge_rel), float(ridge_abs), capacity, C.byref(handle), quad, C.byref(logdet),
                          C.byref(info))
        else:
            k_dd = self._kernel(x, None, fill="lower")
            self.ctx.call("smn_fit_create_from_kernel", code, k_dd.ptr, n, n, y.ptr, c, float(ridge_rel), float(ridge_abs),
                          capacity, C.byref(handle), quad, C.byref(logdet), C.byref(info))
        self._handle = handle
        self.quad = np.array(list(quad), dtype=np.float64)
        self.logdet, self.info = float(logdet.value), int(info.value)
        nbytes = C.c_size_t()
        self.ctx.call_on("smn_fit_info", self._handle, None, None, None, C.byref(nbytes))
        self.nbytes = int(nbytes.value)
        max_points, ridge = C.c_int64(), C.c_double()
        self.ctx.call_on("smn_fit_stats", self._handle, C.byref(max_points), C.byref(ridge), None, None)
        self.ridge, self.max_points = float(ridge.value), int(max_points.value)
        if reserve is not None:
            self.reserve(reserve)

    def _scaled(self, x2):
        """x2 [rows, d] as the fused state sees it: multiplied by the kernel function's input scales (the snapshot taken with
        the kernel function), or x2 itself."""
        s = getattr(self.kernel_fn, "input_scales", None)
        if s is None:
            return x2
        if x2.shape[1] != s.shape[0]:
            raise ValueError("input_scales has %d entries for inputs with %d features" % (s.shape[0], x2.shape[1]))
        return self.kernel_fn.scaled(x2, self.ctx)

    @classmethod
    def from_model(cls, model, capacity=2048, reserve=None):
        """The posterior of `model.predict` at the model's current hyper-parameters (SPR or MultiSPR)."""
        from .spax.kernels import NTKKernel
        if not hasattr(model.likelihood, "lml_params"):
            raise NotImplementedError("posterior() needs a Gaussian or Student-t likelihood")
        kernel_fn = model.kernel.get_kernel_fn()
        mode = "ntk" if isinstance(model.kernel, NTKKernel) else "nngp"
        df, scale = model.likelihood.lml_params()
        student_quad = model._draws_quad(kernel_fn, scale) if df > 0.0 else None
        post = cls(kernel_fn, model.x_data, model.y_data, ridge_rel=model.eps.safe_value, capacity=capacity, mode=mode,
                   ctx=model.x_data.ctx, reserve=reserve)
        post.multi = hasattr(model, "num_outputs")
        post.y_mean, post.y_std = float(model.y_mean), float(model.y_std)
        post.df, post.scale, post.student_quad = float(df), float(scale), student_quad
        post.hyper.update(df=float(df), scale=float(scale))
        post._quad_model = model
        post._y_parts = [np.asarray(model.y_host, dtype=np.float64).reshape(post.num_data, post.num_outputs)]
        if getattr(model, "_from_labels", False):
            post.label_targets = model.label_targets   # the model's own onehot(labels) - 1/C rule
        return post

    # ---- the training inputs: what was handed in at creation, then every appended chunk; joined when someone reads them
    @property
    def x_train(self):
        if self._x_pending:
            host = lambda a: a.raw_numpy() if isinstance(a, DeviceArray) else np.asarray(a)   # noqa: E731
            parts = [host(self._x_train)] + [host(p) for p in self._x_pending]
            joined = np.concatenate([p.reshape((p.shape[0],) + parts[0].shape[1:]) for p in parts], axis=0)
            self._x_train = as_device(joined, self.ctx, dtype=self.dtype) if isinstance(self._x_train, DeviceArray) else joined
            self._x_pending = []
        return self._x_train

    @x_train.setter
    def x_train(self, x):
        self._x_train, self._x_pending = x, []

    # ---- the Student-t head's quadratic form y^T ((b/a) K + 1e-6 I)^-1 y: another matrix than K~, so an append cannot carry
    # it forward from L; it goes stale there and is recomputed over all the points by the model's own fp64 route when read
    @property
    def student_quad(self):
        if self._student_stale:
            m = self._quad_model
            y = np.concatenate(self._y_parts, axis=0)
            shadow = type(m)(m.kernel, m.likelihood, self.x_train, y if self.multi else y.reshape(-1), m.y_mean, m.y_std,
                             eps=m.eps.safe_value)
            self._student_quad = shadow._draws_quad(self.kernel_fn, self.scale)
            self._student_stale = False
        return self._student_quad

    @student_quad.setter
    def student_quad(self, value):
        self._student_quad, self._student_stale = value, False

    def _sync_stats(self):
        """num_data, nbytes, max_points, quad, logdet from the device state."""
        n, nbytes, max_points = C.c_int64(), C.c_size_t(), C.c_int64()
        quad, logdet = (C.c_double * self.num_outputs)(), C.c_double()
        self.ctx.call_on("smn_fit_info", self._handle, C.byref(n), None, None, C.byref(nbytes))
        self.ctx.call_on("smn_fit_stats", self._handle, C.byref(max_points), None, quad, C.byref(logdet))
        self.num_data, self.nbytes, self.max_points = int(n.value), int(nbytes.value), int(max_points.value)
        self.quad, self.logdet = np.array(list(quad), dtype=np.float64), float(logdet.value)

    # ---- growing the training set
    def reserve(self, max_points):
        """Room for up to `max_points` training points (smn_fit_reserve): one O(N^2) copy of the factor into a larger
        allocation -- old and new state are both alive while it runs --, after which appends up to that size neither copy
        nor allocate (`nbytes` stays put).  Within the current room (`max_points`, a multiple of 128) nothing happens.  The
        state predicts as before at once; per-call cost follows the reserved size, and since the read-out's sums run over
        the padded row the last bits of a prediction may differ from the unreserved state's."""
        if self._handle is None:
            raise ValueError("this FittedPosterior is closed")
        max_points = int(max_points)
        if max_points < self.num_data:
            raise ValueError("reserve: max_points = %d is below the %d training points" % (max_points, self.num_data))
        self.ctx.call_on("smn_fit_reserve", self._handle, max_points)
        self._sync_stats()
        return self

    def _check_append(self, x, y):
        """Everything about append's arguments that needs no device; returns (k, y as a host [k, C] float64 array or None
        when y is a device array of the right shape)."""
        if self._handle is None:
            raise ValueError("this FittedPosterior is closed")
        xs = tuple(int(s) for s in getattr(x, "shape", np.shape(x)))
        if len(xs) < 1 or xs[0] < 1:
            raise ValueError("append needs at least one new point, got x of shape %s" % (xs,))
        k, c = xs[0], self.num_outputs
        if self.fused:
            feats = int(np.prod(xs[1:])) if len(xs) > 1 else 1
            if feats != self.num_features:
                raise ValueError("x has %d features, the training data %d" % (feats, self.num_features))
        else:
            tail = tuple(int(s) for s in self._x_train.shape[1:])
            if xs[1:] != tail:
                raise ValueError("x has rows of shape %s, the training data %s" % (xs[1:], tail))
        if isinstance(y, DeviceArray):
            ys = tuple(y.shape)
            if ys != (k, c) and not (c == 1 and ys == (k,)):
                raise ValueError("y must be [%d] or [%d, %d], got %s" % (k, k, c, ys))
            return k, None
        y = np.asarray(y)
        if self.label_targets is not None and y.ndim == 1 and np.issubdtype(y.dtype, np.integer):
            y = self.label_targets(y, c)
        y = np.asarray(y, dtype=np.float64)
        if y.ndim == 1 and c == 1:
            y = y[:, None]
        if y.shape != (k, c):
            raise ValueError("y must be [%d] or [%d, %d] (C = %d outputs), got %s" % (k, k, c, c, y.shape))
        return k, y

    def append(self, x, y):
        """Add k observations (x [k, ...] in the training inputs' layout, y [k] or [k, C] in the units of the training
        targets; host or device arrays; integer labels for a posterior of MultiSPR.from_labels) without refitting:
        O(N^2 k + N k^2 + k^3) (smn_fit_append / smn_fit_append_from_kernel).  Returns self.

        THE RIDGE IS FROZEN: `ridge` = ridge_abs + ridge_rel tr(K_dd)/n0 is fixed when the state is made and every appended
        point gets it as an absolute ridge.  After any appends the state is the posterior of all N points under
        K(X, X) + ridge I -- what FittedPosterior(..., ridge_rel=0, ridge_abs=post.ridge) on all the points gives --, not the
        fit whose relative ridge is recomputed at the new N; the two coincide when the kernel's diagonal is constant.

        A state without room (`max_points`) grows itself to max(N + k, 1.5 N) points rounded up to 128 -- an O(N^2) copy
        with both states alive; `reserve` first to avoid it.  k > capacity goes in chunks of `capacity` points, each seeing
        the earlier ones as training points.  A chunk whose Schur complement is not positive definite is not taken:
        numpy.linalg.LinAlgError names the pivot and how many points did go in, and the state stays usable at that size.
        Updates num_data, quad, logdet, nbytes, max_points; the next predict_grad rebuilds what it keeps beside the factor.
        Student-t likelihood: the quadratic form of predictive_params / test_nll / sample belongs to another matrix,
        (b/a) K + 1e-6 I, and is recomputed over all N points by the model's fp64 route at the first call that reads it --
        one fp64 O(N^3) factorisation --; predict, predict_grad and classify never read it and stay O(N^2 k).  The degrees
        of freedom use the new N."""
        k, y_host = self._check_append(x, y)
        ctx, c, n_before = self.ctx, self.num_outputs, self.num_data
        xd = as_device(x, ctx, dtype=self.dtype)
        yd = as_device(y, ctx, dtype=self.dtype) if y_host is None else ctx.to_device(np.ascontiguousarray(y_host, dtype=self.dtype))
        if y_host is None:
            y_host = np.asarray(yd.raw_numpy(), dtype=np.float64).reshape(k, c)
        quad, logdet, info = (C.c_double * c)(), C.c_double(), C.c_int()
        if self.fused:
            x2 = self._scaled(_as2d(xd))
            ctx.call_on("smn_fit_append", self._handle, x2.ptr, k, self.num_features, yd.ptr, quad, C.byref(logdet), C.byref(info))
            self._sync_stats()
            went = self.num_data - n_before
            if went:   # (a host array is copied: the caller may reuse it; a device array is kept as a view)
                self._x_pending.append(_rows(xd, 0, went) if isinstance(x, DeviceArray) else np.array(np.asarray(x)[:went]))
        else:
            went = 0
            for start, rows in chunks(k, self.capacity):
                xc = _rows(xd, start, rows)
                k_nd = self._kernel(xc, self.x_train)
                k_nn = self._kernel(xc, None, fill="lower")
                n = self.num_data
                ctx.call_on("smn_fit_append_from_kernel", self._handle, k_nd.ptr, rows, n, n, k_nn.ptr, rows, _at(yd, start * c), quad,
                            C.byref(logdet), C.byref(info))
                self._sync_stats()
                if info.value != 0:
                    break
                went += rows
                self._x_pending.append(xc)
                self.x_train   # (joined now: the next chunk's cross kernel is against all of them)
        if went:
            if self._y_parts is None:
                self._y_parts = [np.asarray(self._y_first.raw_numpy(), dtype=np.float64).reshape(n_before, c)]
            self._y_parts.append(y_host[:went])
            self._y_first = None
            if self.df > 0.0:
                self._student_stale = True
        if info.value != 0:
            raise np.linalg.LinAlgError("append: the Schur complement of the new points is not positive definite at pivot %d "
                                        "(1-based, among all training points); %d of the %d new points went in and the state "
                                        "holds %d" % (info.value, went, k, self.num_data))
        return self

    # ---- shrinking the training set
    def remove(self, indices):
        """Take k observations out without refitting (smn_fit_remove): O(N^2 k) -- about m^2 (64 + 32)^2 / 64 flops per pass
        of at most 32 points for the m points behind the first removed one -- instead of O(N^3); removing exactly the last k
        points costs O(N k) and undoes an `append` of them bit for bit.  Returns self.

        `indices`: an int, a sequence or array of ints, or a boolean mask of length num_data; negative values count from the
        end; a value given twice (after that normalisation) is a ValueError, as are an empty selection, one that takes every
        point (a posterior keeps at least one) and a value out of range -- all before any device call.  A REMOVED POINT'S INDEX
        SHIFTS THE LATER ONES DOWN: after remove([3]) the old point 4 is point 3, as with numpy.delete; all the indices of one
        call refer to the numbering before it.

        THE RIDGE IS FROZEN, as for `append`: `ridge` stays what it was when the state was made, so afterwards the state is
        the posterior of the kept points under K(X_R, X_R) + ridge I -- what FittedPosterior(..., ridge_rel=0,
        ridge_abs=post.ridge) on the kept points gives --, not the fit whose relative ridge is recomputed on them.

        No kernel is evaluated (fused and matrix-form posteriors go through the same entry); the kept rows of the factor are
        re-triangularised by orthogonal transformations, which is backward stable and cannot fail.  `max_points` and `nbytes`
        stay as they are (the room is kept for later appends).  Updates num_data, quad, logdet, x_train; the next predict_grad
        rebuilds what it keeps beside the factor; under a Student-t likelihood the quadratic form is recomputed over the kept
        points at the first call that reads it, as after an append."""
        if self._handle is None:
            raise ValueError("this FittedPosterior is closed")
        n, c = self.num_data, self.num_outputs
        idx = normalise_indices(indices, n)
        if idx.size >= n:
            raise ValueError("remove: the selection takes all %d training points; a posterior keeps at least one" % n)
        quad, logdet = (C.c_double * c)(), C.c_double()
        self.ctx.call_on("smn_fit_remove", self._handle, idx.ctypes.data_as(C.POINTER(C.c_int64)), int(idx.size), quad, C.byref(logdet))
        keep = np.ones(n, dtype=bool)
        keep[idx] = False
        x = self.x_train                                       # (joined)
        if isinstance(x, DeviceArray):
            self._x_train = as_device(np.ascontiguousarray(x.raw_numpy()[keep]), self.ctx, dtype=self.dtype)
        else:
            self._x_train = np.asarray(x)[keep]
        if self._y_parts is None:
            self._y_parts = [np.asarray(self._y_first.raw_numpy(), dtype=np.float64).reshape(n, c)]
        self._y_parts = [np.concatenate(self._y_parts, axis=0)[keep]]
        self._y_first = None
        if self.df > 0.0:
            self._student_stale = True
        self._sync_stats()
        return self

    # ---- lifetime
    def close(self):
        """Free the device state (idempotent).  A state whose context is already closed is left to the driver."""
        handle, self._handle = getattr(self, "_handle", None), None
        if handle is not None and getattr(self.ctx, "handle", None):
            self.ctx.call_on("smn_fit_destroy", handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- kernel pieces of the matrix form
    def _kernel(self, x1, x2, fill="full"):
        if isinstance(self.kernel_fn, CnnKernelFn):
            if self.mode != "nngp":
                raise NotImplementedError("the conv kernels are NNGP-only")
            return self.kernel_fn(x1, x2, get="nngp", fill=fill)
        host = lambda a: None if a is None else np.asarray(a)   # noqa: E731  (what predict_fn hands such a callable)
        return as_device(self.kernel_fn(host(x1), host(x2), self.mode), self.ctx, dtype=self.dtype)

    def _prior_var(self, xc):
        """K(x_t, x_t) [rows] for the matrix form: the per-image pass of the conv kernels (the bits of their symmetric
        diagonal); for any other callable the diagonal of kernel_fn(x, None)."""
        fn = self.kernel_fn
        if isinstance(fn, CnnKernelFn):
            return fn.diag(as_device(xc, self.ctx, dtype=self.dtype))
        return self.ctx.to_device(np.ascontiguousarray(self._kernel(xc, None).diagonal(), dtype=self.dtype))

    # ---- predictions
    def predict(self, x, cov="diag"):
        """(mean [T,C], var [T]) for cov="diag", (mean, cov [T,T]) for cov="full", mean alone for cov=None: device arrays in
        normalised units.  Any T for "diag" / None -- nothing of size T x T is formed --; "full" needs T <= capacity."""
        if cov not in ("diag", "full", None):
            raise ValueError("cov must be 'diag', 'full' or None, got %r" % (cov,))
        if self._handle is None:
            raise ValueError("this FittedPosterior is closed")
        ctx, c = self.ctx, self.num_outputs
        xt = as_device(x, ctx, dtype=self.dtype)
        t = int(xt.shape[0])
        if t < 1:
            raise ValueError("predict needs at least one test point")
        if cov == "full" and t > self.capacity:
            raise ValueError("cov='full' needs T = %d <= capacity = %d (the T x T Schur block sits behind the factor); make the "
                             "posterior with a larger capacity or ask for cov='diag'" % (t, self.capacity))
        mean = ctx.empty((t, c), self.dtype)
        var = ctx.empty((t,), self.dtype) if cov == "diag" else None
        full = ctx.empty((t, t), self.dtype) if cov == "full" else None
        vptr, cptr = (None if var is None else var.ptr), (None if full is None else full.ptr)
        if self.fused:
            xt = _as2d(xt)
            if xt.shape[1] != self.num_features:
                raise ValueError("x has %d features, the training data %d" % (xt.shape[1], self.num_features))
            xt = self._scaled(xt)
            ctx.call_on("smn_fit_predict", self._handle, xt.ptr, t, xt.shape[1], mean.ptr, vptr, cptr, t)
        else:
            n = self.num_data
            for start, rows in chunks(t, self.capacity):
                xc = _rows(xt, start, rows)
                k_td = self._kernel(xc, self.x_train)
                ktt = self._prior_var(xc) if cov == "diag" else None
                k_tt = self._kernel(xc, None) if cov == "full" else None
                ctx.call_on("smn_fit_apply", self._handle, k_td.ptr, rows, n, None if ktt is None else ktt.ptr,
                            None if k_tt is None else k_tt.ptr, rows, _at(mean, start * c),
                            None if var is None else _at(var, start), cptr, t)
        if cov is None:
            return mean
        return mean, (var if cov == "diag" else full)

    def predict_grad(self, x, mean=True, var=True):
        """(dmean [T,C,d], dvar [T,d]): the derivatives of `predict(x, cov="diag")` with respect to the test inputs, as device
        arrays (None for the one not asked for); any T.  Units are those of `predict`: normalised targets, per unit of the
        input features as they are handed in, so in target units d mean is y_std * dmean and d var is y_std^2 * dvar.  Under
        the Student-t likelihood the predictive scale^2 is shape * var with predictive_params()'s shape, so its gradient is
        shape * dvar.  Fused posteriors (MLP / dense-ResNet kernel functions); the first call adds the transposed factor,
        alpha and X^T to the device state (`nbytes` grows).

        A matrix-form posterior over get_cnn_kernel returns saliency maps, (dmean [T,C,H,W,Cin], dvar [T,H,W,Cin]), for
        images of at most 1024 pixels: per chunk of `capacity` rows kernel_fn(x_chunk, x_train), smn_fit_weights for
        U = K_td K~^-1 and one smn_kernel_cnn_input_grad_cross call with the seeds alpha = K~^-1 Y (fetched once per call),
        gbar = -2 U and gdiag = 1 -- one forward and one reverse sweep per (test, training) pair for all C + 1 seeds.  The
        partner lists are cut by the chunk's size, so a row's last bits may depend on the rows it shares a chunk with.
        Every other matrix-form posterior (the pooled kernel, the conv ResNet, foreign callables) has no input derivative."""
        if not self.fused:
            fn = getattr(self, "kernel_fn", None)
            if not (isinstance(fn, CnnKernelFn) and fn.entry == "smn_kernel_cnn"):
                raise NotImplementedError("predict_grad needs an MLP / dense-ResNet kernel function or get_cnn_kernel: the "
                                          "pooled kernel, the conv ResNet and foreign callables (matrix-form posteriors) have "
                                          "no input derivative here")
            return self._predict_grad_cnn(x, mean, var)
        if self._handle is None:
            raise ValueError("this FittedPosterior is closed")
        if not (mean or var):
            raise ValueError("predict_grad: ask for mean, var or both")
        ctx, c = self.ctx, self.num_outputs
        xt = _as2d(as_device(x, ctx, dtype=self.dtype))
        t, d = int(xt.shape[0]), self.num_features
        if t < 1:
            raise ValueError("predict_grad needs at least one test point")
        if xt.shape[1] != d:
            raise ValueError("x has %d features, the training data %d" % (xt.shape[1], d))
        dmean = ctx.empty((t, c, d), self.dtype) if mean else None
        dvar = ctx.empty((t, d), self.dtype) if var else None
        xt = self._scaled(xt)
        ctx.call_on("smn_fit_predict_grad", self._handle, xt.ptr, t, d, None if dmean is None else dmean.ptr,
                    None if dvar is None else dvar.ptr)
        s = getattr(self.kernel_fn, "input_scales", None)
        if s is not None:              # per unit of the inputs as handed in: d/dx = s o d/d(s o x)
            sv = np.ascontiguousarray(s, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
            for g, rows in ((dmean, t * c), (dvar, t)):
                if g is not None:
                    ctx.call("smn_scale_columns", g.dcode, g.ptr, rows, d, d, sv, g.ptr, d)
        nbytes = C.c_size_t()
        ctx.call_on("smn_fit_info", self._handle, None, None, None, C.byref(nbytes))
        self.nbytes = int(nbytes.value)
        return dmean, dvar

    def _predict_grad_cnn(self, x, mean, var):
        """predict_grad of a matrix-form posterior over get_cnn_kernel (see there)."""
        if self._handle is None:
            raise ValueError("this FittedPosterior is closed")
        if not (mean or var):
            raise ValueError("predict_grad: ask for mean, var or both")
        if self.mode != "nngp":
            raise NotImplementedError("the conv kernels are NNGP-only")
        fn, ctx, c = self.kernel_fn, self.ctx, self.num_outputs
        shape = tuple(int(s) for s in getattr(x, "shape", np.shape(x)))
        tail = tuple(int(s) for s in self._x_train.shape[1:])
        if len(shape) != 4 or shape[1:] != tail:
            raise ValueError("x has rows of shape %s, the training data %s" % (shape[1:], tail))
        if shape[0] < 1:
            raise ValueError("predict_grad needs at least one test point")
        t, h, w, cin = shape
        fn._check_input_grad(h, w)                           # above 1024 pixels: NotImplementedError before any device call
        xt = as_device(x, ctx, dtype=self.dtype)
        x_train = as_device(self.x_train, ctx, dtype=self.dtype)
        n, code = self.num_data, _lib.dtype_code(self.dtype)
        dmean = ctx.empty((t, c, h, w, cin), self.dtype) if mean else None
        dvar = ctx.empty((t, h, w, cin), self.dtype) if var else None
        alpha = None
        if mean:
            alpha = ctx.empty((n, c), self.dtype)
            ctx.call_on("smn_fit_weights", self._handle, None, 0, n, None, n, alpha.ptr)
        if var:
            ones = ctx.to_device(np.ones(min(self.capacity, t), dtype=self.dtype))
            minus2 = np.full(n, -2.0).ctypes.data_as(C.POINTER(C.c_double))
        per_row = h * w * cin
        for start, rows in chunks(t, self.capacity):
            xc = _rows(xt, start, rows)
            u = None
            if var:
                k_td = self._kernel(xc, x_train)
                u = ctx.empty((rows, n), self.dtype)
                ctx.call_on("smn_fit_weights", self._handle, k_td.ptr, rows, n, u.ptr, n, None)
                ctx.call("smn_scale_columns", code, u.ptr, rows, n, n, minus2, u.ptr, n)       # gbar = -2 U
            ctx.call("smn_kernel_cnn_input_grad_cross", code, fn.act, fn.num_hiddens, fn.w_std, fn.b_std, fn.last_w_std,
                     xc.ptr, rows, x_train.ptr, n, h, w, cin, None if alpha is None else alpha.ptr, c,
                     None if u is None else u.ptr, n, ones.ptr if var else None,
                     None if dmean is None else _at(dmean, start * c * per_row), None if dvar is None else _at(dvar, start * per_row))
        nbytes = C.c_size_t()
        ctx.call_on("smn_fit_info", self._handle, None, None, None, C.byref(nbytes))
        self.nbytes = int(nbytes.value)
        return dmean, dvar

    def _marginals(self, x):
        mean, var = self.predict(x, cov="diag")
        return (np.asarray(mean.raw_numpy(), dtype=np.float64) * self.y_std + self.y_mean,
                np.asarray(var.raw_numpy(), dtype=np.float64) * self.y_std ** 2)

    def test_nll(self, x, y):
        """The model's test_nll (SPR: mean over points; MultiSPR: mean over points of the sum over outputs) from the
        predictive marginals alone: any number of test points."""
        from .spax.likelihoods import _norm_logpdf, _t_logpdf
        ms, var = self._marginals(x)
        t, c = ms.shape
        ys = np.asarray(y, dtype=np.float64).reshape(t, c) * self.y_std + self.y_mean
        if self.df > 0.0:
            cond_df = self.df + self.num_data * c
            sigma = np.sqrt((self.df + self.student_quad) / cond_df * self.scale * var)
            lp = _t_logpdf(ys, cond_df, ms, sigma[:, None])
        else:
            lp = _norm_logpdf(ys, ms, np.sqrt(var)[:, None])
        return -float(np.mean(np.sum(lp, axis=1)))

    def predictive_params(self):
        """(df_post, shape) of the joint predictive law, as the model's predictive_params."""
        if not self.df > 0.0:
            return None, 1.0
        df_post = self.df + self.num_data * self.num_outputs
        return df_post, (self.df + self.student_quad) / df_post * self.scale

    def sample(self, key, x, num_samples, jitter=1e-6):
        """num_samples joint draws of the latent function at x ([S,T], or [S,T,C] from a MultiSPR): sample_posterior's
        composition -- smn_cholesky of the covariance with the relative ridge `jitter`, then smn_mvn_draws -- on
        predict(x, cov="full"); T <= capacity."""
        from .spax.priors import split_key
        seed, point0 = split_key(key)
        s = int(num_samples)
        if s < 1:
            raise ValueError("num_samples must be at least 1")
        df_post, shape = self.predictive_params()
        mean, cov = self.predict(x, cov="full")
        ctx = self.ctx
        t, c = mean.shape
        out_shape = (s, t, c) if self.multi else (s, t)
        nan = lambda: ctx.to_device(np.full(out_shape, np.nan, dtype=mean.dtype))   # noqa: E731
        if df_post is not None and not (np.isfinite(shape) and shape > 0.0):
            return nan()
        info = C.c_int()
        ctx.call("smn_cholesky", cov.dcode, cov.ptr, t, t, t, t, 0.0, float(jitter), C.byref(info), None)
        if info.value != 0:
            return nan()
        out = ctx.empty(out_shape, mean.dtype)
        ctx.call("smn_mvn_draws", mean.dcode, mean.ptr, cov.ptr, t, t, c, s, df_post or 0.0, shape, seed, point0, None, None,
                 out.ptr)
        return out

    def classify(self, x):
        """Predicted labels (a posterior made from a MultiSPR): argmax_c of the posterior mean, first maximum."""
        if not self.multi:
            raise NotImplementedError("classify / accuracy belong to a posterior made from a MultiSPR")
        return np.argmax(np.asarray(self.predict(x, cov=None).raw_numpy(), dtype=np.float64), axis=1)

    def accuracy(self, x, labels):
        return float(np.mean(self.classify(x) == np.asarray(labels).reshape(-1)))
