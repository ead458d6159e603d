"""spax/models.py mirror — SPR (exact GP / Student-t process regression).  SVSP is out of scope
(sparse variational classifier: SURVEY.md section 2, row 7)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DeviceArray, as_device
from ..nt_kernels import CnnKernelFn, KernelFn
from .base import ConstraintTrainVar, Module
from .bijectors import positive
from .utils import jitter

__all__ = ["SPR", "grad_route", "lml_value_and_grads"]


def lml_value_and_grads(terms, quad, logdet, n, df, scale, a=None, b=None):
    """Host part of the analytic gradient, shared by every kernel family: from terms = sum G dK~/d(w_std, b_std,
    last_w_std, eps), quad = y^T K~^-1 y and logdet K~ to (log-pdf, derivatives of the log-pdf with respect to the
    constrained values).  The derivatives come as a dict with keys "w_std", "b_std", "last_w_std", "eps" and, for the
    Student-t head (df = 2a > 0, scale = b/a), "a" and "b"."""
    import math
    from .utils import digamma
    q, ld = quad, logdet
    dlp = {}                                                  # d logpdf / d constrained value
    for key, t in zip(("w_std", "b_std", "last_w_std", "eps"), terms):
        dlp[key] = 0.5 * t
    if df <= 0.0:                                             # likelihoods.py:25-28
        lp = -0.5 * q - 0.5 * n * math.log(2.0 * math.pi) - 0.5 * ld
    else:                                                     # likelihoods.py:45-50, utils.py:178-183
        a_, b_ = a, b
        t = 0.5 * (df + n)
        qs = q / scale
        lp = (-t * math.log1p(qs / df) - 0.5 * n * math.log(df * math.pi) + math.lgamma(t) - math.lgamma(0.5 * df)
              - 0.5 * (ld + n * math.log(scale)))
        d_scale = t * qs / ((df + qs) * scale) - 0.5 * n / scale
        d_df = (-0.5 * math.log1p(qs / df) + t * qs / (df * (df + qs)) - 0.5 * n / df
                + 0.5 * digamma(t) - 0.5 * digamma(0.5 * df))
        dlp["a"] = 2.0 * d_df - d_scale * b_ / (a_ * a_)      # df = 2a, scale = b/a
        dlp["b"] = d_scale / a_
    return lp, dlp


def grad_route(kernel_fn, likelihood):
    """The fused C-ABI entry SPR.loss_and_grad uses for this kernel function and likelihood: "smn_spr_loss_grad" (MLP /
    dense ResNet) or "smn_spr_cnn_loss_grad" (get_cnn_kernel).  Anything else, the conv ResNet included, has no analytic
    gradient: NotImplementedError, which train.build_train_step(method="auto") answers with central differences."""
    if hasattr(likelihood, "lml_params"):
        if isinstance(kernel_fn, KernelFn):
            return "smn_spr_loss_grad"
        if isinstance(kernel_fn, CnnKernelFn) and kernel_fn.entry == "smn_kernel_cnn":
            return "smn_spr_cnn_loss_grad"
    raise NotImplementedError("analytic gradients need an MLP / dense-ResNet KernelFn or a get_cnn_kernel CnnKernelFn and "
                              "a Gaussian or Student-t likelihood; use train.value_and_grad_fd")


class SPR(Module):
    def __init__(self, kernel, likelihood, x_data, y_data, y_mean, y_std, *, eps: float = 1e-6):
        super().__init__()
        self.kernel = kernel
        self.likelihood = likelihood
        self.x_data = as_device(x_data)              # resident in HBM for the life of the model
        self.y_host = np.asarray(y_data, dtype=np.float64).reshape(-1)
        self.y_data = as_device(self.y_host, self.x_data.ctx, dtype=self.x_data.dtype)
        self.y_mean = float(np.asarray(y_mean))
        self.y_std = float(np.asarray(y_std))
        self.num_data = self.x_data.shape[0]
        self.eps = ConstraintTrainVar(eps, constraint=positive())

    def _f64_data(self):
        if self.x_data.dtype == np.float64:
            return self.x_data, self.y_data
        if getattr(self, "_x64", None) is None:
            ctx = self.x_data.ctx
            self._x64 = ctx.to_device(self.x_data.numpy().astype(np.float64))
            self._y64 = ctx.to_device(self.y_host)
        return self._x64, self._y64

    def _student_quad_f64(self, kernel_fn, scale):
        """y^T (K + (1e-6 / scale) I)^-1 y / scale  =  y^T (scale K + 1e-6 I)^-1 y in fp64 (likelihoods.py:60-61).
        It depends on the training data and the hyper-parameters only -- not on the test points -- and the reference's
        evaluation loop calls test_nll twice per check point, on the validation and on the test split
        (experiments/regression/train.py:203-212, test.py:89-99): the value of the last parameter setting is kept, so the
        second call costs the fp32 posterior alone.  (Measured at N = 16384: this fp64 build + factorisation is 44 ms
        against 29 ms for the posterior, and running the two concurrently on two contexts buys 3 % -- both are bound by the
        matrix pipes, not by latency; profiles/r04_two_context_probe.txt.)"""
        key = (tuple(kernel_fn.params), float(scale))
        hit = getattr(self, "_quad64_cache", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        xd, yd = self._f64_data()
        net, act, L, w, b, lw = kernel_fn.params
        quad, info = C.c_double(), C.c_int()
        xd.ctx.call("smn_spr_loss", xd.dcode, net, act, L, w, b, lw, xd.ptr, xd.shape[0], xd.shape[1],
                    xd.shape[1], yd.ptr, 1e-6 / scale, 0.0, 1.0, None, C.byref(quad), None, C.byref(info))
        val = float("nan") if info.value else quad.value / scale
        self._quad64_cache = (key, val)
        return val

    # ---- spax/models.py:93-98
    def loss(self):
        eps = self.eps.safe_value
        kernel_fn = self.kernel.get_kernel_fn()
        if isinstance(kernel_fn, KernelFn) and hasattr(self.likelihood, "lml_params"):
            # fused: build K(X,X)+eps I in the factorisation workspace, factor, carry y through
            df, scale = self.likelihood.lml_params()
            x, ctx = self.x_data, self.x_data.ctx
            net, act, L, w, b, lw = kernel_fn.params
            lp, info = C.c_double(), C.c_int()
            ctx.call("smn_spr_loss", x.dcode, net, act, L, w, b, lw, x.ptr, x.shape[0], x.shape[1], x.shape[1],
                     self.y_data.ptr, eps, df, scale, C.byref(lp), None, None, C.byref(info))
            log_prob = lp.value
        else:
            cov = self.kernel.K(kernel_fn, self.x_data) + jitter(self.num_data, eps=eps)
            log_prob = self.likelihood.prior_logpdf(self.y_host, cov)
        return -log_prob / self.num_data

    def loss_and_grad(self):
        """(loss, {variable name: d loss / d RAW value}) -- the analytic counterpart of
        objax.GradValues(model.loss, model.vars()) in experiments/regression/train.py:61-67.
        One augmented factorisation gives alpha = K~^-1 y, K~^-1, the quadratic form and logdet; one pass over
        the lower triangle contracts G = coef alpha alpha^T - K~^-1 with the forward-mode
        dK/d(w_std, b_std, last_w_std): over X X^T / d for MLP / dense-ResNet kernels (csrc/grad.hip), over the image
        pairs for get_cnn_kernel (csrc/cnn_grad.hip, images of up to 1024 pixels).  The (a, b) derivatives of the
        Student-t head and the softplus chain rule are closed forms on the host (lml_value_and_grads).  Anything else --
        the conv ResNet, a likelihood without lml_params, larger images -- raises NotImplementedError."""
        kernel_fn = self.kernel.get_kernel_fn()
        mlp = grad_route(kernel_fn, self.likelihood) == "smn_spr_loss_grad"
        eps = self.eps.safe_value
        df, scale = self.likelihood.lml_params()
        x, ctx = self.x_data, self.x_data.ctx
        n = self.num_data
        quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
        terms = (C.c_double * 4)()
        if mlp:
            net, act, L, w, b, lw = kernel_fn.params
            ctx.call("smn_spr_loss_grad", x.dcode, net, act, L, w, b, lw, x.ptr, n, x.shape[1], x.shape[1],
                     self.y_data.ptr, eps, df, scale, C.byref(quad), C.byref(logdet), C.byref(info), terms)
        else:
            if len(x.shape) != 4:
                raise ValueError("conv kernel expects x of shape [N,H,W,C]")
            act, L, w, b, lw = kernel_fn.params
            try:
                ctx.call("smn_spr_cnn_loss_grad", x.dcode, act, L, w, b, lw, x.ptr, n, x.shape[1], x.shape[2], x.shape[3],
                         self.y_data.ptr, eps, df, scale, C.byref(quad), C.byref(logdet), C.byref(info), terms)
            except _lib.SmnError as e:
                if e.code == _lib.ENOTSUP:                    # images above the tangent kernel's limit
                    raise NotImplementedError(str(e)) from e
                raise
        nan = float("nan")
        if info.value != 0:
            return nan, {k: nan for k in self.vars()}
        student = df > 0.0
        lp, dlp = lml_value_and_grads(terms, quad.value, logdet.value, n, df, scale,
                                      self.likelihood.a.safe_value if student else None,
                                      self.likelihood.b.safe_value if student else None)
        owners = {"w_std": self.kernel.w_std, "b_std": self.kernel.b_std, "last_w_std": self.kernel.last_w_std,
                  "eps": self.eps}
        if student:
            owners.update(a=self.likelihood.a, b=self.likelihood.b)
        names = {id(v): k for k, v in self.vars().items()}
        grads = {}
        for key, g in dlp.items():
            var = owners[key]
            grads[names[id(var)]] = float(-g / n * var.constraint.grad(var.value))
        return -lp / n, grads

    # ---- spax/models.py:100-120
    def test_nll(self, x, y):
        eps = self.eps.safe_value
        kernel_fn = self.kernel.get_kernel_fn()
        mean, cov = self.kernel.predict(kernel_fn, self.x_data, self.y_data, x, eps=eps)
        require = self.likelihood.require
        if require:
            if "cov_data" in require:
                if isinstance(kernel_fn, KernelFn):
                    # likelihoods.py:60-61 needs y^T (b/a K + 1e-6 I)^-1 y with K WITHOUT the eps jitter
                    # (models.py:107 "TODO: check"); hand the quadratic form over instead of an N x N matrix.
                    # That matrix carries only a 1e-6 jitter: in fp32 it is not numerically PD (the
                    # reference's fp32 inv() returns noise there), so this one quadratic form always runs
                    # in fp64 on upcast copies of the training data.
                    cov_data = self._student_quad_f64(kernel_fn, self.likelihood.lml_params()[1])
                else:
                    cov_data = self.kernel.K(kernel_fn, self._f64_data()[0])   # fp64 for the same reason
            aux_dict = dict(cov_data=cov_data, y_data=self.y_host)
            aux = tuple(aux_dict[k] for k in require)
        else:
            aux = None

        y = np.asarray(y, dtype=np.float64)
        log_prob = self.likelihood.logpdf(
            (y * self.y_std) + self.y_mean,
            (np.asarray(mean, dtype=np.float64).flatten() * self.y_std) + self.y_mean,
            cov * self.y_std ** 2 if isinstance(cov, DeviceArray) else np.asarray(cov, dtype=np.float64) * self.y_std ** 2,
            aux,
        )
        ll = np.mean(log_prob)
        return -ll
