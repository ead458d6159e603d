"""spax/models.py mirror — SPR (exact GP / Student-t process regression), MultiSPR (the same for C outputs that share
one kernel matrix: exact multi-class classification on one-hot targets) and SVSP (the sparse variational scale-mixture
classifier): evaluation (test_acc_nll / evaluate) and the training loss with its analytic gradient (loss_and_grad) with
respect to every trainable -- the inducing images through a reverse-mode pass of the conv kernel seeded with d loss / d K
(inducing_grad=True).  The exact models also draw joint function samples from their posterior (sample_posterior).  SVSP.loss itself (a value for an autodiff framework to differentiate) still raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DeviceArray, as_device
from ..nt_kernels import CnnKernelFn, KernelFn
from .base import ConstraintTrainVar, Module, TrainVar
from .bijectors import positive
from .likelihoods import _norm_logpdf, _t_logpdf
from .priors import split_key
from .utils import jitter

__all__ = ["SPR", "LowRankSPR", "IterativeSPR", "MultiSPR", "SVSP", "grad_route", "multi_grad_route", "lml_value_and_grads"]


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
    dense ResNet) or "smn_spr_cnn_loss_grad" (get_cnn_kernel).  Anything else, the conv ResNet and get_cnn_pool_kernel included, has no analytic
    gradient: NotImplementedError, which train.build_train_step(method="auto") answers with central differences."""
    if hasattr(likelihood, "lml_params"):
        if isinstance(kernel_fn, KernelFn):
            return "smn_spr_loss_grad"
        if isinstance(kernel_fn, CnnKernelFn) and kernel_fn.entry == "smn_kernel_cnn":
            return "smn_spr_cnn_loss_grad"
    raise NotImplementedError("analytic gradients need an MLP / dense-ResNet KernelFn or a get_cnn_kernel CnnKernelFn and "
                              "a Gaussian or Student-t likelihood; use train.value_and_grad_fd")


def _seen(kernel_fn, x):
    """x as the fused entries must be handed it: multiplied by the kernel function's input scales (KernelFn.scaled), or x
    itself when there are none."""
    if getattr(kernel_fn, "input_scales", None) is None:
        return x
    return kernel_fn.scaled(x, x.ctx)


def _check_scales_length(kernel, x):
    """ValueError when a kernel's input scales do not have one entry per input feature of x [N, d]."""
    s = kernel.get_input_scales() if hasattr(kernel, "get_input_scales") else None
    shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    if s is not None and (len(shape) != 2 or s.shape[0] != shape[1]):
        raise ValueError("input_scales has %d entries for inputs of shape %s: one per feature of x [N, d] is needed"
                         % (s.shape[0], shape))


def _scales_key(kernel_fn):
    s = getattr(kernel_fn, "input_scales", None)
    return None if s is None else tuple(float(v) for v in s)


def _raw_grads(model, d_con, divisor=1.0):
    """{variable name: d / d RAW value} from d_con = {key: (variable, d / d constrained value)}: the chain rule through each
    variable's constraint, over `divisor` (-N turns a log-pdf into the exact models' loss)."""
    names = {id(v): k for k, v in model.vars().items()}
    return {names[id(var)]: float(g / divisor * var.constraint.grad(var.value)) for var, g in d_con.values()}


class _LooMixin:
    """Leave-one-out cross-validation (Rasmussen & Williams 5.4.2) for the exact models: how would the model have predicted
    training point i had it not seen it?  Closed forms on K~^-1 and A = K~^-1 Y, which every gradient call already leaves on
    the device (csrc/loo.hip); leaving out a point leaves out all its C outputs.  Gaussian likelihood: N(mu_i, 1/p_i I_C);
    Student-t likelihood: a C-variate t with nu + (N-1) C degrees of freedom.  SPR is the C = 1 case of the same entries."""

    def _loo_shape(self):
        return self.num_data, getattr(self, "num_outputs", 1)

    def _loo_head_params(self):
        if not hasattr(self.likelihood, "lml_params"):
            raise NotImplementedError("leave-one-out needs a Gaussian or Student-t likelihood")
        return self.likelihood.lml_params()

    def _loo_value(self, want_pred):
        """(Lambda, mean, scale2, info) through smn_loo_multi: any kernel factory, no gradient."""
        df, scale = self._loo_head_params()
        kernel_fn = self.kernel.get_kernel_fn()
        if not isinstance(kernel_fn, (KernelFn, CnnKernelFn)):
            raise NotImplementedError("leave-one-out is wired for the nt_kernels factories; got %s" % type(kernel_fn).__name__)
        x, ctx = self.x_data, self.x_data.ctx
        n, c = self._loo_shape()
        # the matrix of the kernel function's covariance mode (KernelFn under NTKKernel: Theta); the conv kernels have K only
        k = kernel_fn.cov_matrix(x, None, fill="lower") if isinstance(kernel_fn, KernelFn) else kernel_fn(x, None, get="nngp", fill="lower")
        mean = ctx.empty((n, c), x.dtype) if want_pred else None
        scale2 = ctx.empty((n,), x.dtype) if want_pred else None
        lam, info = C.c_double(), C.c_int()
        ctx.call("smn_loo_multi", x.dcode, k.ptr, n, n, self.y_data.ptr, c, self.eps.safe_value, df, scale, C.byref(lam),
                 mean.ptr if want_pred else None, scale2.ptr if want_pred else None, None, None, C.byref(info), None, 0)
        return lam.value, mean, scale2, info.value

    def loo_loss(self):
        """-Lambda / N with Lambda = sum_i log p(Y_i | Y_-i): the leave-one-out predictive log-probability of the training
        set, same divisor as loss().  Works for every kernel factory."""
        lam, _, _, info = self._loo_value(False)
        return float("nan") if info else -lam / self.num_data

    def loo_predict(self):
        """(mean, scale2 [N], df') of the leave-one-out predictive of every training point in normalised units: mean [N]
        (SPR) or [N,C] (MultiSPR); Gaussian: variance scale2 and df' = None; Student-t: shape scale2 (shared by the C outputs)
        and df' = 2a + (N-1) C degrees of freedom."""
        df, _ = self._loo_head_params()
        _, mean, scale2, _ = self._loo_value(True)
        n, c = self._loo_shape()
        m = np.asarray(mean.raw_numpy(), dtype=np.float64)
        if not hasattr(self, "num_outputs"):
            m = m.reshape(-1)
        return m, np.asarray(scale2.raw_numpy(), dtype=np.float64), (df + (n - 1) * c if df > 0.0 else None)

    def loo_loss_and_grad(self):
        """(loo_loss, {variable name: d loo_loss / d RAW value}) with the names, the softplus chain rule and the NaN-on-non-PD
        convention of loss_and_grad.  One factorisation with identity, the leave-one-out head with its seed G
        (d Lambda = sum_ij G_ij dK~_ij; one N^3 product on the MFMA tile engine) and the tangent pass of loss_and_grad over G
        (smn_spr_loo_grad / smn_spr_cnn_loo_grad).  Follows grad_route: the conv ResNet, a likelihood without lml_params and
        images above 1024 pixels raise NotImplementedError."""
        kernel_fn = self.kernel.get_kernel_fn()
        grad_route(kernel_fn, self.likelihood)   # what has no analytic gradient raises before anything else
        if getattr(kernel_fn, "input_scales", None) is not None:
            raise NotImplementedError("loo_loss_and_grad under input scales is not implemented (loss_and_grad is; loo_loss and "
                                      "loo_predict work)")
        n, c = self._loo_shape()
        lam, info = C.c_double(), C.c_int()
        terms, dhead = (C.c_double * 4)(), (C.c_double * 2)()
        df, _ = self._call_grad_entry("loo_grad", c, (C.byref(lam), dhead, C.byref(info), terms, None, None))
        if info.value != 0:
            return self._nan_grads()
        dlam = dict(zip(("w_std", "b_std", "last_w_std", "eps"), terms))   # d Lambda / d constrained value
        if df > 0.0:
            a_, b_ = self.likelihood.a.safe_value, self.likelihood.b.safe_value
            dlam["a"] = 2.0 * dhead[0] - dhead[1] * b_ / (a_ * a_)      # df = 2a, scale = b/a
            dlam["b"] = dhead[1] / a_
        return -lam.value / n, self._raw_grads(dlam, -n)


class _DrawsMixin:
    """Joint function draws from the posterior of the exact models: the predictive law of all T test points and C outputs
    together, where test_nll only ever reads its per-point marginals.  Gaussian likelihood: vec(f) ~ N(mean, I_C x cov).
    Student-t likelihood: a multivariate t with df_post = 2a + N C degrees of freedom and shape matrix
    shape (I_C x cov), shape = (2a + quad) / df_post * b/a -- a Gaussian draw times ONE sqrt(shape df_post / chi2(df_post))
    per draw, shared by all its points and outputs (csrc/draws.hip)."""

    def predict(self, x):
        """(mean [T,C], cov [T,T]) of the kernel's predict (NNGPKernel / NTKKernel, relative ridge eps) as device arrays in normalised units: one
        covariance shared by the outputs (C = 1 for SPR)."""
        return self.kernel.predict(self.kernel.get_kernel_fn(), self.x_data, self.y_data, x, eps=self.eps.safe_value)

    def _draws_quad(self, kernel_fn, scale):
        return self._student_quad_f64(kernel_fn, scale)

    def posterior(self, capacity=2048, reserve=None):
        """Fit once, predict many: a FittedPosterior (posterior.py) of this model at its current hyper-parameters -- the
        factor of K~ = K_dd + eps tr(K_dd)/N I stays on the device and predict / test_nll / sample / classify on it cost
        O(N^2 T) per call, for test sets of any size (chunks of `capacity` points; a full covariance needs T <= capacity).
        A snapshot: later changes to the model's variables do not reach it.  The model's own methods are unaffected.
        The state can grow: `post.append(x, y)` adds observations at O(N^2 k) under the ridge frozen at this moment
        (`post.ridge`; FittedPosterior.append), and `reserve` = the number of training points to make room for up front."""
        from ..posterior import FittedPosterior
        return FittedPosterior.from_model(self, capacity=capacity, reserve=reserve)

    def predictive_params(self):
        """(df_post, shape) of the predictive law in normalised units.  Gaussian likelihood: (None, 1.0), no device work.
        Student-t: df_post = 2a + N C and shape = (2a + quad) / df_post * b/a with quad = y^T ((b/a) K + 1e-6 I)^-1 y, the
        fp64 number test_nll uses: the marginal of a draw at point t is test_nll's Student-t with sigma_t = sqrt(shape cov_tt)."""
        if not hasattr(self.likelihood, "lml_params"):
            raise NotImplementedError("predictive_params needs a Gaussian or Student-t likelihood")
        df, scale = self.likelihood.lml_params()
        if not df > 0.0:
            return None, 1.0
        n, c = self._loo_shape()
        df_post = df + n * c
        quad = self._draws_quad(self.kernel.get_kernel_fn(), scale)
        return df_post, (df + quad) / df_post * scale

    def sample_posterior(self, key, x, num_samples, *, jitter=1e-6):
        """num_samples joint draws of the latent function at x: a device array [S,T] (SPR) or [S,T,C] (MultiSPR) in the
        model's dtype and in NORMALISED units, like predict (test_nll de-normalises as f * y_std + y_mean; do the same to a
        draw to compare it with targets).  predict, then smn_cholesky of the covariance in place with the relative ridge
        `jitter` (cov + jitter tr(cov)/T I), then smn_mvn_draws: the draw of (seed, point, output, draw index) is a pure
        function of those, so `key` is an int seed or (seed, global index of the first point of x), as in SVSP.  A
        covariance that does not factor, or a Student-t shape that is not a positive finite number (the fp64 quadratic form
        of predictive_params failed), gives an all-NaN array (the package's convention for a failed Cholesky); neither
        raises.  1e-6 is the package's default ridge; an fp32 model will usually need more (a posterior covariance is
        ill-conditioned by nature: 1e-3 is a reasonable start), which is the caller's call.  Works for every nt_kernels
        factory, since it needs predict only."""
        seed, point0 = split_key(key)
        s = int(num_samples)
        if s < 1:
            raise ValueError("num_samples must be at least 1")
        df_post, shape = self.predictive_params()
        mean, cov = self.predict(x)
        ctx = mean.ctx
        mean, cov = as_device(mean, ctx), as_device(cov, ctx)     # plain buffers: a lazy scale * A + shift * I is materialised
        t, c = mean.shape
        out_shape = (s, t, c) if hasattr(self, "num_outputs") else (s, t)
        nan = lambda: ctx.to_device(np.full(out_shape, np.nan, dtype=mean.dtype))
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


class _ExactGP(_DrawsMixin, _LooMixin, Module):
    """What SPR and MultiSPR share around the fused gradient entries (csrc/grad.hip, cnn_grad.hip, loo.hip): which entry a
    kernel function takes, its argument list, the errors it translates, and the host chain rule behind it."""

    _multi = False                                            # MultiSPR: the *_multi entries, whatever its C

    def _f64_data(self):
        if self.x_data.dtype == np.float64:
            return self.x_data, self.y_data
        if getattr(self, "_x64", None) is None:
            ctx = self.x_data.ctx
            self._x64 = ctx.to_device(self.x_data.numpy().astype(np.float64))
            self._y64 = ctx.to_device(self.y_host)
        return self._x64, self._y64

    def _f64_seen(self, kernel_fn, x64):
        """The fp64 copy of the training inputs as the kernel sees them.  Under input scales this is the upcast of the inputs
        scaled in the STORAGE dtype (what every other route is handed), not x64 scaled in fp64: the model stays the model of
        x * s.astype(dtype)."""
        if getattr(kernel_fn, "input_scales", None) is None:
            return x64
        xs = _seen(kernel_fn, self.x_data)
        return xs if xs.dtype == np.float64 else xs.ctx.to_device(xs.numpy().astype(np.float64))

    def _call_grad_entry(self, kind, c, outs):
        """One fused entry on the training data, "smn_spr_" + kind (MLP / dense ResNet) or "smn_spr_cnn_" + kind
        (get_cnn_kernel) as grad_route decides: (x, y, [c unless None,] eps, df, scale, *outs).  Returns (df, scale)."""
        kernel_fn = self.kernel.get_kernel_fn()
        mlp = grad_route(kernel_fn, self.likelihood) == "smn_spr_loss_grad"
        eps = self.eps.safe_value
        df, scale = self.likelihood.lml_params()
        x, ctx = self.x_data, self.x_data.ctx
        if mlp:
            name, data = "smn_spr_" + kind, (x.ptr, self.num_data, x.shape[1], x.shape[1])
        else:
            if len(x.shape) != 4:
                raise ValueError("conv kernel expects x of shape [N,H,W,C]")
            name, data = "smn_spr_cnn_" + kind, (x.ptr, self.num_data, x.shape[1], x.shape[2], x.shape[3])
        args = (x.dcode, *kernel_fn.params, *data, self.y_data.ptr) + (() if c is None else (c,)) + (eps, df, scale) + outs
        try:
            ctx.call(name, *args)
        except _lib.SmnError as e:
            if not mlp and e.code == _lib.ENOTSUP and (c or 1) <= 48:   # images above the tangent kernel's limit
                raise NotImplementedError(str(e)) from e
            raise
        return df, scale

    def _nan_grads(self):
        """(loss, gradients) when the kernel matrix is not positive definite."""
        nan = float("nan")
        return nan, {k: nan for k in self.vars()}

    def _raw_grads(self, d_con, divisor):
        """_raw_grads for d_con = {"w_std" | "b_std" | "last_w_std" | "eps" | "a" | "b": d / d constrained value}."""
        owners = {"w_std": self.kernel.w_std, "b_std": self.kernel.b_std, "last_w_std": self.kernel.last_w_std,
                  "eps": self.eps}
        if "a" in d_con:
            owners.update(a=self.likelihood.a, b=self.likelihood.b)
        return _raw_grads(self, {key: (owners[key], g) for key, g in d_con.items()}, divisor)

    def _inputs_entry(self, want_gx, want_feat):
        """smn_spr_loss_grad_inputs on the training inputs as the kernel sees them: (kernel_fn, x~, quad, logdet, info, terms,
        gx [N, d] device array = d log p / d x~ or None, feat [d] = sum_n gx o x~ or None, df, scale)."""
        kernel_fn = self.kernel.get_kernel_fn()
        if grad_route(kernel_fn, self.likelihood) != "smn_spr_loss_grad":
            raise NotImplementedError("gradients in the inputs need an MLP / dense-ResNet KernelFn")
        n, c = self._loo_shape()
        x = _seen(kernel_fn, self.x_data)
        ctx, d = x.ctx, x.shape[1]
        df, scale = self.likelihood.lml_params()
        quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
        terms = (C.c_double * 4)()
        gx = ctx.empty((n, d), x.dtype) if want_gx else None
        feat = np.zeros(d) if want_feat else None
        ctx.call("smn_spr_loss_grad_inputs", x.dcode, *kernel_fn.params, x.ptr, n, d, d, self.y_data.ptr, c, self.eps.safe_value,
                 df, scale, C.byref(quad), None, C.byref(logdet), C.byref(info), terms, gx.ptr if want_gx else None, d,
                 feat.ctypes.data_as(C.POINTER(C.c_double)) if want_feat else None)
        return kernel_fn, x, quad.value, logdet.value, info.value, terms, gx, feat, df, scale

    def _lml_loss_and_grad_scaled(self):
        """loss_and_grad under input scales: the scalar entries as without them (on s o x), plus `input_scales`, a length-d
        array of d loss / d RAW value: d log p / d s_j = feat_j / s_j (csrc/input_grad_sym.hip), over -N, through the
        constraint."""
        n, c = self._loo_shape()
        kernel_fn, _, quad, logdet, info, terms, _, feat, df, scale = self._inputs_entry(False, True)
        var = self.kernel.input_scales
        name = {id(v): k for k, v in self.vars().items()}[id(var)]
        if info != 0:
            loss, grads = self._nan_grads()
            grads[name] = np.full(var.value.shape, np.nan)
            return loss, grads
        student = df > 0.0
        lp, dlp = lml_value_and_grads(terms, quad, c * logdet, n * c, df, scale,
                                      self.likelihood.a.safe_value if student else None,
                                      self.likelihood.b.safe_value if student else None)
        grads = self._raw_grads(dlp, -n)
        grads[name] = (feat / kernel_fn.input_scales) / -n * var.constraint.grad(var.value)
        return -lp / n, grads

    def loss_input_grad(self):
        """(loss, d loss / d x): the gradient of loss() in the training inputs as an [N, d] device array, per unit of the inputs
        as handed in (under input scales: s o the gradient in the scaled inputs) -- learned or inducing inputs, dataset
        distillation.  One smn_spr_loss_grad_inputs call: loss_and_grad's pipeline followed by the two-sided tangent pass and
        one N^2 d product on the tile engine (csrc/input_grad_sym.hip).  MLP / dense-ResNet kernels, Gaussian or Student-t
        likelihood; a matrix that is not positive definite gives NaN for both."""
        n, c = self._loo_shape()
        kernel_fn, x, quad, logdet, info, terms, gx, _, df, scale = self._inputs_entry(True, False)
        ctx, d = x.ctx, x.shape[1]
        if info != 0:
            return float("nan"), ctx.to_device(np.full((n, d), np.nan, dtype=x.dtype))
        student = df > 0.0
        lp, _ = lml_value_and_grads(terms, quad, c * logdet, n * c, df, scale,
                                    self.likelihood.a.safe_value if student else None,
                                    self.likelihood.b.safe_value if student else None)
        s = kernel_fn.input_scales
        fac = np.ascontiguousarray((np.ones(d) if s is None else s) / -n, dtype=np.float64)   # loss = -log p / N
        ctx.call("smn_scale_columns", gx.dcode, gx.ptr, n, d, d, fac.ctypes.data_as(C.POINTER(C.c_double)), gx.ptr, d)
        return -lp / n, gx

    def _lml_loss_and_grad(self):
        """loss_and_grad of both models: the head in dimension N C with log-determinant C logdet K~."""
        if getattr(self.kernel, "input_scales", None) is not None:
            return self._lml_loss_and_grad_scaled()
        n, c = self._loo_shape()
        quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
        terms = (C.c_double * 4)()
        if self._multi:
            outs = (C.byref(quad), None, C.byref(logdet), C.byref(info), terms)
            df, scale = self._call_grad_entry("loss_grad_multi", c, outs)
        else:
            df, scale = self._call_grad_entry("loss_grad", None, (C.byref(quad), C.byref(logdet), C.byref(info), terms))
        if info.value != 0:
            return self._nan_grads()
        student = df > 0.0
        lp, dlp = lml_value_and_grads(terms, quad.value, c * logdet.value, n * c, df, scale,
                                      self.likelihood.a.safe_value if student else None,
                                      self.likelihood.b.safe_value if student else None)
        return -lp / n, self._raw_grads(dlp, -n)


class SPR(_ExactGP):
    def __init__(self, kernel, likelihood, x_data, y_data, y_mean, y_std, *, eps: float = 1e-6):
        super().__init__()
        _check_scales_length(kernel, x_data)         # (before anything touches a device)
        self.kernel = kernel
        self.likelihood = likelihood
        self.x_data = as_device(x_data)              # resident in HBM for the life of the model
        self.y_host = np.asarray(y_data, dtype=np.float64).reshape(-1)
        self.y_data = as_device(self.y_host, self.x_data.ctx, dtype=self.x_data.dtype)
        self.y_mean = float(np.asarray(y_mean))
        self.y_std = float(np.asarray(y_std))
        self.num_data = self.x_data.shape[0]
        self.eps = ConstraintTrainVar(eps, constraint=positive())

    def _student_quad_f64(self, kernel_fn, scale):
        """y^T (K + (1e-6 / scale) I)^-1 y / scale  =  y^T (scale K + 1e-6 I)^-1 y in fp64 (likelihoods.py:60-61).
        It depends on the training data and the hyper-parameters only -- not on the test points -- and the reference's
        evaluation loop calls test_nll twice per check point, on the validation and on the test split
        (experiments/regression/train.py:203-212, test.py:89-99): the value of the last parameter setting is kept, so the
        second call costs the fp32 posterior alone.  (Measured at N = 16384: this fp64 build + factorisation is 44 ms
        against 29 ms for the posterior, and running the two concurrently on two contexts buys 3 % -- both are bound by the
        matrix pipes, not by latency; profiles/r04_two_context_probe.txt.)"""
        key = (tuple(kernel_fn.params), float(scale), _scales_key(kernel_fn))
        hit = getattr(self, "_quad64_cache", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        xd, yd = self._f64_data()
        xd = self._f64_seen(kernel_fn, xd)
        net, act, L, w, b, lw = kernel_fn.params
        quad, info = C.c_double(), C.c_int()
        xd.ctx.call("smn_spr_loss", xd.dcode, net, act, L, w, b, lw, xd.ptr, xd.shape[0], xd.shape[1],
                    xd.shape[1], yd.ptr, 1e-6 / scale, 0.0, 1.0, None, C.byref(quad), None, C.byref(info))
        val = float("nan") if info.value else quad.value / scale
        self._quad64_cache = (key, val)
        return val

    def _draws_quad(self, kernel_fn, scale):
        """The quadratic form of test_nll's Student-t head, by test_nll's own two routes."""
        if isinstance(kernel_fn, KernelFn):
            return self._student_quad_f64(kernel_fn, scale)
        from .utils import factor_stats
        cov_data = self.kernel.K(kernel_fn, self._f64_data()[0])
        return factor_stats(self.y_host, scale * cov_data + jitter(self.num_data))[0]

    # ---- spax/models.py:93-98
    def loss(self):
        eps = self.eps.safe_value
        kernel_fn = self.kernel.get_kernel_fn()
        if isinstance(kernel_fn, KernelFn) and hasattr(self.likelihood, "lml_params"):
            # fused: build K(X,X)+eps I in the factorisation workspace, factor, carry y through
            df, scale = self.likelihood.lml_params()
            x, ctx = _seen(kernel_fn, self.x_data), self.x_data.ctx
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
        the conv ResNet, a likelihood without lml_params, larger images -- raises NotImplementedError.
        A kernel with input scales (NNGPKernel(..., input_scales=...)) adds the entry `input_scales`, a length-d array, from one
        smn_spr_loss_grad_inputs call on the scaled inputs (csrc/input_grad_sym.hip); the scalar entries are computed as without
        scales."""
        return self._lml_loss_and_grad()

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


class LowRankSPR(Module):
    """SPR on a rank-M approximation of the kernel matrix: K(X, X) ~ L L^T from the greedy pivoted Cholesky
    (lowrank.pivoted_cholesky), never the N x N matrix.  The model covariance is

        K^ = L L^T + diag(resid)   correction="fitc": the FITC approximation on the M greedy inducing points
        K^ = L L^T                 correction="none": SoR / DTC

    and the log-marginal likelihood and the predictions of K^ + lam I come from the Woodbury identity on the device
    (lowrank.woodbury_fit, csrc/lowrank.hip): O(N M^2) work, O(N M) memory, the M x M side in fp64.  Same trainables and names
    as SPR (kernel.w_std / b_std / last_w_std, eps, the likelihood's a / b), so train.build_train_step(method="auto") trains it
    by central differences and checkpoints carry over.

    loss()        lam = eps, absolute, and SPR.loss's Gaussian / multivariate-t heads, over N.
    predict(x)    (mean [T, 1], var [T]) of the latent function in normalised units under lam = eps trace(K) / N, the relative
                  ridge of SPR.predict; the test set streams through in chunks, nothing of size N x N or T x T is formed.
    test_nll      SPR.test_nll's per-point heads on those marginals.  DEVIATION for the Student-t head: its quadratic form is
                  the one of that same fit, y^T (scale (K^ + lam I))^-1 y = quad / scale.  The reference (and SPR) take it from
                  a separate matrix scale K + 1e-6 I; under a rank-M K^ that matrix divides the part of y outside the span of
                  L by 1e-6, which is an artefact of the approximation and not a statement about the data.

    rank: columns asked for (1 <= rank <= N, at most 4096); tol: stop early when the residual trace falls to tol trace(K).
    Every kernel function pivoted_cholesky accepts works.  The factor is kept while the hyper-parameters do not change.
    An fp32 model under "fitc" loses digits in loss() as eps shrinks (pivot rows weigh 1 / eps: 1.3e-6 relative at
    eps >= 1e-2, 6.5e-5 at 1e-4, 2.8e-2 at 1e-6): use fp64 data or correction="none" there.  The leave-one-out entries,
    posterior(), sample_posterior and input scales are not implemented.

    Frozen pivots.  By default every call selects its pivots greedily at the current hyper-parameters, so loss() is only piecewise
    smooth in them and has no gradient.  freeze_pivots() keeps the inducing set -- the greedy choice at the current values, or
    an array of indices -- until refresh_pivots() re-selects it or unfreeze_pivots() goes back to greedy: loss, predict and
    test_nll then build the factor at those pivots (lowrank.pivoted_cholesky(pivots=...)), loss() is smooth, and
    loss_and_grad() returns it with its analytic gradient in the raw values of w_std, b_std, last_w_std, eps and the Student-t
    head's a and b (lowrank.woodbury_grad, csrc/lowrank_grad.hip; MLP / dense-ResNet kernels with NNGP covariance), which
    train.build_train_step(method="auto" | "analytic") then uses.  The gradient is that of the frozen objective: the selection
    itself is not differentiated.  The fp32 limit of loss() under "fitc" at small eps holds for the gradient too."""

    _frozen_pivots = None                            # class-level default: not frozen (objects made by __new__ included)

    def __init__(self, kernel, likelihood, x_data, y_data, y_mean, y_std, *, rank, correction="fitc", eps: float = 1e-6,
                 tol: float = 0.0):
        super().__init__()
        from .. import lowrank                       # (lowrank imports nothing from spax: no cycle, but keep start-up light)
        shape = tuple(x_data.shape) if hasattr(x_data, "shape") else np.shape(x_data)
        if len(shape) < 2 or shape[0] < 1:
            raise ValueError("x_data must be [N, ...] with N >= 1, got shape %s" % (shape,))
        if isinstance(rank, bool) or int(rank) != rank:
            raise ValueError("rank must be an integer, got %r" % (rank,))
        if not 1 <= int(rank) <= min(shape[0], _lib.LOWRANK_MAX_RANK):
            raise ValueError("rank must lie in [1, min(N = %d, %d)], got %d" % (shape[0], _lib.LOWRANK_MAX_RANK, rank))
        if correction not in ("fitc", "none"):
            raise ValueError("correction must be 'fitc' or 'none', got %r" % (correction,))
        if not float(tol) >= 0.0:
            raise ValueError("tol must be >= 0, got %r" % (tol,))
        if getattr(kernel, "input_scales", None) is not None:
            raise NotImplementedError("LowRankSPR does not support input scales")
        if not hasattr(likelihood, "lml_params"):
            raise NotImplementedError("LowRankSPR needs a Gaussian or Student-t likelihood")
        y = np.asarray(y_data, dtype=np.float64).reshape(-1)
        if y.shape[0] != shape[0]:
            raise ValueError("y_data has %d entries for N = %d inputs" % (y.shape[0], shape[0]))
        self._lowrank = lowrank
        self.kernel, self.likelihood = kernel, likelihood
        self.rank, self.correction, self.tol = int(rank), correction, float(tol)
        self.x_data = as_device(x_data)
        self.y_host = y
        self.y_mean, self.y_std = float(np.asarray(y_mean)), float(np.asarray(y_std))
        self.num_data = self.x_data.shape[0]
        self.eps = ConstraintTrainVar(eps, constraint=positive())
        self._factor_cache = None                    # (key, PivotedCholesky, {lam: WoodburyFit})

    # ---- what is not there, refused before any device call
    def _missing(self, what):
        raise NotImplementedError("LowRankSPR has no %s: the exact models (SPR) do" % what)

    # ---- frozen pivots
    @property
    def pivots(self):
        """The frozen pivots (np.int64, a copy) or None."""
        p = self._frozen_pivots
        return None if p is None else p.copy()

    def freeze_pivots(self, pivots=None):
        """Keep the inducing set: the greedy selection at the current hyper-parameters (None), or the given distinct indices.
        Right after freeze_pivots() loss, predict and test_nll return the bits they returned before it.  Returns self."""
        if pivots is None:
            self._frozen_pivots = None
            pivots = self._factor()[1].pivots
        else:
            pivots = self._lowrank._check_pivots(pivots, self.num_data)
            if pivots.shape[0] > min(self.num_data, _lib.LOWRANK_MAX_RANK):
                raise ValueError("at most %d pivots, got %d" % (min(self.num_data, _lib.LOWRANK_MAX_RANK), pivots.shape[0]))
        self._frozen_pivots = np.array(pivots, dtype=np.int64)
        return self

    def refresh_pivots(self):
        """Re-select the frozen pivots greedily at the current hyper-parameters.  Returns self."""
        return self.freeze_pivots(None)

    def unfreeze_pivots(self):
        """Back to a greedy selection on every call.  Returns self."""
        self._frozen_pivots = None
        return self

    def loss_and_grad(self):
        """(loss, {variable name: d loss / d RAW value}) of the FROZEN model, as SPR.loss_and_grad returns them: the loss is
        loss()'s value (same bits); the gradient holds the pivots fixed.  NotImplementedError while the pivots are not frozen
        (the greedy objective has no gradient) and for kernel functions outside the MLP / dense-ResNet NNGP family."""
        if self._frozen_pivots is None:
            self._missing("analytic gradient while the pivots are not frozen: call freeze_pivots() first "
                          "(train.build_train_step(method='auto') falls back to central differences)")
        kernel_fn = self.kernel.get_kernel_fn()
        if not (isinstance(kernel_fn, KernelFn) and kernel_fn.cov == "nngp"):
            raise NotImplementedError("LowRankSPR.loss_and_grad needs an MLP / dense-ResNet KernelFn with NNGP covariance; "
                                      "use train.value_and_grad_fd")
        _, _, fit = self._fit(False)
        if fit.info != 0:
            nan = float("nan")
            return nan, {k: nan for k in self.vars()}
        n = self.num_data
        df, scale = self.likelihood.lml_params()
        student = df > 0.0
        quad = float(fit.quad[0])
        coef = (df + n) / ((df + quad / scale) * scale) if student else 1.0
        terms = self._lowrank.woodbury_grad(fit, kernel_fn, self.x_data, coef)
        lp, dlp = lml_value_and_grads(terms, quad, fit.logdet, n, df, scale,
                                      self.likelihood.a.safe_value if student else None,
                                      self.likelihood.b.safe_value if student else None)
        owners = {"w_std": self.kernel.w_std, "b_std": self.kernel.b_std, "last_w_std": self.kernel.last_w_std, "eps": self.eps}
        if student:
            owners.update(a=self.likelihood.a, b=self.likelihood.b)
        return -lp / n, _raw_grads(self, {key: (owners[key], g) for key, g in dlp.items()}, -n)

    def loo_loss(self):
        self._missing("leave-one-out objective")

    def loo_predict(self):
        self._missing("leave-one-out predictions")

    def loo_loss_and_grad(self):
        self._missing("leave-one-out gradient")

    def posterior(self, *args, **kwargs):
        self._missing("fitted posterior")

    def sample_posterior(self, *args, **kwargs):
        self._missing("joint posterior draws")

    # ---- the factor and the fits on it, kept by hyper-parameter content
    def _factor(self):
        kernel_fn = self.kernel.get_kernel_fn()
        params = getattr(kernel_fn, "params", None)
        frozen = self._frozen_pivots
        key = None if params is None else (type(kernel_fn).__name__, getattr(kernel_fn, "entry", None),
                                           getattr(kernel_fn, "cov", None), tuple(params),
                                           None if frozen is None else frozen.tobytes())
        hit = self._factor_cache
        if hit is not None and key is not None and frozen is not None and hit[0] == key[:4] + (None,) \
                and np.array_equal(hit[1].pivots, frozen):
            hit = self._factor_cache = (key, hit[1], hit[2])   # the greedy factor these pivots came from: the same bits, kept
        if hit is None or key is None or hit[0] != key:
            if frozen is None:
                res = self._lowrank.pivoted_cholesky(kernel_fn, self.x_data, self.rank, tol=self.tol)
            else:
                res = self._lowrank.pivoted_cholesky(kernel_fn, self.x_data, tol=self.tol, pivots=frozen)
            hit = self._factor_cache = (key, res, {})
        return kernel_fn, hit[1], hit[2]

    def _fit(self, relative):
        """The WoodburyFit under lam = eps (loss) or eps trace(K) / N (predict, test_nll)."""
        kernel_fn, res, fits = self._factor()
        eps = self.eps.safe_value
        lam = eps * float(res.trace[0]) / self.num_data if relative else eps
        if lam not in fits:
            fits.clear() if len(fits) > 4 else None
            fits[lam] = self._lowrank.woodbury_fit(res, self.y_host, lam, self.correction == "fitc")
        return kernel_fn, res, fits[lam]

    def loss(self):
        _, _, fit = self._fit(False)
        if fit.info != 0:
            return float("nan")
        df, scale = self.likelihood.lml_params()
        student = df > 0.0
        lp, _ = lml_value_and_grads((0.0,) * 4, float(fit.quad[0]), fit.logdet, self.num_data, df, scale,
                                    self.likelihood.a.safe_value if student else None,
                                    self.likelihood.b.safe_value if student else None)
        return -lp / self.num_data

    def _predict(self, x, chunk):
        kernel_fn, res, fit = self._fit(True)
        ctx, dt = self.x_data.ctx, self.x_data.dtype
        xt = np.asarray(x.numpy() if isinstance(x, DeviceArray) else x)
        if xt.shape[1:] != tuple(self.x_data.shape[1:]):
            raise ValueError("x has shape %s, the training inputs %s" % (xt.shape, tuple(self.x_data.shape)))
        t = xt.shape[0]
        mean, var = np.full((t, 1), np.nan, dtype=dt), np.full(t, np.nan, dtype=dt)
        if fit.info != 0 or t == 0:
            return fit, mean, var
        if getattr(res, "_z", None) is None:         # the inducing inputs Z = x[pivots]: rank rows, gathered once per factor
            res._z = ctx.to_device(np.ascontiguousarray(self.x_data.numpy()[res.pivots]))
        for a in range(0, t, chunk):
            xc = ctx.to_device(np.ascontiguousarray(xt[a:a + chunk], dtype=dt))
            kzt = self._lowrank.kernel_cross(kernel_fn, res._z, xc)
            ktt = self._lowrank.kernel_diag(kernel_fn, xc)
            m, v = fit.readout(kzt, ktt)
            mean[a:a + chunk], var[a:a + chunk] = m.raw_numpy(), v.raw_numpy()
        return fit, mean, var

    def predict(self, x, cov="diag", chunk=2048):
        """(mean [T, 1], var [T]) as host arrays in the model's dtype and in normalised units: the DTC / FITC predictive of the
        latent function at x, `chunk` test points at a time (a point's bits do not depend on the chunking).  Only the
        diagonal exists: a T x T covariance would defeat the purpose.  NaN when I + L^T W L does not factor."""
        if cov != "diag":
            raise NotImplementedError("LowRankSPR.predict has cov='diag' only")
        if int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        _, mean, var = self._predict(x, int(chunk))
        return mean, var

    def test_nll(self, x, y, chunk=2048):
        fit, mean, var = self._predict(x, int(chunk))
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        mu = mean.astype(np.float64).reshape(-1) * self.y_std + self.y_mean
        v = var.astype(np.float64) * self.y_std ** 2
        df, scale = self.likelihood.lml_params()
        if df > 0.0:                                  # likelihoods.py:52-65 with the quadratic form of this fit (class docstring)
            cond_df = df + self.num_data
            sigma = np.sqrt((df + float(fit.quad[0]) / scale) / cond_df * scale * v)
            log_prob = _t_logpdf(y * self.y_std + self.y_mean, cond_df, mu, sigma)
        else:
            log_prob = _norm_logpdf(y * self.y_std + self.y_mean, mu, np.sqrt(v))
        return -np.mean(log_prob)


class IterativeSPR(Module):
    """SPR without the N x N matrix: the exact posterior of K(X, X) + lam I by preconditioned conjugate gradients, with K applied
    matrix-free (lowrank.kernel_matmul / lowrank.pcg_solve, csrc/kernel_matmul.hip and csrc/pcg.hip).  Memory is O(N (d + rank));
    every solve costs (iterations) x (one build of the N x N rectangle) on the MFMA.  Same trainables and names as SPR
    (NNGPKernel or NTKKernel over get_mlp_kernel / get_dense_resnet_kernel, eps, the likelihood's a / b), so the values of an SPR
    or a LowRankSPR -- trained where training is cheap -- carry over: IterativeSPR.from_model(model).

    fit()         solves K~ alpha = y in normalised units under lam = eps trace(K) / N, the relative ridge of SPR.predict (the
                  trace from lowrank.kernel_diag), preconditioned by M = L L^T + lam I with L = lowrank.pivoted_cholesky(kernel_fn,
                  x, rank) (the fused route where it exists; rank=0: unpreconditioned).  alpha, the factor and the PcgResult
                  (model.solve_info) are kept while the hyper-parameters do not change.
    predict(x)    (mean [T, 1], var [T] or None) in normalised units as host fp64 arrays.  mean = K(x*, X) alpha by the cross form
                  of kernel_matmul, `chunk` points at a time; K(x*, X) is never stored.  var=True adds var = k** - k*^T K~^-1 k* by
                  block solves: ONE PCG PER BLOCK of var_block <= 48 test points (right-hand sides K(X, x*_block)), so T points
                  cost ceil(T / var_block) solves of the size of fit().
    test_nll      SPR.test_nll's per-point heads on those marginals.  DEVIATION for the Student-t head, as LowRankSPR documents
                  and for the same reason: its quadratic form is y^T alpha of this solve, y^T (scale K~)^-1 y = quad / scale.
    A solve that ends with info != 0 makes predict warn with the residual reached; the values are still returned.
    loss, loss_and_grad, the leave-one-out entries, posterior() and sample_posterior are not implemented: there is no
    log-determinant here (train on LowRankSPR or SPR)."""

    def __init__(self, kernel, likelihood, x_data, y_data, y_mean, y_std, *, rank=256, eps: float = 1e-6, tol: float = 1e-6,
                 max_iter: int = 1000):
        super().__init__()
        from .. import lowrank
        shape = tuple(x_data.shape) if hasattr(x_data, "shape") else np.shape(x_data)
        if len(shape) < 2 or shape[0] < 1:
            raise ValueError("x_data must be [N, ...] with N >= 1, got shape %s" % (shape,))
        if isinstance(rank, bool) or int(rank) != rank:
            raise ValueError("rank must be an integer, got %r" % (rank,))
        if not 0 <= int(rank) <= _lib.LOWRANK_MAX_RANK:
            raise ValueError("rank must lie in [0, %d] (0: no preconditioner), got %d" % (_lib.LOWRANK_MAX_RANK, rank))
        if not 0.0 < float(tol) < 1.0:
            raise ValueError("tol must lie in (0, 1), got %r" % (tol,))
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
            raise ValueError("max_iter must be an integer >= 1, got %r" % (max_iter,))
        if not hasattr(likelihood, "lml_params"):
            raise NotImplementedError("IterativeSPR needs a Gaussian or Student-t likelihood")
        y = np.asarray(y_data, dtype=np.float64).reshape(-1)
        if y.shape[0] != shape[0]:
            raise ValueError("y_data has %d entries for N = %d inputs" % (y.shape[0], shape[0]))
        self._lowrank = lowrank
        self.kernel, self.likelihood = kernel, likelihood
        self.rank, self.tol, self.max_iter = min(int(rank), shape[0]), float(tol), int(max_iter)
        self.x_data = as_device(x_data)
        self.y_host = y
        self.y_mean, self.y_std = float(np.asarray(y_mean)), float(np.asarray(y_std))
        self.num_data = self.x_data.shape[0]
        self.eps = ConstraintTrainVar(eps, constraint=positive())
        self.solve_info = None
        self._fit_cache = None                       # (key, kernel_fn, lam, PivotedCholesky or None, PcgResult, y^T alpha)

    @classmethod
    def from_model(cls, model, **kw):
        """The matrix-free model of an SPR or a LowRankSPR: its kernel and likelihood objects (so the trained values carry
        over), its data and its eps; rank, tol and max_iter from **kw."""
        for name in ("kernel", "likelihood", "x_data", "y_host", "y_mean", "y_std", "eps"):
            if not hasattr(model, name):
                raise TypeError("from_model needs an SPR or a LowRankSPR, got %s" % type(model).__name__)
        kw.setdefault("eps", model.eps.safe_value)
        return cls(model.kernel, model.likelihood, model.x_data, model.y_host, model.y_mean, model.y_std, **kw)

    # ---- what is not there, refused before any device call
    def _missing(self, what):
        raise NotImplementedError("IterativeSPR has no %s: there is no log-determinant here; LowRankSPR (approximate) and SPR "
                                  "(exact, N x N) do" % what)

    def loss(self):
        self._missing("training objective")

    def loss_and_grad(self):
        self._missing("analytic gradient")

    def loo_loss(self):
        self._missing("leave-one-out objective")

    def loo_predict(self):
        self._missing("leave-one-out predictions")

    def loo_loss_and_grad(self):
        self._missing("leave-one-out gradient")

    def posterior(self, *args, **kwargs):
        self._missing("fitted posterior")

    def sample_posterior(self, *args, **kwargs):
        self._missing("joint posterior draws")

    # ---- the solve, kept by hyper-parameter content
    def _kernel_fn(self):
        kernel_fn = self.kernel.get_kernel_fn()
        if not isinstance(kernel_fn, KernelFn):
            raise NotImplementedError("IterativeSPR exists for get_mlp_kernel / get_dense_resnet_kernel (NNGPKernel or NTKKernel), "
                                      "not for %s" % type(kernel_fn).__name__)
        return kernel_fn

    def fit(self):
        """Solve K~ alpha = y (see the class docstring); returns the PcgResult, also kept as model.solve_info."""
        kernel_fn = self._kernel_fn()
        eps = self.eps.safe_value
        key = (kernel_fn.cov, tuple(kernel_fn.params), _scales_key(kernel_fn), eps, self.rank, self.tol, self.max_iter)
        hit = self._fit_cache
        if hit is None or hit[0] != key:
            lr = self._lowrank
            trace = float(np.sum(np.asarray(lr.kernel_diag(kernel_fn, self.x_data).raw_numpy(), dtype=np.float64)))
            lam = eps * trace / self.num_data
            pre = lr.pivoted_cholesky(kernel_fn, self.x_data, self.rank) if self.rank > 0 else None
            sol = lr.pcg_solve(kernel_fn, self.x_data, self.y_host, lam, precond=pre, tol=self.tol, max_iter=self.max_iter)
            quad = float(self.y_host @ sol.x.numpy()[:, 0])
            hit = self._fit_cache = (key, kernel_fn, lam, pre, sol, quad)
        self.solve_info = hit[4]
        return hit[4]

    def _warn(self, sol, what):
        if sol.info != 0:
            import warnings
            warnings.warn("IterativeSPR: %s ended with info = %d after %d iterations (true relative residual %.3e, tol %.1e); the "
                          "values are returned as they are" % (what, sol.info, sol.iters, float(np.nanmax(sol.resid)), self.tol),
                          RuntimeWarning, stacklevel=3)

    def predict(self, x, var=False, chunk=2048, var_block=48):
        """(mean [T, 1], var [T] or None): see the class docstring.  var=True costs one PCG per block of var_block test points."""
        if int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        if not 1 <= int(var_block) <= _lib.PCG_MAX_COLS:
            raise ValueError("var_block must lie in [1, %d], got %r" % (_lib.PCG_MAX_COLS, var_block))
        xt = np.asarray(x.numpy() if isinstance(x, DeviceArray) else x)
        if xt.ndim < 2 or xt.shape[1:] != tuple(self.x_data.shape[1:]):
            raise ValueError("x has shape %s, the training inputs %s" % (xt.shape, tuple(self.x_data.shape)))
        sol = self.fit()
        self._warn(sol, "the solve of fit()")
        _, kernel_fn, lam, pre, _, _ = self._fit_cache
        lr, ctx, dt = self._lowrank, self.x_data.ctx, self.x_data.dtype
        t = xt.shape[0]
        mean = np.zeros((t, 1), dtype=np.float64)
        for a in range(0, t, int(chunk)):
            xc = ctx.to_device(np.ascontiguousarray(xt[a:a + int(chunk)], dtype=dt))
            mean[a:a + int(chunk)] = lr.kernel_matmul(kernel_fn, xc, self.x_data, sol.x).numpy()
        if not var:
            return mean, None
        out = np.zeros(t, dtype=np.float64)
        self.var_info = []
        for a in range(0, t, int(var_block)):
            xb = ctx.to_device(np.ascontiguousarray(xt[a:a + int(var_block)], dtype=dt))
            rhs = np.asarray(lr.kernel_cross(kernel_fn, self.x_data, xb).numpy(), dtype=np.float64)
            ktt = np.asarray(lr.kernel_diag(kernel_fn, xb).raw_numpy(), dtype=np.float64)
            blk = lr.pcg_solve(kernel_fn, self.x_data, rhs, lam, precond=pre, tol=self.tol, max_iter=self.max_iter)
            self._warn(blk, "a variance block solve")
            self.var_info.append(blk)
            out[a:a + int(var_block)] = ktt - np.einsum("ij,ij->j", rhs, blk.x.numpy())
        return mean, out

    def test_nll(self, x, y, chunk=2048, var_block=48):
        mean, var = self.predict(x, var=True, chunk=chunk, var_block=var_block)
        quad = self._fit_cache[5]
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        mu = mean.reshape(-1) * self.y_std + self.y_mean
        v = var * self.y_std ** 2
        df, scale = self.likelihood.lml_params()
        if df > 0.0:                                  # likelihoods.py:52-65 with the quadratic form of this solve (class docstring)
            cond_df = df + self.num_data
            sigma = np.sqrt((df + quad / scale) / cond_df * scale * v)
            log_prob = _t_logpdf(y * self.y_std + self.y_mean, cond_df, mu, sigma)
        else:
            log_prob = _norm_logpdf(y * self.y_std + self.y_mean, mu, np.sqrt(v))
        return -np.mean(log_prob)


def multi_grad_route(kernel_fn, likelihood):
    """grad_route for MultiSPR: "smn_spr_loss_grad_multi" (MLP / dense ResNet) or "smn_spr_cnn_loss_grad_multi"
    (get_cnn_kernel); anything else raises NotImplementedError, as grad_route does."""
    return grad_route(kernel_fn, likelihood) + "_multi"


class MultiSPR(_ExactGP):
    """Exact GP / Student-t process with C outputs over ONE kernel matrix: y_data [N,C], K~ = K(x,x) + eps I.

    Gaussian likelihood: the C columns are independent GPs that share K~ (the log-pdf is the sum of C
    multivariate_normal.logpdf).  Student-t likelihood: sigma^2 ~ IG(a, b) is shared by all outputs, so the prior over
    all N C outputs is ONE multivariate t, vec(Y) ~ MVT_{NC}(2a, 0, (b/a) (I_C x K~)) -- the model of a C-output network
    whose last-layer variance carries one inverse-gamma scale, and not C one-vs-rest Student-t processes.  Everything that
    is expensive -- the build of K~, its factorisation, -K~^-1 and the tangent pass over the pairs -- is done once for the
    C columns (include/smnngp.h, the *_multi entries); 1 <= C <= 48.

    Trainables and their names are SPR's (kernel.w_std, kernel.b_std, kernel.last_w_std, eps, likelihood.a / .b), so
    train.train_vars, train.build_train_step and the checkpoint reader work on it unchanged.  Classification: targets
    onehot(labels) - 1/C (from_labels), the predicted class is the arg-max of the posterior mean (classify, accuracy)."""

    _multi = True

    def __init__(self, kernel, likelihood, x_data, y_data, y_mean=0., y_std=1., *, eps: float = 1e-6):
        super().__init__()
        _check_scales_length(kernel, x_data)
        self.kernel = kernel
        self.likelihood = likelihood
        self.x_data = as_device(x_data)
        self.num_data = self.x_data.shape[0]
        y = np.asarray(y_data, dtype=np.float64)
        if y.ndim == 1:
            y = y[:, None]
        if y.ndim != 2 or y.shape[0] != self.num_data or y.shape[1] < 1:
            raise ValueError("y_data must be [N,C] with N = %d rows, got %s" % (self.num_data, y.shape))
        self.y_host = np.ascontiguousarray(y)
        self.num_outputs = y.shape[1]
        self.y_data = as_device(self.y_host, self.x_data.ctx, dtype=self.x_data.dtype)
        self.y_mean = float(np.asarray(y_mean))
        self.y_std = float(np.asarray(y_std))
        self.eps = ConstraintTrainVar(eps, constraint=positive())

    @classmethod
    def from_labels(cls, kernel, likelihood, x_data, labels, num_classes, y_mean=0., y_std=1., *, eps: float = 1e-6):
        """The classifier: targets onehot(labels) - 1/num_classes (every row sums to zero, its arg-max is the label)."""
        model = cls(kernel, likelihood, x_data, cls.label_targets(labels, num_classes), y_mean, y_std, eps=eps)
        model._from_labels = True   # (its posteriors take labels in append, through label_targets)
        return model

    @staticmethod
    def label_targets(labels, num_classes):
        labels = np.asarray(labels).reshape(-1)
        c = int(num_classes)
        if labels.size and (labels.min() < 0 or labels.max() >= c or np.any(labels != np.floor(labels))):
            raise ValueError("labels must be integers in [0, %d)" % c)
        y = np.full((labels.shape[0], c), -1.0 / c)
        y[np.arange(labels.shape[0]), labels.astype(np.int64)] += 1.0
        return y

    def _head(self):
        if not hasattr(self.likelihood, "lml_params"):
            raise NotImplementedError("MultiSPR needs a Gaussian or Student-t likelihood")
        return self.likelihood.lml_params()

    def _joint_lml(self, kernel_fn, x, y, eps, df, scale, seen=False):
        """(log-pdf, total quadratic form, info) of y [N,C] under K(x,x) + eps I: the fused build for the MLP family, the
        conv build followed by smn_lml_multi for the conv kernels.  seen: x already carries the kernel function's input
        scales."""
        ctx, n, c = x.ctx, self.num_data, self.num_outputs
        lp, quad, info = C.c_double(), C.c_double(), C.c_int()
        if isinstance(kernel_fn, KernelFn):
            net, act, L, w, b, lw = kernel_fn.params
            x = x if seen else _seen(kernel_fn, x)
            ctx.call("smn_spr_loss_multi", x.dcode, net, act, L, w, b, lw, x.ptr, n, x.shape[1], x.shape[1], y.ptr, c,
                     eps, df, scale, C.byref(lp), C.byref(quad), None, None, C.byref(info))
        elif isinstance(kernel_fn, CnnKernelFn):
            k = kernel_fn(x, None, get="nngp", fill="lower")
            ctx.call("smn_lml_multi", x.dcode, k.ptr, n, n, y.ptr, c, eps, df, scale, C.byref(lp), C.byref(quad), None,
                     None, C.byref(info))
        else:
            raise NotImplementedError("MultiSPR is wired for the nt_kernels factories; got %s" % type(kernel_fn).__name__)
        return lp.value, quad.value, info.value

    def loss(self):
        """-log p(Y) / N; at C = 1 this is SPR.loss."""
        df, scale = self._head()
        lp, _, _ = self._joint_lml(self.kernel.get_kernel_fn(), self.x_data, self.y_data, self.eps.safe_value, df, scale)
        return -lp / self.num_data

    def loss_and_grad(self):
        """(loss, {variable name: d loss / d RAW value}), the analytic counterpart of SPR.loss_and_grad for C columns: one
        factorisation of [[K~], [I], [Y^T]] gives A = K~^-1 Y, -K~^-1, the C quadratic forms and logdet K~, one pass contracts
        G = coef A A^T - C K~^-1 with the forward-mode dK/d(w_std, b_std, last_w_std) (csrc/grad.hip, csrc/cnn_grad.hip), and
        lml_value_and_grads supplies the head in dimension N C with log-determinant C logdet K~.  The conv ResNet, a
        likelihood without lml_params and images above 1024 pixels raise NotImplementedError."""
        return self._lml_loss_and_grad()

    # predict(x) -> (mean [T,C], cov [T,T]) is _DrawsMixin's, shared with SPR

    def _student_quad_f64(self, kernel_fn, scale):
        """tr(Y^T (scale K + 1e-6 I)^-1 Y) with K WITHOUT eps, always in fp64 (SPR._student_quad_f64 for C columns); the
        value of the last parameter setting is kept."""
        key = (type(kernel_fn).__name__, getattr(kernel_fn, "entry", None), tuple(kernel_fn.params), float(scale),
               _scales_key(kernel_fn))
        hit = getattr(self, "_quad64_cache", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        xd, yd = self._f64_data()
        _, quad, info = self._joint_lml(kernel_fn, self._f64_seen(kernel_fn, xd), yd, 1e-6 / scale, 0.0, 1.0, seen=True)
        val = float("nan") if info else quad / scale
        self._quad64_cache = (key, val)
        return val

    def test_nll(self, x, y):
        """-mean_t sum_c log p(y_tc) under the predictive marginals in de-normalised units: N(mean_tc, sqrt(cov_tt)), or
        Student-t with nu + N C degrees of freedom and sigma_t = sqrt(d / (nu + N C) (b/a) cov_tt),
        d = nu + tr(Y^T ((b/a) K + 1e-6 I)^-1 Y) (spax/likelihoods.py:52-65 in dimension N C).  At C = 1: SPR.test_nll."""
        df, scale = self._head()
        mean, cov = self.predict(x)
        t, c = mean.shape
        y = np.asarray(y, dtype=np.float64).reshape(t, c)
        ys = y * self.y_std + self.y_mean
        ms = np.asarray(mean, dtype=np.float64).reshape(t, c) * self.y_std + self.y_mean
        var = np.asarray(cov.diagonal(), dtype=np.float64) * self.y_std ** 2
        if df > 0.0:
            cond_df = df + self.num_data * c
            d = df + self._student_quad_f64(self.kernel.get_kernel_fn(), scale)
            sigma = np.sqrt(d / cond_df * scale * var)
            lp = _t_logpdf(ys, cond_df, ms, sigma[:, None])
        else:
            lp = _norm_logpdf(ys, ms, np.sqrt(var)[:, None])
        return -float(np.mean(np.sum(lp, axis=1)))

    def classify(self, x):
        """Predicted labels: argmax_c of the posterior mean (first maximum)."""
        mean, _ = self.predict(x)
        return np.argmax(np.asarray(mean, dtype=np.float64), axis=1)

    def accuracy(self, x, labels):
        """Fraction of x classified as `labels`."""
        return float(np.mean(self.classify(x) == np.asarray(labels).reshape(-1)))

    def loo_classify(self):
        """Leave-one-out labels of the training points: argmax_c of the leave-one-out mean (first maximum)."""
        return np.argmax(self.loo_predict()[0], axis=1)

    def loo_accuracy(self, labels=None):
        """Fraction of the training points whose leave-one-out label is `labels` (default: the arg-max of y_host)."""
        labels = np.argmax(self.y_host, axis=1) if labels is None else np.asarray(labels).reshape(-1)
        return float(np.mean(self.loo_classify() == labels))


class SVSP(Module):
    """spax/models.py:9-78: sparse variational GP / Student-t process classifier over `num_latent_gps` classes, with the
    reference's constructor, trainables (inducing_variable, q_mu, q_sqrt, eps), `test_acc_nll` and, in place of the
    autodiff `loss`, `loss_and_grad` (every trainable, the inducing images included).

    Everything that grows with the data runs on the device: the cross kernel K(Z, x) and the per-image diagonal
    K(x_t, x_t) of the conv kernels, the posterior moments (smn_svsp_moments; the I x I side in fp64 whatever `dtype` is), and
    the Monte-Carlo softmax head (smn_mc_softmax), which draws its S variates per (point, class) in registers.  Between the
    last two the host turns the T x C variances into sigma = sqrt(scale * var) (one small download and upload per batch).
    The reference's [B,B] test
    covariance is never formed: sample_f_iid reads its diagonal only, so every point is independent of its batch.
    `dtype` is the precision of the images, the cross kernel, the moments and the head's arithmetic.
    K(Z, Z) is kept per (kernel, hyper-parameters, CONTENT of the inducing images): it is I^2 image pairs.  The two I x I
    factorisations are not kept: smn_svsp_moments redoes them in every call, a few launches at I = 200."""

    def __init__(self, prior, kernel, inducing_variable, *, num_latent_gps: int = 1, eps: float = 1e-6, dtype=np.float64):
        super().__init__()
        self.prior = prior
        self.kernel = kernel
        self.num_latent_gps = int(num_latent_gps)
        self.inducing_variable = TrainVar(np.asarray(inducing_variable))
        self.num_inducing = self.inducing_variable.value.shape[0]
        self.q_mu = TrainVar(np.zeros((self.num_latent_gps, self.num_inducing)))
        self.q_sqrt = ConstraintTrainVar(np.ones((self.num_latent_gps, self.num_inducing)), constraint=positive())
        self.eps = ConstraintTrainVar(eps, constraint=positive())
        self.dtype = np.dtype(dtype)
        _lib.dtype_code(self.dtype)                               # float32 / float64 only
        self._kzz_cache = None

    @classmethod
    def from_greedy(cls, prior, kernel, x_pool, num_inducing, *, num_latent_gps: int = 1, eps: float = 1e-6, dtype=np.float64):
        """An SVSP whose inducing images are the `num_inducing` images of x_pool [N,H,W,C] that carry the kernel at its
        current hyper-parameters: the pivots of the greedy pivoted Cholesky of K(x_pool, x_pool) (lowrank.py; largest
        conditional variance first, the pool's N x N matrix is never formed).  Selection is global, without per-class quotas.
        ValueError, before any device call, for num_inducing outside [1, N]; ValueError when the pool runs out of numerical
        rank before num_inducing points are found."""
        from ..lowrank import _check, pivoted_cholesky
        kernel_fn = kernel.get_kernel_fn()
        _check(kernel_fn, x_pool, num_inducing, 0.0, "auto")
        pool = x_pool if isinstance(x_pool, DeviceArray) else np.asarray(x_pool, dtype=np.dtype(dtype))
        res = pivoted_cholesky(kernel_fn, pool, num_inducing)
        if res.rank < int(num_inducing):
            raise ValueError("x_pool has numerical rank %d under this kernel: fewer than num_inducing = %d distinct points"
                             % (res.rank, int(num_inducing)))
        host = pool.numpy() if isinstance(pool, DeviceArray) else pool
        return cls(prior, kernel, host[res.pivots], num_latent_gps=num_latent_gps, eps=eps, dtype=dtype)

    def loss(self, key, x_batch, y_batch, num_train, num_samples, aux=False):
        raise NotImplementedError("SVSP.loss is a value for an autodiff framework to differentiate; this engine returns the "
                                  "negative ELBO together with its analytic gradient: SVSP.loss_and_grad")

    def loss_and_grad(self, key, x_batch, y_batch, num_train, num_samples, *, kernel_grads=True, aux=False, return_gbar=False,
                      inducing_grad=False):
        """(n_elbo, {variable name: d n_elbo / d RAW value}) of spax/models.py:30-56 -- the analytic counterpart of
        objax.GradValues(model.loss, train_vars) in experiments/classification/train.py:61-75 -- for every trainable:
        q_mu and q_sqrt (arrays [C,I]), eps, w_std, b_std, last_w_std, for InverseGammaPrior a and b, and, with
        inducing_grad=True, `inducing_variable` (a float64 array [I,H,W,C]; the variable has no constraint, so the raw value
        is the value).  aux=True appends (-ll, kl / num_train) as the reference's aux does.

        One symmetric fp64 build of K over [Z; x_batch], one smn_svsp_elbo_grad (forward, correlated Monte-Carlo softmax
        head, reverse pass; leaves d loss / d K on the device) and, with kernel_grads, one forward-mode tangent pass
        (smn_kernel_cnn_grad_terms) that contracts d loss / d K with dK / d(w_std, b_std, last_w_std).  That pass exists for
        get_cnn_kernel and images of up to 1024 pixels: anything else raises NotImplementedError with kernel_grads=True;
        kernel_grads=False works for both conv kernels and omits the three kernel entries (the others are the same bits).
        inducing_grad=True adds one reverse pass of the conv kernel over the same images (smn_kernel_cnn_input_grad, fp64,
        seeded with d loss / d K, n_grad = I); it has the tangent pass's limits (get_cnn_kernel, at most 1024 pixels, else
        NotImplementedError), works with kernel_grads either way and leaves every other returned object the same bits.
        The closed-form inverse-gamma terms, (a, b) -> (df, scale, s) and the softplus chain rule are host arithmetic.
        `key` as in test_acc_nll: an int seed or (seed, global index of the batch's first point).  The model's `dtype`
        selects the arithmetic of the head's variates and exponentials; everything else is fp64.
        return_gbar=True appends the device array d loss / d K [I+B, I+B] (what the two conv passes consume).
        A matrix that is not positive definite gives NaN for the loss and every gradient."""
        seed, point0 = split_key(key)
        kernel_fn = self.kernel.get_kernel_fn()
        if not isinstance(kernel_fn, CnnKernelFn):
            raise NotImplementedError("SVSP is wired for get_cnn_kernel / get_conv_resnet_kernel; got %s" % type(kernel_fn).__name__)
        z_host = np.asarray(self.inducing_variable.value, dtype=np.float64)
        x_host = x_batch.numpy() if isinstance(x_batch, DeviceArray) else np.asarray(x_batch)
        x_host = np.asarray(x_host, dtype=np.float64)
        if z_host.ndim != 4 or x_host.ndim != 4 or x_host.shape[1:] != z_host.shape[1:]:
            raise ValueError("x_batch %s does not have the shape of the inducing images %s" % (x_host.shape, z_host.shape[1:]))
        if kernel_grads and (kernel_fn.entry != "smn_kernel_cnn" or z_host.shape[1] * z_host.shape[2] > 1024):
            raise NotImplementedError("kernel_grads=True needs get_cnn_kernel and images of at most 1024 pixels (the tangent "
                                      "pass of smn_kernel_cnn_grad_terms); pass kernel_grads=False")
        if inducing_grad and (kernel_fn.entry != "smn_kernel_cnn" or z_host.shape[1] * z_host.shape[2] > 1024):
            raise NotImplementedError("inducing_grad=True needs get_cnn_kernel and images of at most 1024 pixels (the reverse "
                                      "pass of smn_kernel_cnn_input_grad)")
        ctx = (x_batch.ctx if isinstance(x_batch, DeviceArray) else None) or kernel_fn.ctx or _lib.default_context()
        n_i, n_b, c = self.num_inducing, x_host.shape[0], self.num_latent_gps
        labels = np.ascontiguousarray(np.asarray(y_batch).reshape(-1), dtype=np.int32)
        if labels.shape[0] != n_b:
            raise ValueError("y_batch has %d labels for %d points" % (labels.shape[0], n_b))
        q_mu = np.ascontiguousarray(self.q_mu.value, dtype=np.float64)
        q_raw = np.asarray(self.q_sqrt.value, dtype=np.float64)
        q_var = np.ascontiguousarray(self.q_sqrt.constraint(q_raw), dtype=np.float64)    # diag(q_sqrt) itself: not squared
        if q_mu.shape != (c, n_i) or q_var.shape != (c, n_i):
            raise ValueError("q_mu / q_sqrt must be [num_latent_gps, num_inducing] = %s" % ((c, n_i),))
        pp = self.prior.elbo_params()
        eps, n_train = self.eps.safe_value, float(num_train)
        u = ctx.to_device(np.ascontiguousarray(np.concatenate([z_host, x_host])))         # fp64 whatever the model's dtype
        k = kernel_fn(u, None, get="nngp")
        n_u = n_i + n_b
        q_mu_d, q_var_d = ctx.to_device(q_mu), ctx.to_device(q_var)
        g_mu_d, g_var_d = ctx.empty((c, n_i), np.float64), ctx.empty((c, n_i), np.float64)
        gbar = ctx.empty((n_u, n_u), np.float64)
        nll, kl_n, g_eps, gscale, g_s, dfterm = (C.c_double() for _ in range(6))
        info = C.c_int()
        ctx.call("smn_svsp_elbo_grad", _lib.dtype_code(self.dtype), k.ptr, n_u, n_i, n_b, c, q_mu_d.ptr, q_var_d.ptr, eps, pp["s"],
                 n_train, labels.ctypes.data_as(C.POINTER(C.c_int)), int(num_samples), pp["df"], pp["scale"], seed, point0, None,
                 None, C.byref(nll), C.byref(kl_n), g_mu_d.ptr, g_var_d.ptr, C.byref(g_eps), C.byref(gscale), C.byref(g_s),
                 C.byref(dfterm), gbar.ptr, n_u, C.byref(info))
        names = {id(v): name for name, v in self.vars().items()}
        grads = {}
        nll_v, kl_v = nll.value, kl_n.value + pp["kl_extra"] / n_train
        grads[names[id(self.q_mu)]] = g_mu_d.raw_numpy()
        grads[names[id(self.q_sqrt)]] = g_var_d.raw_numpy() * self.q_sqrt.constraint.grad(q_raw)
        d_con = {"eps": (self.eps, g_eps.value)}                                          # d loss / d constrained value
        if pp["df"] > 0.0:
            a, b = self.prior.a.safe_value, self.prior.b.safe_value                       # df = 2a, scale = b/a, s = a/b
            d_con["a"] = (self.prior.a, 2.0 * dfterm.value - gscale.value * b / (a * a) + g_s.value / b + pp["d_extra"]["a"] / n_train)
            d_con["b"] = (self.prior.b, gscale.value / a - g_s.value * a / (b * b) + pp["d_extra"]["b"] / n_train)
        if kernel_grads:
            terms = (C.c_double * 4)()
            if info.value == 0:
                act, depth, w, b_, lw = kernel_fn.params
                zeros = ctx.to_device(np.zeros(n_u))
                ctx.call("smn_kernel_cnn_grad_terms", _lib.F64, act, depth, w, b_, lw, u.ptr, n_u, u.shape[1], u.shape[2], u.shape[3],
                         gbar.ptr, n_u, zeros.ptr, 0.0, terms)
            for i, key_ in enumerate(("w_std", "b_std", "last_w_std")):
                d_con[key_] = (getattr(self.kernel, key_), terms[i] if info.value == 0 else float("nan"))
        grads.update(_raw_grads(self, d_con))
        if inducing_grad:
            if info.value == 0:
                act, depth, w, b_, lw = kernel_fn.params
                gz = ctx.empty(z_host.shape, np.float64)
                ctx.call("smn_kernel_cnn_input_grad", _lib.F64, act, depth, w, b_, lw, u.ptr, n_u, u.shape[1], u.shape[2], u.shape[3],
                         gbar.ptr, n_u, n_i, gz.ptr)
                grads[names[id(self.inducing_variable)]] = gz.raw_numpy()
            else:
                grads[names[id(self.inducing_variable)]] = np.full(z_host.shape, np.nan)
        value = nll_v + kl_v
        if info.value != 0:
            nan = float("nan")
            value, nll_v, kl_v = nan, nan, nan
        out = (value, grads)
        if aux:
            out += (nll_v, kl_v)
        if return_gbar:
            out += (gbar,)
        return out

    # ---- device state that depends on the kernel hyper-parameters and the inducing images only
    def inducing_state(self, kernel_fn=None, ctx=None, refresh=False):
        """(Z on the device in the model's dtype, K(Z, Z) on the device in fp64) at the current hyper-parameters.  Kept between
        calls; whether the kept pair still belongs to the inducing images is decided by comparing their content with a copy
        (an array edited in place, or another one at a recycled address, is seen).  refresh: rebuild regardless."""
        kernel_fn = kernel_fn or self.kernel.get_kernel_fn()
        ctx = ctx or _lib.default_context()
        if not isinstance(kernel_fn, CnnKernelFn):
            raise NotImplementedError("SVSP evaluation is wired for get_cnn_kernel / get_conv_resnet_kernel (the kernels "
                                      "of experiments/classification); got %s" % type(kernel_fn).__name__)
        z_host = self.inducing_variable.value
        if z_host.ndim != 4:
            raise ValueError("inducing_variable must be [I,H,W,C] images")
        key = (kernel_fn.entry, tuple(kernel_fn.params), z_host.shape, ctx)
        hit = self._kzz_cache
        if not refresh and hit is not None and hit[0] == key and np.array_equal(hit[3], z_host):
            return hit[1], hit[2]
        z64 = ctx.to_device(np.ascontiguousarray(z_host, dtype=np.float64))
        k_zz = kernel_fn(z64, None, get="nngp")                   # fp64, full, whatever the model's dtype
        z = z64 if self.dtype == np.float64 else ctx.to_device(np.ascontiguousarray(z_host, dtype=self.dtype))
        self._kzz_cache = (key, z, k_zz, z_host.copy())
        return z, k_zz

    def posterior_moments(self, x_batch, ctx=None):
        """(mean [T,C], var [T,C]) device arrays of the latent function at x_batch, info, number of var entries <= 0."""
        ctx = ctx or (x_batch.ctx if isinstance(x_batch, DeviceArray) else _lib.default_context())
        kernel_fn = self.kernel.get_kernel_fn()
        z, k_zz = self.inducing_state(kernel_fn, ctx)
        x = as_device(x_batch, ctx, dtype=self.dtype)
        if len(x.shape) != 4 or tuple(x.shape[1:]) != tuple(z.shape[1:]):
            raise ValueError("x_batch %s does not have the shape of the inducing images %s (resizing is the caller's job)"
                             % (tuple(x.shape), tuple(z.shape[1:])))
        t, (n_i, c) = x.shape[0], (self.num_inducing, self.num_latent_gps)
        q_mu = np.asarray(self.q_mu.value, dtype=np.float64)
        q_var = np.asarray(self.q_sqrt.constraint(self.q_sqrt.value), dtype=np.float64)   # diag(q_sqrt) itself: not squared
        if q_mu.shape != (c, n_i) or q_var.shape != (c, n_i):
            raise ValueError("q_mu / q_sqrt must be [num_latent_gps, num_inducing] = %s" % ((c, n_i),))
        k_zt = kernel_fn(z, x, get="nngp")                        # [I,T]
        ktt = kernel_fn.diag(x)                                   # [T] prior variances, the bits of the symmetric diagonal
        mean, var = ctx.empty((t, c), self.dtype), ctx.empty((t, c), self.dtype)
        info, nonpos = C.c_int(), C.c_int64()
        q_mu_d, q_var_d = ctx.to_device(q_mu), ctx.to_device(q_var)                        # fp64 whatever the model's dtype
        ctx.call("smn_svsp_moments", x.dcode, k_zz.ptr, k_zt.ptr, ktt.ptr, q_mu_d.ptr, q_var_d.ptr, n_i, t, c,
                 self.eps.safe_value, mean.ptr, var.ptr, C.byref(info), C.byref(nonpos))
        return mean, var, info.value, nonpos.value

    def predict_scores(self, key, x_batch, y_batch, num_samples):
        """Per point: (log-likelihood of the label [T], predicted class [T], class scores [T,C]) as host arrays."""
        seed, point0 = split_key(key)
        mean, var, _, _ = self.posterior_moments(x_batch)
        ctx = mean.ctx
        t, c = mean.shape
        labels = np.ascontiguousarray(np.asarray(y_batch).reshape(-1), dtype=np.int32)
        if labels.shape[0] != t:
            raise ValueError("y_batch has %d labels for %d points" % (labels.shape[0], t))
        df, scale = self.prior.head_params()
        with np.errstate(invalid="ignore"):
            sigma = ctx.to_device(np.sqrt(scale * var.raw_numpy()).astype(self.dtype))    # NaN where var < 0, as the reference
        ll, score = ctx.empty((t,), np.float64), ctx.empty((t, c), np.float64)
        pred_d = C.c_void_p()
        ctx.call("smn_malloc", max(4 * t, 16), C.byref(pred_d))
        try:
            ctx.call("smn_mc_softmax", mean.dcode, mean.ptr, sigma.ptr, labels.ctypes.data_as(C.POINTER(C.c_int)), t, c,
                     int(num_samples), df, seed, point0, None, ll.ptr, pred_d, score.ptr)
            pred = np.empty(t, dtype=np.int32)
            ctx.call("smn_memcpy_d2h", pred.ctypes.data_as(C.c_void_p), pred_d, 4 * t)
        finally:
            ctx.call("smn_free", pred_d)
        return ll.raw_numpy(), pred, score.raw_numpy()

    # ---- spax/models.py:58-78
    def test_acc_nll(self, key, x_batch, y_batch, num_samples):
        """(nll, correct_count) of one batch.  `key`: int seed or (seed, global index of the batch's first point)."""
        ll, pred, _ = self.predict_scores(key, x_batch, y_batch, num_samples)
        return float(-np.mean(ll)), int(np.sum(pred == np.asarray(y_batch).reshape(-1)))

    def evaluate(self, x, y, num_samples, seed=10, batch=None):
        """experiments/classification/test.py:45-57 (test_epoch) over a whole set -> (nll, accuracy in percent).  The set
        is cut into chunks of `batch` points for memory only: a point's variates are keyed by its global index, so the
        result does not depend on the chunking."""
        n = len(y)
        batch = int(batch) if batch else 2500
        nll_sum, correct = 0.0, 0
        for i0 in range(0, n, batch):
            i1 = min(n, i0 + batch)
            nll, cc = self.test_acc_nll((seed, i0), x[i0:i1], y[i0:i1], num_samples)
            nll_sum += nll * (i1 - i0)
            correct += cc
        return nll_sum / n, correct * 100.0 / n
