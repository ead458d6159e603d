"""Host-side holder of the NNGP kernel's three positive hyper-parameters — the counterpart of the class the
reference defines at spax/kernels.py:9-41 (same public names: K, predict, get_params, get_kernel_fn; the trainables
w_std / b_std / last_w_std are the names its checkpoint reader looks for, experiments/regression/test.py:38-43).

Nothing numerical happens here: a kernel function built by `nt_kernels` is a handle on the fused device kernels, and
`predict` hands (kernel_fn, x, y) to the augmented-Cholesky posterior of `predict.py`.
"""
from __future__ import annotations

import numpy as np

from ..nt_kernels import CnnKernelFn, KernelFn
from ..predict import gradient_descent_mse_ensemble
from .base import ConstraintTrainVar, Module
from .bijectors import positive

__all__ = ["NNGPKernel", "NTKKernel"]

_TRAINABLES = ("w_std", "b_std", "last_w_std")


class NNGPKernel(Module):
    """`get_kernel_fn(w_std, b_std, last_w_std) -> kernel_fn` is any of the `nt_kernels.get_*_kernel` factories with the
    architecture arguments bound (experiments/regression/train.py:128-134).

    input_scales (default None): a sequence of d positive numbers, one per input feature -- automatic relevance
    determination.  The covariance function becomes that of the scaled inputs, k(x, x') = K(s o x, s o x'), i.e. a per-feature
    prior variance of the first-layer weights, and s is ONE more trainable, the vector variable `input_scales` (positive(),
    stored softplus-inverse).  The MLP / dense-ResNet factories only: a conv kernel or a foreign callable raises
    NotImplementedError in get_kernel_fn, before any device call.  None registers nothing: vars() is what it was."""

    def __init__(self, get_kernel_fn, w_std: float = 1.0, b_std: float = 1.0, last_w_std: float = 1.0, input_scales=None):
        super().__init__()
        if not callable(get_kernel_fn):
            raise TypeError("get_kernel_fn must be callable: (w_std, b_std, last_w_std) -> kernel_fn")
        self._get_kernel_fn = get_kernel_fn
        for name, value in zip(_TRAINABLES, (w_std, b_std, last_w_std)):
            setattr(self, name, ConstraintTrainVar(value, constraint=positive()))   # stored softplus-inverse
        if input_scales is not None:
            s = np.array(input_scales, dtype=np.float64).reshape(-1)
            if s.size == 0 or not np.all(np.isfinite(s)) or not np.all(s > 0.0):
                raise ValueError("input_scales must be a non-empty sequence of positive finite numbers")
            self.input_scales = ConstraintTrainVar(s, constraint=positive())

    # -- current (constrained) values -------------------------------------------------------------------------
    def get_params(self):
        """(w_std, b_std, last_w_std) as positive floats — spax/kernels.py:34-35."""
        return tuple(getattr(self, name).safe_value for name in _TRAINABLES)

    def get_kernel_fn(self):
        """A kernel function at the current hyper-parameters; rebuilt on every call because the trainables may have
        moved since the last one (spax/kernels.py:37-41).  With input scales, their current values ride on it."""
        kernel_fn = self._get_kernel_fn(*self.get_params())
        s = self.get_input_scales()
        if s is None:
            return kernel_fn
        if not isinstance(kernel_fn, KernelFn):
            raise NotImplementedError("input_scales need an MLP / dense-ResNet kernel function (get_mlp_kernel, "
                                      "get_dense_resnet_kernel); got %s" % type(kernel_fn).__name__)
        return kernel_fn.with_input_scales(s)

    def get_input_scales(self):
        """The current (constrained) input scales as a float64 vector, or None."""
        var = getattr(self, "input_scales", None)
        return None if var is None else np.asarray(var.constraint(var.value), dtype=np.float64).reshape(-1)

    # -- the two uses the model makes of a kernel function ----------------------------------------------------
    def K(self, kernel_fn, x, x2=None):
        """NNGP kernel matrix of x against x2 (against itself when x2 is None) — spax/kernels.py:23-27.  Passing x
        twice, as the reference does, would hide the symmetry from the device kernel; None keeps the lower-tile path."""
        other = None if (x2 is None or x2 is x) else x2
        return kernel_fn(x, other, get="nngp")

    def predict(self, kernel_fn, x, y, x_test, eps=1e-6):
        """Posterior mean [T, C] and covariance [T, T] at x_test — spax/kernels.py:29-32.  `eps` is neural_tangents'
        RELATIVE ridge (diag_reg), not the absolute jitter of the likelihood heads."""
        posterior = gradient_descent_mse_ensemble(kernel_fn, x, y, diag_reg=eps)
        return tuple(posterior(x_test=x_test, get="nngp", compute_cov=True))


class NTKKernel(NNGPKernel):
    """Drop-in sibling of NNGPKernel whose covariance function is the neural tangent kernel Theta of the same architecture:
    same trainables, names, get_params, get_kernel_fn, K and predict.  With it SPR / MultiSPR are exact GPs (or Student-t
    processes) on Theta~ = Theta(X,X) + eps I: loss, gradients, leave-one-out, predictions, draws and classification.

    The semantics are "a GP whose covariance function is Theta": posterior mean Theta_td Theta~^-1 y and covariance
    Theta_tt - Theta_td Theta~^-1 Theta_dt.  This is deliberately NOT neural_tangents' get="ntk" ensemble covariance
    (K_tt + a^T K_dd a - a^T K_dt - K_td a, the spread of an ensemble of trained networks), which stays where it is:
    gradient_descent_mse_ensemble(...)(get="ntk").  The two means coincide.

    get_mlp_kernel and get_dense_resnet_kernel are fused on the device (the SMN_NET_NTK flag of the C ABI).  The conv
    factories have no Theta: NotImplementedError, before any device call.  Any other callable is asked for get="ntk", as
    NNGPKernel asks such a callable for get="nngp"."""

    def get_kernel_fn(self):
        kernel_fn = super().get_kernel_fn()
        if isinstance(kernel_fn, CnnKernelFn):
            raise NotImplementedError("NTKKernel: the conv kernels are NNGP-only (get_mlp_kernel / get_dense_resnet_kernel "
                                      "have the tangent kernel)")
        return kernel_fn.with_cov("ntk") if isinstance(kernel_fn, KernelFn) else kernel_fn

    def K(self, kernel_fn, x, x2=None):
        """Theta of x against x2 (against itself when x2 is None)."""
        if isinstance(kernel_fn, CnnKernelFn):
            raise NotImplementedError("NTKKernel: the conv kernels are NNGP-only")
        other = None if (x2 is None or x2 is x) else x2
        return kernel_fn(x, other, get="ntk")

    def predict(self, kernel_fn, x, y, x_test, eps=1e-6):
        """Posterior mean [T, C] and covariance [T, T] of the GP with covariance function Theta at x_test, with the relative
        ridge of NNGPKernel.predict: Theta~ = Theta_dd + eps tr(Theta_dd)/N I."""
        if isinstance(kernel_fn, CnnKernelFn):
            raise NotImplementedError("NTKKernel: the conv kernels are NNGP-only")
        posterior = gradient_descent_mse_ensemble(kernel_fn, x, y, diag_reg=eps)
        return tuple(posterior(x_test=x_test, get="ntk_gp", compute_cov=True))
