"""spax/priors.py mirror — the mixing priors of the sparse variational classifier (SVSP): `GaussianPrior` (svgp) and
`InverseGammaPrior(alpha, beta)` (svtp), with the reference's names and trainables (a, b).

`sample_f_iid` (spax/priors.py:28-34, :60-68) is served by the device generator of the library
(smn_rng_variates: Philox4x32-10, include/smnngp.h); SVSP.test_acc_nll does not even call it -- its head draws the same
variates in registers -- but the method is kept so that code written against the reference runs.  `sample_f`
(correlated draws from the full [B,B] covariance) and `kl_divergence` are the two halves of the training loss; the
engine computes both, with their gradients, inside one device call (SVSP.loss_and_grad -> smn_svsp_elbo_grad), so as
stand-alone methods they raise NotImplementedError.  `elbo_params` gives that call what it needs from the prior: df,
scale, s = the weight of the q_mu quadratic form in the KL, and the closed-form inverse-gamma terms with their
derivatives (priors.py:78-81 of the reference).

`key` is an int seed or a pair (seed, point0), point0 being the global index of the first point of the batch: a variate
is a function of (seed, global point index, class, draw, df) alone.  Bit parity with a JAX PRNG key is impossible and
not claimed.
"""
from __future__ import annotations

import numpy as np

from .._lib import default_context
from .base import ConstraintTrainVar, Module
from .bijectors import positive

__all__ = ["Prior", "GaussianPrior", "InverseGammaPrior", "split_key"]


def split_key(key):
    """int seed or (seed, point0) -> (seed as uint64, point0)."""
    if isinstance(key, (tuple, list)):
        seed, point0 = key
    else:
        seed, point0 = key, 0
    seed, point0 = int(seed), int(point0)
    if point0 < 0:
        raise ValueError("point0 must be >= 0")
    return seed & 0xFFFFFFFFFFFFFFFF, point0


class Prior(Module):
    def head_params(self):
        """(df, variance scale): variates are Student-t(df) (df <= 0: normal) and sigma = sqrt(scale * var)."""
        raise NotImplementedError

    def sample_f_iid(self, key, mean, cov_or_var, num_samples, ctx=None, dtype=np.float64):
        """mean [C,B]; cov_or_var [C,B,B] (only its diagonal is read, as in the reference) or [C,B] variances ->
        device samples [C,B,S] = mean + sigma * xi with xi from smn_rng_variates."""
        ctx = ctx or default_context()
        seed, point0 = split_key(key)
        df, scale = self.head_params()
        mean = np.asarray(mean, dtype=np.float64)
        var = np.asarray(cov_or_var, dtype=np.float64)
        if var.ndim == 3:
            var = np.diagonal(var, axis1=-2, axis2=-1)
        if mean.ndim != 2 or var.shape != mean.shape:
            raise ValueError("mean must be [C,B] and cov_or_var [C,B,B] or [C,B]")
        num_class, num_batch = mean.shape
        with np.errstate(invalid="ignore"):
            sigma = np.sqrt(scale * var)                              # NaN for a negative variance, as jnp.sqrt gives
        xi = ctx.empty((num_batch, num_class, int(num_samples)), dtype)
        ctx.call("smn_rng_variates", xi.dcode, seed, df, point0, num_batch, num_class, int(num_samples), xi.ptr)
        f = xi.raw_numpy().transpose(1, 0, 2) * sigma[..., None] + mean[..., None]
        return ctx.to_device(np.ascontiguousarray(f, dtype=dtype))

    def sample_f(self, key, mean, cov, num_samples):
        raise NotImplementedError("sample_f draws correlated samples for the training loss of SVSP; the engine draws them "
                                  "on the device inside SVSP.loss_and_grad (smn_svsp_head_grad), not as a separate array")

    def kl_divergence(self, k_ii, k_ii_inv, q_mu, q_sigma, num_inducing, num_class):
        raise NotImplementedError("kl_divergence belongs to the training loss of SVSP; SVSP.loss_and_grad(..., aux=True) "
                                  "returns it (divided by num_train) next to the likelihood term")

    def elbo_params(self):
        """dict(df, scale, s, kl_extra, d_extra) for SVSP.loss_and_grad: kl = kl_gaussian(s) + kl_extra, and d_extra maps a
        trainable of the prior to d kl_extra / d constrained value."""
        raise NotImplementedError


class GaussianPrior(Prior):
    def head_params(self):
        return 0.0, 1.0

    def elbo_params(self):
        return dict(df=0.0, scale=1.0, s=1.0, kl_extra=0.0, d_extra={})


class InverseGammaPrior(Prior):
    def __init__(self, alpha, beta):
        super().__init__()
        self.alpha = alpha
        self.beta = beta
        self.a = ConstraintTrainVar(alpha, constraint=positive())
        self.b = ConstraintTrainVar(beta, constraint=positive())

    def head_params(self):
        a, b = self.a.safe_value, self.b.safe_value
        return 2.0 * a, b / a

    def elbo_params(self):
        import math
        from .utils import digamma, trigamma
        a, b = self.a.safe_value, self.b.safe_value
        alpha, beta = float(self.alpha), float(self.beta)
        extra = (alpha * math.log(b / beta) - math.lgamma(a) + math.lgamma(alpha) + (a - alpha) * digamma(a)
                 + (beta - b) * a / b)                                             # priors.py:78-81
        return dict(df=2.0 * a, scale=b / a, s=a / b, kl_extra=extra,
                    d_extra=dict(a=(a - alpha) * trigamma(a) + (beta - b) / b, b=alpha / b - a * beta / (b * b)))
