"""spax — host-side mirror of the hot-path surface of the reference library of the same name.

Sub-modules (import them by name, as the reference's experiments do):
    spax.models       SPR, LowRankSPR (SPR on a rank-M pivoted-Cholesky factor), IterativeSPR (the exact posterior by matrix-free PCG), MultiSPR (C outputs over one kernel matrix),
                      SVSP (evaluation: test_acc_nll / evaluate)
    spax.kernels      NNGPKernel, NTKKernel (the same models on the tangent kernel of the MLP / dense-ResNet architectures)
    spax.likelihoods  GaussianLikelihood, StudentTLikelihood
    spax.priors       GaussianPrior, InverseGammaPrior (sample_f_iid; the training-side methods raise)
    spax.bijectors    positive
    spax.utils        jitter, multivariate_normal_logpdf, multivariate_t_logpdf, ...
Training the sparse variational classifier (SVSP.loss, Prior.sample_f, Prior.kl_divergence) is not part of this path.
"""
import importlib as _importlib

from .base import ConstraintTrainVar, Module, TrainVar

for _name in ("bijectors", "utils", "likelihoods", "kernels", "priors", "models"):
    globals()[_name] = _importlib.import_module("." + _name, __name__)
del _name

__all__ = ["Module", "TrainVar", "ConstraintTrainVar", "bijectors", "utils", "likelihoods", "kernels", "priors", "models"]
