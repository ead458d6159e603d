#!/usr/bin/env python3
"""Automatic relevance determination on the device path: y depends on 2 of 8 input features, the model learns one positive
scale per feature (NNGPKernel(..., input_scales=...)) by marginal likelihood, and the six irrelevant scales shrink.

    python examples/ard_synthetic.py [--kernel {nngp,ntk}]

Trains every variable (w_std, b_std, last_w_std, eps, a / b and the scales) with the analytic gradient
(SPR.loss_and_grad -> smn_spr_loss_grad_inputs) and prints the scales and the test NLL beside those of the same model without
scales, for the Gaussian and the Student-t likelihood.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smnngp import nt_kernels, train                                  # noqa: E402
from smnngp.spax.kernels import NNGPKernel, NTKKernel                 # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR                                    # noqa: E402

D, N_TRAIN, N_TEST, STEPS, LR = 8, 160, 200, 150, 0.05


def dataset(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_TRAIN + N_TEST, D))
    y = np.sin(2.0 * x[:, 0]) + 0.5 * x[:, 1] + 0.1 * rng.standard_normal(len(x))
    ym, ys = y[:N_TRAIN].mean(), y[:N_TRAIN].std()
    y = (y - ym) / ys
    return (x[:N_TRAIN], y[:N_TRAIN]), (x[N_TRAIN:], y[N_TRAIN:]), (ym, ys)


def fit(kernel_cls, method, scales, train_set, stats):
    kernel = kernel_cls(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.3, 1.0,
                        input_scales=scales)
    likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    model = SPR(kernel, likelihood, train_set[0], train_set[1], stats[0], stats[1], eps=1e-2)
    step = train.build_train_step(model, method="analytic")
    first = last = None
    for _ in range(STEPS):
        last = step(LR)
        first = last if first is None else first
    return model, first, last


def main():
    argv = sys.argv[1:]
    kernel_cls = NTKKernel if argv[:2] == ["--kernel", "ntk"] else NNGPKernel
    train_set, test_set, stats = dataset()
    for method in ("gp", "tp"):
        plain, p0, p1 = fit(kernel_cls, method, None, train_set, stats)
        ard, a0, a1 = fit(kernel_cls, method, np.ones(D), train_set, stats)
        s = ard.kernel.get_input_scales()
        print("%s  without scales: loss %.4f -> %.4f  test NLL %.4f" % (method, p0, p1, plain.test_nll(*test_set)))
        print("%s  with scales:    loss %.4f -> %.4f  test NLL %.4f" % (method, a0, a1, ard.test_nll(*test_set)))
        print("    scales: %s   (features 0 and 1 carry the signal)" % " ".join("%.3f" % v for v in s))


if __name__ == "__main__":
    main()
