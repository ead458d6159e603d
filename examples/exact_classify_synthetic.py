#!/usr/bin/env python3
"""Exact multi-class classification with MultiSPR (gp and tp) on the synthetic image problem of classify_synthetic.py:
class templates plus noise, targets onehot(label) - 1/C, ALL C outputs carried through one factorisation of the conv-NNGP
kernel matrix.  A few Adam steps on the hyper-parameters with the analytic gradient (smn_spr_cnn_loss_grad_multi), then
the loss, the test NLL of the targets and the accuracy of argmax_c mean.  --objective loo trains on the leave-one-out
predictive log-probability of the training set instead of the log-marginal likelihood (smn_spr_cnn_loo_grad) and prints the
leave-one-out accuracy and NLL of the training points beside the test figures.

    python examples/exact_classify_synthetic.py [--train 400] [--test 400] [--classes 10] [--hw 8] [--channels 1]
                                                [--layers 2] [--steps 5] [--lr 0.05] [--dtype float64|float32]
                                                [--objective lml|loo]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smnngp import nt_kernels, train                                          # noqa: E402
from smnngp.spax.kernels import NNGPKernel                                    # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood    # noqa: E402
from smnngp.spax.models import MultiSPR                                       # noqa: E402


def problem(num_train, num_test, num_class, hw, channels, seed=5):
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((num_class, hw, hw, channels))

    def images(n):
        lab = rng.integers(0, num_class, n)
        return templates[lab] + 1.6 * rng.standard_normal((n, hw, hw, channels)), lab

    return images(num_train) + images(num_test)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train", type=int, default=400)
    ap.add_argument("--test", type=int, default=400)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--hw", type=int, default=8)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--objective", default="lml", choices=["lml", "loo"])
    args = ap.parse_args()
    loo = args.objective == "loo"
    dtype = np.dtype(args.dtype).type
    x, lab, xt, labt = problem(args.train, args.test, args.classes, args.hw, args.channels)
    x, xt = x.astype(dtype), xt.astype(dtype)
    yt = MultiSPR.label_targets(labt, args.classes)
    print("%d training and %d test images %dx%dx%d, %d classes, %d-layer ReLU get_cnn_kernel, %s"
          % (args.train, args.test, args.hw, args.hw, args.channels, args.classes, args.layers, args.dtype))
    for method in ("gp", "tp"):
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(args.layers, args.classes, "relu", w_std=w, b_std=b,
                                                                      last_w_std=l), 1.2, 0.1, 1.0)
        lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
        model = MultiSPR.from_labels(kernel, lik, x, lab, args.classes, eps=args.eps)
        step = train.build_train_step(model, method="auto", objective=args.objective)

        def loo_report():
            return "  LOO accuracy %.2f %%  LOO NLL %.6f" % (100.0 * model.loo_accuracy(lab), model.loo_loss()) if loo else ""

        print("%s: start  loss %.6f  test NLL %.6f  accuracy %.2f %%%s"
              % (method, model.loss(), model.test_nll(xt, yt), 100.0 * model.accuracy(xt, labt), loo_report()))
        t0 = time.perf_counter()
        for it in range(args.steps):
            print("%s: step %d  loss %.6f" % (method, it, step(args.lr)))
        dt = time.perf_counter() - t0
        print("%s: end    loss %.6f  test NLL %.6f  accuracy %.2f %%%s   (%.1f ms per step)"
              % (method, model.loss(), model.test_nll(xt, yt), 100.0 * model.accuracy(xt, labt), loo_report(),
                 1e3 * dt / max(args.steps, 1)))


if __name__ == "__main__":
    main()
