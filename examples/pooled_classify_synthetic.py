#!/usr/bin/env python3
"""Where global average pooling matters: a synthetic image problem whose class is a small PATTERN placed at a RANDOM
position.  Each image is noise plus one of C 3x3 patterns at a position drawn per image, so two images of the same class
rarely agree pixel by pixel.  get_cnn_kernel (Flatten) compares pixel (h, w) of one image with pixel (h, w) of the other
only and sees the class when the positions happen to coincide; get_cnn_pool_kernel (GlobalAvgPool) compares every pixel of
one image with every pixel of the other and is blind to the position.  Both run through MultiSPR.from_labels (exact GP and
exact Student-t process) from the same hyper-parameters; printed per kernel: the time of one build of K(X, X), and per head
the test accuracy, the test NLL of the targets and the loss before and after a few Adam steps of
train.build_train_step(method="auto") -- analytic gradients for get_cnn_kernel, central differences for the pooled kernel,
which has no analytic gradient.

    python examples/pooled_classify_synthetic.py [--train 300] [--test 300] [--classes 4] [--hw 8] [--layers 3]
                                                 [--steps 20] [--lr 0.1] [--dtype float64|float32]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smnngp import nt_kernels, train                                          # noqa: E402
from smnngp._lib import as_device                                             # noqa: E402
from smnngp.spax.kernels import NNGPKernel                                    # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood    # noqa: E402
from smnngp.spax.models import MultiSPR                                       # noqa: E402


def problem(num_train, num_test, num_class, hw, seed=5, noise=0.35):
    rng = np.random.default_rng(seed)
    patterns = 1.5 * rng.standard_normal((num_class, 3, 3))

    def images(n):
        lab = rng.integers(0, num_class, n)
        x = noise * rng.standard_normal((n, hw, hw, 1))
        for i in range(n):
            r, c = rng.integers(0, hw - 2, 2)
            x[i, r:r + 3, c:c + 3, 0] += patterns[lab[i]]
        return x, lab

    return images(num_train) + images(num_test)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train", type=int, default=300)
    ap.add_argument("--test", type=int, default=300)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--hw", type=int, default=8)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.1)
    args = ap.parse_args()
    dtype = np.dtype(args.dtype).type
    x, lab, xt, labt = problem(args.train, args.test, args.classes, args.hw)
    x, xt = x.astype(dtype), xt.astype(dtype)
    yt = MultiSPR.label_targets(labt, args.classes)
    print("%d training and %d test images %dx%dx1, %d classes (a 3x3 pattern at a random position), %d ReLU layers, %s"
          % (args.train, args.test, args.hw, args.hw, args.classes, args.layers, args.dtype))
    for name, factory in (("get_cnn_kernel", nt_kernels.get_cnn_kernel), ("get_cnn_pool_kernel", nt_kernels.get_cnn_pool_kernel)):
        kfn = factory(args.layers, args.classes, "relu", w_std=1.4, b_std=0.1, last_w_std=1.0)
        xd = as_device(x)
        times = []
        for _ in range(5):                       # the first builds pay for the workspaces; the median is reported
            xd.ctx.synchronize()
            t0 = time.perf_counter()
            kfn(xd, None, fill="lower")
            xd.ctx.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        print("%-20s one build of K(X, X): %.2f ms (median of 5)" % (name, float(np.median(times))))
        for method in ("gp", "tp"):
            kernel = NNGPKernel(lambda w, b, l, f=factory: f(args.layers, args.classes, "relu", w_std=w, b_std=b, last_w_std=l),
                                1.4, 0.1, 1.0)
            lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
            model = MultiSPR.from_labels(kernel, lik, x, lab, args.classes, eps=args.eps)
            # analytic gradients for get_cnn_kernel; the pooled kernel has none and "auto" takes central differences
            step = train.build_train_step(model, method="auto")
            for when in ("start", "end"):
                print("%-20s %s %-5s: test accuracy %6.2f %%  test NLL %9.5f  loss %9.5f"
                      % (name, method, when, 100.0 * model.accuracy(xt, labt), model.test_nll(xt, yt), model.loss()))
                if when == "start":
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step(args.lr)
                    print("%-20s %s      : %d Adam steps, %.1f ms per step"
                          % (name, method, args.steps, 1e3 * (time.perf_counter() - t0) / max(args.steps, 1)))


if __name__ == "__main__":
    main()
