#!/usr/bin/env python3
"""Which pixels moved this prediction?  Saliency maps from a fitted conv-NNGP classifier.

The problem of pooled_classify_synthetic.py: every image is noise plus one of C 3x3 patterns at a position drawn per image.
MultiSPR.from_labels over get_cnn_kernel (exact GP and exact Student-t process) is fitted once (`model.posterior()`), and
`post.predict_grad(x_test, var=False)` returns d mean[t, k] / d x_t for every test image and class in one pass per chunk
(csrc/cnn_input_grad.hip, the cross multi-seed form).  Printed per class: the share of sum |d mean_k / d x| that falls inside
the 3x3 window where the test image's pattern sits, averaged over the test images of that class, beside the 9/64 a map that
ignored the pattern would put there (for --hw 8).  A number, not an assertion.

    python examples/saliency_synthetic.py [--train 300] [--test 100] [--classes 4] [--hw 8] [--layers 3] [--dtype float64|float32]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smnngp import nt_kernels                                                 # noqa: E402
from smnngp.spax.kernels import NNGPKernel                                    # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood    # noqa: E402
from smnngp.spax.models import MultiSPR                                       # noqa: E402


def problem(num_train, num_test, num_class, hw, seed=5, noise=0.35):
    """pooled_classify_synthetic.problem, which also returns where each pattern was put."""
    rng = np.random.default_rng(seed)
    patterns = 1.5 * rng.standard_normal((num_class, 3, 3))

    def images(n):
        lab = rng.integers(0, num_class, n)
        x = noise * rng.standard_normal((n, hw, hw, 1))
        pos = np.zeros((n, 2), dtype=np.int64)
        for i in range(n):
            r, c = rng.integers(0, hw - 2, 2)
            x[i, r:r + 3, c:c + 3, 0] += patterns[lab[i]]
            pos[i] = r, c
        return x, lab, pos

    return images(num_train) + images(num_test)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train", type=int, default=300)
    ap.add_argument("--test", type=int, default=100)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--hw", type=int, default=8)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--eps", type=float, default=1e-2)
    args = ap.parse_args()
    dtype = np.dtype(args.dtype).type
    x, lab, _, xt, labt, post = problem(args.train, args.test, args.classes, args.hw)
    x, xt = x.astype(dtype), xt.astype(dtype)
    chance = 9.0 / (args.hw * args.hw)
    print("%d training and %d test images %dx%dx1, %d classes (a 3x3 pattern at a random position), %d ReLU layers, %s"
          % (args.train, args.test, args.hw, args.hw, args.classes, args.layers, args.dtype))
    for method in ("gp", "tp"):
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(args.layers, args.classes, "relu", w_std=w, b_std=b, last_w_std=l),
                            1.4, 0.1, 1.0)
        lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
        model = MultiSPR.from_labels(kernel, lik, x, lab, args.classes, eps=args.eps)
        with model.posterior(capacity=64) as fitted:
            dmean, _ = fitted.predict_grad(xt, var=False)
            acc = fitted.accuracy(xt, labt)
        a = np.abs(np.asarray(dmean.raw_numpy(), dtype=np.float64))[..., 0]           # [T, C, H, W]
        print("%s: test accuracy %.2f %%; share of sum |d mean_k / d x| inside the pattern's window (chance %.3f):"
              % (method, 100.0 * acc, chance))
        for k in range(args.classes):
            rows = np.flatnonzero(labt == k)
            shares = [a[i, k, post[i, 0]:post[i, 0] + 3, post[i, 1]:post[i, 1] + 3].sum() / a[i, k].sum() for i in rows]
            print("    class %d (%3d test images): %.3f" % (k, len(rows), float(np.mean(shares)) if shares else float("nan")))


if __name__ == "__main__":
    main()
