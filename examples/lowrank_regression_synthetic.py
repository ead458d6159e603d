#!/usr/bin/env python3
"""How much rank does the regression need?  The reference's `syn-t` problem (regression_synthetic.py), gp and tp heads: SPR is
trained for a few steps, then LowRankSPR -- the same model on the rank-M greedy pivoted-Cholesky factor, K^ = L L^T + diag(resid)
("fitc") or K^ = L L^T ("none"), evaluated by the Woodbury identity without the N x N matrix -- is put at the same
hyper-parameters for a sweep of ranks: training loss and test NLL beside SPR's.  Last, a LowRankSPR is trained by itself
(central differences: train.build_train_step(method="auto")) at one rank.

The losses and the Gaussian test NLL converge to SPR's as the rank grows.  The Student-t test NLL does not: LowRankSPR takes
its quadratic form from its own fit, y^T (scale (K^ + lam I))^-1 y (LowRankSPR's docstring), SPR from the reference's separate
matrix scale K + 1e-6 I, which on this data is a much larger number (hence a wider predictive law) at any rank.

    python examples/lowrank_regression_synthetic.py [--ranks 2,4,8,16,32,64] [--steps 60] [--train-rank 16] [--lowrank-steps 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from smnngp import nt_kernels, train                                  # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR, LowRankSPR                        # noqa: E402
from regression_synthetic import dataset                              # noqa: E402


def parts(method):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    return kernel, (GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0))


def copy_vars(src, dst):
    """The trainables of one model into another of the same structure: names agree up to the class name in front."""
    tail = lambda k: k.split(").", 1)[1]
    values = {tail(k): v.value for k, v in src.vars().items()}
    for k, v in dst.vars().items():
        v.assign(values[tail(k)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ranks", default="2,4,8,16,32,64")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--train-rank", type=int, default=16)
    ap.add_argument("--lowrank-steps", type=int, default=20)
    ap.add_argument("--eps", type=float, default=1e-2)
    args = ap.parse_args()
    (xtr, ytr), _, (xte, yte), (ym, ys) = dataset("syn-t")
    n = xtr.shape[0]
    ranks = [r for r in (int(v) for v in args.ranks.split(",")) if 1 <= r <= n]
    for method in ("gp", "tp"):
        exact = SPR(*parts(method), xtr, ytr, ym, ys, eps=args.eps)
        step = train.build_train_step(exact)
        for _ in range(args.steps):
            step(0.03)
        print("%s, syn-t, N = %d: SPR after %d steps  loss %.5f  TEST NLL %.5f" % (method, n, args.steps, exact.loss(),
                                                                                  exact.test_nll(xte, yte)))
        print("  rank made   trace left   fitc: loss   TEST NLL    none: loss   TEST NLL")
        for r in ranks:
            row = []
            for correction in ("fitc", "none"):
                model = LowRankSPR(*parts(method), xtr, ytr, ym, ys, rank=r, correction=correction, eps=args.eps)
                copy_vars(exact, model)
                row += [model.loss(), model.test_nll(xte, yte)]
            res = model._factor()[1]
            print("  %4d %4d   %.3e   %12.5f %10.5f   %12.5f %10.5f" % (r, res.rank, res.trace[-1] / res.trace[0], *row))
    r = min(args.train_rank, n)
    model = LowRankSPR(*parts("tp"), xtr, ytr, ym, ys, rank=r, correction="fitc", eps=args.eps)
    step = train.build_train_step(model, method="auto")              # no analytic gradient: central differences
    print("LowRankSPR (tp, fitc, rank %d) trained by central differences:" % r)
    print("  [%3d] TEST NLL %.5f" % (0, model.test_nll(xte, yte)))
    for i in range(1, args.lowrank_steps + 1):
        loss = step(0.03)
        if i % 5 == 0:
            print("  [%3d] loss %.5f  TEST NLL %.5f" % (i, loss, model.test_nll(xte, yte)))


if __name__ == "__main__":
    main()
