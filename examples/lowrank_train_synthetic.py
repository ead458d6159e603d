#!/usr/bin/env python3
"""Training LowRankSPR with frozen inducing points.  The reference's `syn-t` problem (regression_synthetic.py), gp and tp heads:
two copies of the same rank-M model freeze the greedy pivots, then take k Adam steps side by side -- one by the analytic
gradient (LowRankSPR.loss_and_grad: one factor, one fit and one smn_lowrank_grad per step), one by central differences of the
same frozen loss() (9 evaluations per step for gp, 13 for tp) -- and re-select their pivots every r steps (refresh_pivots()).
Printed per step block: both losses, the largest difference between the two gradients, and the test NLL.

With the pivots frozen loss() is a smooth function of the hyper-parameters, so the two runs follow each other to the accuracy
of the differences; a refresh may move the loss by a jump (a different inducing set is a different model), in both runs alike.
The gradient is that of the frozen objective: how the selection would move with the hyper-parameters is not part of it.

    python examples/lowrank_train_synthetic.py [--rank 16] [--steps 30] [--refresh 10] [--lr 0.03] [--correction fitc]
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
from smnngp.spax.models import LowRankSPR                             # noqa: E402
from regression_synthetic import dataset                              # noqa: E402


def parts(method):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    return kernel, (GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--refresh", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--correction", default="fitc", choices=["fitc", "none"])
    args = ap.parse_args()
    (xtr, ytr), _, (xte, yte), (ym, ys) = dataset("syn-t")
    n = xtr.shape[0]
    r = min(args.rank, n)
    for method in ("gp", "tp"):
        make = lambda: LowRankSPR(*parts(method), xtr, ytr, ym, ys, rank=r, correction=args.correction, eps=args.eps).freeze_pivots()
        analytic, fd = make(), make()
        step_a = train.build_train_step(analytic, method="analytic")
        step_f = train.build_train_step(fd, method="fd", h=1e-5)
        print("%s, syn-t, N = %d, rank %d, %s: analytic gradient beside central differences, pivots refreshed every %d steps"
              % (method, n, r, args.correction, args.refresh))
        print("  [%3d] TEST NLL %.5f" % (0, analytic.test_nll(xte, yte)))
        for i in range(1, args.steps + 1):
            _, ga = analytic.loss_and_grad()
            _, gf = train.value_and_grad_fd(analytic.loss, train.train_vars(analytic), h=1e-5)
            gap = max(abs(ga[k] - gf[k]) for k in ga)
            la, lf = step_a(args.lr), step_f(args.lr)
            note = ""
            if i % args.refresh == 0:
                before = analytic.pivots
                analytic.refresh_pivots(), fd.refresh_pivots()
                note = "  refreshed: %d of %d pivots changed" % (len(set(before) ^ set(analytic.pivots)) // 2, len(before))
            if i % 5 == 0 or note:
                print("  [%3d] loss analytic %.6f  fd %.6f  max |grad - fd| %.2e  TEST NLL %.5f / %.5f%s"
                      % (i, la, lf, gap, analytic.test_nll(xte, yte), fd.test_nll(xte, yte), note))


if __name__ == "__main__":
    main()
