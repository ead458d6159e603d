#!/usr/bin/env python
"""Train where training is cheap, predict exactly: the reference's `syn-t` problem (regression_synthetic.py).  A `LowRankSPR` is
trained (frozen pivots, analytic gradients), its hyper-parameters are handed to `IterativeSPR.from_model`, which solves the EXACT
posterior by preconditioned conjugate gradients on a kernel matrix that is never stored, and the test NLL is printed beside the
low-rank model's and beside an `SPR` (the N x N model) at the same values.  Then the iteration counts with and without the
pivoted-Cholesky preconditioner.

    python examples/matrix_free_synthetic.py [--rank 16] [--steps 40] [--eps 1e-2]

At syn-t's N the dense model is of course the faster one; the matrix-free route is for the N where K does not fit."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from smnngp import nt_kernels, train                                  # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR, IterativeSPR, LowRankSPR          # noqa: E402
from regression_synthetic import dataset                              # noqa: E402


def parts(method):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    return kernel, (GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--tol", type=float, default=1e-8)
    args = ap.parse_args()
    (xtr, ytr), _, (xte, yte), (ym, ys) = dataset("syn-t")
    n = xtr.shape[0]
    rank = min(args.rank, n)
    for method in ("gp", "tp"):
        low = LowRankSPR(*parts(method), xtr, ytr, ym, ys, rank=rank, correction="fitc", eps=args.eps).freeze_pivots()
        step = train.build_train_step(low, method="auto")
        for i in range(1, args.steps + 1):
            step(0.03)
            if i % 10 == 0:
                low.refresh_pivots()
        exact = SPR(low.kernel, low.likelihood, xtr, ytr, ym, ys, eps=low.eps.safe_value)       # the same trainables
        print("%s, syn-t, N = %d, hyper-parameters of a rank-%d LowRankSPR after %d steps:" % (method, n, rank, args.steps))
        print("  TEST NLL   LowRankSPR %.5f   SPR %.5f" % (low.test_nll(xte, yte), exact.test_nll(xte, yte)))
        for r in (rank, 0):
            it = IterativeSPR.from_model(low, rank=r, tol=args.tol)
            nll = it.test_nll(xte, yte)
            sol = it.solve_info
            blocks = [b.iters for b in it.var_info]
            print("  IterativeSPR rank %3d: TEST NLL %.5f   fit: %3d iterations, true residual %.1e   variance blocks: %d solves, "
                  "%d..%d iterations" % (r, nll, sol.iters, float(sol.resid[0]), len(blocks), min(blocks), max(blocks)))


if __name__ == "__main__":
    main()
