#!/usr/bin/env python3
"""Which inducing images?  On the synthetic image problem of train_classify_synthetic.py (class templates plus noise) a sparse
variational classifier (SVSP, svgp) is trained twice for the same few epochs: once with the FIRST M training images as its
(fixed) inducing images, once with the M images that the greedy pivoted Cholesky of K(train, train) picks
(SVSP.from_greedy: largest conditional variance first; the N x N matrix is never formed).  Prints, for both, the mean nELBO of
every epoch, validation NLL and accuracy, and the trace decay tr(K - L L^T) / tr(K) against the rank: the share of the prior
variance of the training set that M inducing images leave unexplained, greedy against first-M.

    python examples/greedy_inducing_synthetic.py [--train 1024] [--valid 512] [--inducing 32] [--hw 8] [--classes 4]
                                                 [--epochs 4] [--batch 64] [--samples 32] [--lr 1e-2]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from smnngp import lowrank, nt_kernels, train_svsp                    # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.models import SVSP                                   # noqa: E402
from smnngp.spax.priors import GaussianPrior                          # noqa: E402
from train_classify_synthetic import build, problem                   # noqa: E402


def first_m_trace(kernel_fn, x, m):
    """tr(K - K[:, Z] K[Z, Z]^-1 K[Z, :]) for Z = the first m rows, from the diagonal and m rows of K (fp64, host)."""
    diag = np.asarray(kernel_fn.diag(x).raw_numpy(), dtype=np.float64)
    kzx = np.asarray(kernel_fn(x[:m], x).raw_numpy(), dtype=np.float64)
    out = [diag.sum()]
    for r in range(1, m + 1):
        c = np.linalg.cholesky(kzx[:r, :r] + 1e-12 * np.eye(r) * diag.max())
        out.append(float(np.maximum(diag - np.sum(np.linalg.solve(c, kzx[:r]) ** 2, axis=0), 0.0).sum()))
    return np.asarray(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train", type=int, default=1024)
    ap.add_argument("--valid", type=int, default=512)
    ap.add_argument("--inducing", type=int, default=32)
    ap.add_argument("--hw", type=int, default=8)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--eval-samples", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--eps", type=float, default=1e-3)
    args = ap.parse_args()
    xt, yt, xv, yv = problem(args.train, args.valid, args.classes, args.hw, args.channels)
    m = args.inducing
    first = build("svgp", xt[:m].copy(), args.classes, args.layers, np.float64, args.eps)
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(args.layers, args.classes, "relu", w_std=w, b_std=b, last_w_std=l),
                        1.2, 0.1, 1.0)                                               # build()'s kernel, with its own trainables
    greedy = SVSP.from_greedy(GaussianPrior(), kernel, xt, m, num_latent_gps=args.classes, eps=args.eps)
    kernel_fn = first.kernel.get_kernel_fn()

    res = lowrank.pivoted_cholesky(kernel_fn, xt, m)
    tf = first_m_trace(kernel_fn, xt, m)
    print("trace left out, tr(K - L L^T) / tr(K), %d training images %dx%dx%d:" % (args.train, args.hw, args.hw, args.channels))
    print("  rank   greedy    first-M")
    for r in sorted(set([0, 1, 2, 4, 8, 16, 32, 64, 128, m]) & set(range(m + 1))):
        print("  %4d   %.5f   %.5f" % (r, res.trace[min(r, res.rank)] / res.trace[0], tf[r] / tf[0]))
    print("  greedy pivots (first 12): %s;  classes of all %d: %s" % (res.pivots[:12].tolist(), res.rank,
                                                                      np.bincount(yt[res.pivots], minlength=args.classes).tolist()))

    for name, model in (("first-M", first), ("greedy", greedy)):
        step = train_svsp.build_svsp_train_step(model, train_svsp.svsp_train_vars(model, inducing=False), num_train=args.train,
                                                num_samples=args.samples)
        sched = train_svsp.PlateauSchedule(args.lr)
        nll0, acc0 = model.evaluate(xv, yv, args.eval_samples)
        print("%s inducing images (M = %d, fixed):" % (name, m))
        print("  before: validation NLL %.5f  ACC %.2f" % (nll0, acc0))
        for e in range(args.epochs):
            nelbo = train_svsp.train_epoch(step, xt, yt, args.batch, sched.lr, seed=1, epoch=e)
            nll, acc = train_svsp.valid_epoch(model, xv, yv, args.eval_samples, schedule=sched)
            print("  epoch %2d  nELBO %.5f  validation NLL %.5f  ACC %.2f" % (e, nelbo, nll, acc))


if __name__ == "__main__":
    main()
