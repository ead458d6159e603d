#!/usr/bin/env python3
"""Timing probe for the frozen-pivot LowRankSPR gradient (profiles/r34_lowrank_grad.txt).

    python scratch/lowrank_grad_probe.py [--n 16384] [--d 3072] [--ranks 256,1024] [--reps 3] [--heads gp,tp] [--grad-only]

Per rank and head, on one device, f32, a 4-layer ReLU MLP: (i) one cold loss_and_grad() (factor at the frozen pivots + fit +
smn_lowrank_grad), (ii) one cold loss() on the same frozen model, (iii) one central-difference step through
train.build_train_step(method="fd"), (iv) smn_lowrank_grad alone (lowrank.woodbury_grad on a kept fit).  Each is the median of
--reps runs behind one warm-up; "cold" means the factor cache is dropped first.  --grad-only runs (iv) alone, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/lowrank_grad_probe.py --grad-only --ranks 1024
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smnngp import lowrank, nt_kernels, train                         # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import LowRankSPR                             # noqa: E402


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=3072)
    ap.add_argument("--ranks", default="256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--heads", default="gp,tp")
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--grad-only", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((args.n, args.d), dtype=np.float32)
    y = np.sin(x[:, 0].astype(np.float64)) + 0.1 * rng.standard_normal(args.n)
    make = lambda w, b, l: nt_kernels.get_mlp_kernel(4, act="relu", w_std=w, b_std=b, last_w_std=l)
    for rank in (int(r) for r in args.ranks.split(",")):
        for head in args.heads.split(","):
            lik = GaussianLikelihood() if head == "gp" else StudentTLikelihood(2.0, 2.0)
            model = LowRankSPR(NNGPKernel(make, 1.3, 0.2, 0.9), lik, x, y, 0.0, 1.0, rank=rank, correction="fitc", eps=args.eps)
            t0 = time.perf_counter()
            model.freeze_pivots()
            t_greedy = (time.perf_counter() - t0) * 1e3
            kernel_fn, res, fit = model._fit(False)
            t_grad = timed(lambda: lowrank.woodbury_grad(fit, kernel_fn, model.x_data, 1.0), args.reps)
            tag = "n %d d %d rank %d (made %d) %s f32" % (args.n, args.d, rank, res.rank, head)
            flops = 2.0 * args.n * res.rank * args.d
            print("lrg-probe %s: (iv) smn_lowrank_grad alone %.2f ms  [contraction product 2 n m d = %.3g flop]" % (tag, t_grad, flops))
            if args.grad_only:
                continue

            def cold(f):
                def run():
                    model._factor_cache = None
                    return f()
                return run
            t_lg = timed(cold(model.loss_and_grad), args.reps)
            t_loss = timed(cold(model.loss), args.reps)
            step = train.build_train_step(model, method="fd")
            raw = {k: np.array(v.value) for k, v in model.vars().items()}

            def fd_step():
                for k, v in model.vars().items():
                    v.assign(raw[k])
                model._factor_cache = None
                step(1e-3)
            t_fd = timed(fd_step, max(1, args.reps - 1))
            for k, v in model.vars().items():
                v.assign(raw[k])
            print("lrg-probe %s: greedy freeze %.1f ms  (i) loss_and_grad %.2f ms  (ii) cold loss %.2f ms  (iii) fd step %.1f ms  "
                  "(i)/(ii) %.2f  (iii)/(i) %.2f" % (tag, t_greedy, t_lg, t_loss, t_fd, t_lg / t_loss, t_fd / t_lg))


if __name__ == "__main__":
    main()
