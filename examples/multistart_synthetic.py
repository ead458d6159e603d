#!/usr/bin/env python3
"""Multi-start training of the reference's regression model on its offline `syn-t` data set: G initialisations drawn
around the reference's defaults are trained side by side, one batched device call per step
(train.build_multistart_step -> smn_spr_loss_grad_batch), and the best one is evaluated on the test split.

    python examples/multistart_synthetic.py [--starts 16] [--steps 100] [--method tp|gp] [--dtype float64|float32]
    python examples/multistart_synthetic.py --time [--out FILE]     # batched call against G serial calls, table to FILE
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from regression_synthetic import dataset                              # noqa: E402
from smnngp import _lib, nt_kernels, train                    # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR                                    # noqa: E402


def run(args):
    (xtr, ytr), (xva, yva), (xte, yte), (ym, ys) = dataset("syn-t")
    dtype = np.dtype(args.dtype).type
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    likelihood = GaussianLikelihood() if args.method == "gp" else StudentTLikelihood(2.0, 2.0)
    model = SPR(kernel, likelihood, xtr.astype(dtype), ytr.astype(dtype), ym, ys, eps=1e-2)
    rng = np.random.default_rng(args.seed)
    # start 0 is the reference's own initialisation; the others are drawn around it in raw (softplus-inverse) space
    starts = {k: float(v.value) + np.concatenate([[0.0], 0.7 * rng.standard_normal(args.starts - 1)]) for k, v in model.vars().items()}
    step = train.build_multistart_step(model, starts)
    t0 = time.perf_counter()
    for i in range(1, args.steps + 1):
        losses = step(args.lr)
        if i % max(1, args.steps // 5) == 0:
            print("[%5d] best %.5f  median %.5f  not PD: %d" % (i, np.nanmin(losses), np.nanmedian(losses), int(np.isnan(losses).sum())))
    dt = time.perf_counter() - t0
    print("%d starts x %d steps in %.2f s (%.2f ms per step)" % (args.starts, args.steps, dt, 1e3 * dt / args.steps))
    for s, v in enumerate(step.losses):
        print("  start %3d  loss %.5f%s" % (s, v, "   <- reference initialisation" if s == 0 else ""))
    best = step.assign_best()
    ws, bs, ls = kernel.get_params()
    print("best start %d: loss %.5f  ws %.4f  bs %.3E  ls %.4f  e %.3E" % (best, step.losses[best], ws, bs, ls, model.eps.safe_value))
    print("valid NLL %.5f  TEST NLL %.5f" % (model.test_nll(xva, yva), model.test_nll(xte, yte)))


def timing(args):
    """One batched call (median of `reps` runs after warm-up) against G serial smn_spr_loss_grad calls in the same process
    (three repetitions: median and spread), per shape, dtype and G.  Times are host wall clock around the synchronous calls."""
    ctx = _lib.default_context()
    shapes = [(245, 6, np.float32), (245, 6, np.float64), (1000, 8, np.float32), (1000, 8, np.float64), (2048, 8, np.float32)]
    layers, reps = 2, args.reps
    lines = ["# smn_spr_loss_grad_batch against G serial smn_spr_loss_grad calls (MLP, relu, %d hidden layers, Student-t head)" % layers,
             "# batched: median of %d calls after 3 warm-up calls; serial: G calls timed together, 3 repetitions (median, spread = max - min)" % reps,
             "# us per problem.  pass: batched < serial - spread (G >= 16, N = 245); G = 1: batched <= serial + spread",
             "%6s %3s %8s %4s %14s %14s %12s %8s" % ("N", "d", "dtype", "G", "batched us/pb", "serial us/pb", "spread us/pb", "ratio")]
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms = (C.c_double * 4)()
    for n, d, dtype in shapes:
        rng = np.random.default_rng(n)
        x = ctx.to_device(rng.standard_normal((n, d)).astype(dtype))
        y = ctx.to_device(rng.standard_normal((n, 1)).astype(dtype))
        for g in (1, 16, 64, 256):
            w = 1.0 + 0.3 * rng.random(g); b = 0.1 + 0.5 * rng.random(g); lw = 0.8 + 0.4 * rng.random(g)
            eps = 1e-2 * (1.0 + rng.random(g)); df = np.full(g, 4.0); sc = np.full(g, 1.0)
            pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))             # noqa: E731
            bq, bl, bt, bi = np.empty(g), np.empty(g), np.empty((g, 4)), np.zeros(g, dtype=np.int32)

            def serial():
                for i in range(g):
                    ctx.call("smn_spr_loss_grad", x.dcode, _lib.NET_MLP, _lib.ACT["relu"], layers, w[i], b[i], lw[i], x.ptr, n, d, d,
                             y.ptr, eps[i], df[i], sc[i], C.byref(quad), C.byref(logdet), C.byref(info), terms)

            def clock(fn):
                t0 = time.perf_counter()
                fn()
                return time.perf_counter() - t0

            def batched():                                                     # the C call itself, as the serial side is timed
                ctx.call("smn_spr_loss_grad_batch", x.dcode, _lib.NET_MLP, _lib.ACT["relu"], layers, g, pd(w), pd(b), pd(lw), x.ptr, n,
                         d, d, y.ptr, pd(eps), pd(df), pd(sc), pd(bq), pd(bl), bi.ctypes.data_as(C.POINTER(C.c_int)), pd(bt))

            for _ in range(3):
                batched()
            tb = np.median([clock(batched) for _ in range(reps)]) / g
            serial()
            ts = np.array([clock(serial) for _ in range(3)]) / g
            assert not bi.any() and np.isfinite(bt).all(), "a timing problem was not positive definite"
            lines.append("%6d %3d %8s %4d %14.2f %14.2f %12.2f %8.2f" % (n, d, np.dtype(dtype).name, g, 1e6 * tb, 1e6 * np.median(ts),
                                                                        1e6 * (ts.max() - ts.min()), np.median(ts) / tb))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--starts", type=int, default=16)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--lr", type=float, default=0.03)
    p.add_argument("--method", choices=("gp", "tp"), default="tp")
    p.add_argument("--dtype", choices=("float64", "float32"), default="float64")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--time", action="store_true", help="time the batched call against serial calls instead of training")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--out", default=None, help="--time: write the table to this file")
    args = p.parse_args()
    if args.starts < 1:
        p.error("--starts must be >= 1")
    timing(args) if args.time else run(args)


if __name__ == "__main__":
    main()
