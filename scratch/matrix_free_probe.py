"""Timings of the matrix-free product and of IterativeSPR.fit (f32, d = 3072, 4-layer ReLU MLP) for profiles/r35_matrix_free.txt.

    python scratch/matrix_free_probe.py matmul 16384        smn_kernel_mlp_matmul, t = 1 / 16 / 48, beside smn_kernel_mlp (full)
    python scratch/matrix_free_probe.py fit 16384 256       one IterativeSPR.fit (eps = 1e-2), beside SPR.predict when N <= 16384
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from smnngp import lowrank, nt_kernels                                     # noqa: E402
from smnngp._lib import default_context                                    # noqa: E402


def timed(ctx, f, reps=3):
    f()
    ctx.synchronize()
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ctx.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    what, n = sys.argv[1], int(sys.argv[2])
    d = 3072
    ctx = default_context()
    rng = np.random.default_rng(0)
    x = ctx.to_device(rng.standard_normal((n, d)).astype(np.float32))
    kfn = nt_kernels.get_mlp_kernel(4, act="relu", w_std=1.3, b_std=0.2, last_w_std=0.9)
    if what == "matmul":
        build = timed(ctx, lambda: kfn(x, None, get="nngp"))
        print("smn_kernel_mlp full  N=%d: %.2f ms" % (n, build))
        for t in (1, 16, 48):
            v = ctx.to_device(rng.standard_normal((n, t)).astype(np.float32))
            ms = timed(ctx, lambda: lowrank.kernel_matmul(kfn, x, None, v))
            print("smn_kernel_mlp_matmul N=%d t=%2d: %.2f ms  (%.2fx the full build)" % (n, t, ms, ms / build))
    else:
        from smnngp.spax.kernels import NNGPKernel
        from smnngp.spax.likelihoods import GaussianLikelihood
        from smnngp.spax.models import SPR, IterativeSPR
        rank = int(sys.argv[3])
        y = rng.standard_normal(n)
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(4, act="relu", w_std=w, b_std=b, last_w_std=l), 1.3, 0.2, 0.9)
        model = IterativeSPR(kernel, GaussianLikelihood(), x, y, 0.0, 1.0, rank=rank, eps=1e-2)
        t0 = time.perf_counter()
        sol = model.fit()
        ctx.synchronize()
        print("IterativeSPR.fit N=%d rank=%d eps=1e-2: %.3f s, %d iterations, info %d, true residual %.2e" %
              (n, rank, time.perf_counter() - t0, sol.iters, sol.info, float(sol.resid[0])))
        if n <= 16384:
            spr = SPR(kernel, GaussianLikelihood(), x, y, 0.0, 1.0, eps=1e-2)
            xt = ctx.to_device(rng.standard_normal((256, d)).astype(np.float32))
            print("SPR.predict (256 points) N=%d: %.2f ms" % (n, timed(ctx, lambda: spr.predict(xt))))


if __name__ == "__main__":
    main()
