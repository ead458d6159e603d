"""Timing of the greedy pivoted Cholesky (lowrank.pivoted_cholesky; no thresholds): the fused and the matrix route at the benchmark
shape (N = 16384, d = 3072, f32, 4-layer ReLU MLP), and the fused route at N = 262144, where K(X, X) would be 275 GB.

    python scratch/pchol_probe.py        # from the repository root; the numbers of profiles/r30_pchol.txt
"""
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smnngp import lowrank, nt_kernels as nt, _lib

def say(*a):
    print(" ".join(str(x) for x in a), flush=True)

ctx = _lib.default_context()
fn = nt.get_mlp_kernel(4, act="relu", w_std=1.0, b_std=1e-8, last_w_std=1.0)
def gen(n, d, seed=0):
    rng = np.random.default_rng(seed)
    x = np.empty((n, d), dtype=np.float32)
    for a in range(0, n, 16384):
        b = min(n, a + 16384)
        x[a:b] = rng.standard_normal((b - a, d), dtype=np.float32) * np.exp(0.5 * rng.standard_normal((b - a, 1))).astype(np.float32)
    return x

def timed(f, reps=3):
    ts = []
    for _ in range(reps):
        ctx.synchronize(); t0 = time.perf_counter(); r = f(); ctx.synchronize(); ts.append(time.perf_counter() - t0)
    return r, min(ts), sorted(ts)[len(ts) // 2]

n, d = 16384, 3072
xd = ctx.to_device(gen(n, d))
lowrank.pivoted_cholesky(fn, xd, 8)                       # warm-up (module load, workspace)
xbytes = n * d * 4
for m in (256, 1024):
    r, tmin, tmed = timed(lambda: lowrank.pivoted_cholesky(fn, xd, m, route="fused"))
    lbytes = n * 4 * (m - 1) / 2.0                        # mean read of L per step
    say("fused  N=%d d=%d f32 rank=%d: total min %.2f ms median %.2f ms, per step %.4f ms, (X + mean L read)/step = %.1f MB -> %.2f TB/s = %.1f%% of 8 TB/s; rank made %d, trace left %.3e of %.3e"
        % (n, d, m, tmin * 1e3, tmed * 1e3, tmin * 1e3 / m, (xbytes + lbytes) / 1e6, (xbytes + lbytes) * m / tmin / 1e12,
           (xbytes + lbytes) * m / tmin / 8e12 * 100, r.rank, r.trace[-1], r.trace[0]))
lowrank.pivoted_cholesky(fn, xd, 4, route="matrix")
for m in (256, 1024):
    r, tmin, tmed = timed(lambda: lowrank.pivoted_cholesky(fn, xd, m, route="matrix"), reps=2)
    say("matrix N=%d d=%d f32 rank=%d: total min %.2f ms median %.2f ms, per step %.4f ms (includes the diagonal from %d block builds); rank made %d"
        % (n, d, m, tmin * 1e3, tmed * 1e3, tmin * 1e3 / m, (n + 255) // 256, r.rank))
del xd
n = 262144
t0 = time.perf_counter(); xh = gen(n, d, seed=1); say("host data N=%d: %.1f s" % (n, time.perf_counter() - t0))
xd = ctx.to_device(xh); del xh
m = 256
lowrank.pivoted_cholesky(fn, xd, 2)
r, tmin, tmed = timed(lambda: lowrank.pivoted_cholesky(fn, xd, m, route="fused"), reps=2)
xbytes = n * d * 4
say("fused  N=%d d=%d f32 rank=%d (dense K would be %.0f GB): total min %.2f ms, per step %.4f ms, X/step = %.0f MB -> %.2f TB/s = %.1f%% of 8 TB/s; rank made %d"
    % (n, d, m, n * n * 4 / 1e9, tmin * 1e3, tmin * 1e3 / m, xbytes / 1e6, xbytes * m / tmin / 1e12, xbytes * m / tmin / 8e12 * 100, r.rank))
