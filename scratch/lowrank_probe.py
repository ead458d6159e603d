"""Timing of the regression on the pivoted-Cholesky factor (csrc/lowrank.hip; no thresholds).

  1. smn_lowrank_gram (G alone, unit weights) in f32 and f64 at (N, M) = (16384, 256), (16384, 1024), (262144, 256),
     (262144, 1024), beside the route that existed before it: smn_transpose into a second buffer + smn_gram (the NT tile
     engine, one accumulator over all N rows) on the same matrix.  Device events around `reps` calls.
  2. LowRankSPR.loss and a 2048-point test_nll at N = 16384, d = 3072, f32, rank 256 / 1024, and their pieces.

    python scratch/lowrank_probe.py [gram|model]     # from the repository root; the numbers of profiles/r32_lowrank_gp.txt
"""
import ctypes as C
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smnngp import lowrank, nt_kernels as nt, _lib

F32_MFMA_PEAK, F64_MFMA_PEAK, HBM_PEAK = 157.3e12, 78.6e12, 8.0e12   # flop/s, flop/s, bytes/s (MI355X_MICROARCH.md)


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


ctx = _lib.default_context()


def device_ms(f, reps):
    f(); ctx.synchronize()
    ms = C.c_double()
    ctx.call("smn_timer_start")
    for _ in range(reps):
        f()
    ctx.call("smn_timer_stop_ms", C.byref(ms))
    return ms.value / reps


def wall_ms(f, reps=3):
    ts = []
    for _ in range(reps):
        ctx.synchronize(); t0 = time.perf_counter(); r = f(); ctx.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return r, min(ts), sorted(ts)[len(ts) // 2]


def gram_part():
    rng = np.random.default_rng(0)
    for n, m in ((16384, 256), (16384, 1024), (262144, 256), (262144, 1024)):
        host = rng.standard_normal((n, m), dtype=np.float32)
        for dt in (np.float32, np.float64):
            Ld = ctx.to_device(host.astype(dt))
            G = ctx.empty((m, m), np.float64)
            code, es = Ld.dcode, np.dtype(dt).itemsize
            reps = 20 if n * m <= 2 ** 24 else 5
            new = device_ms(lambda: ctx.call("smn_lowrank_gram", code, Ld.ptr, n, m, m, None, None, 0, 1, G.ptr, m, None, None), reps)
            flop, peak = 2.0 * n * m * m, (F32_MFMA_PEAK if dt == np.float32 else F64_MFMA_PEAK)
            lower = flop * (m / (32 * (16 // es)) + 1) / (2 * m / (32 * (16 // es)))          # the block pairs a >= b only
            say("gram  N=%d M=%d %s: smn_lowrank_gram %.3f ms; 2NM^2 = %.3g flop -> %.1f TF/s nominal = %.1f%% of the MFMA peak "
                "(%.1f%% counting the computed lower blocks only); L = %.1f MB -> %.2f TB/s if read once"
                % (n, m, np.dtype(dt).name, new, flop, flop / new / 1e9, flop / new / 1e9 / (peak / 1e12) * 100,
                   lower / new / 1e9 / (peak / 1e12) * 100, n * m * es / 1e6, n * m * es / new / 1e9))
            try:
                Lt, K0, q = ctx.empty((m, n), dt), ctx.empty((m, m), dt), ctx.empty((m,), dt)
                tr = device_ms(lambda: ctx.call("smn_transpose", code, Lt.ptr, n, Ld.ptr, m, n, m), reps)
                nt_ms = device_ms(lambda: ctx.call("smn_gram", code, Lt.ptr, m, n, None, 0, 0, n, K0.ptr, m, q.ptr, None), reps)
                got = np.asarray(K0.raw_numpy(), dtype=np.float64) * n
                err = float(np.abs(got - G.raw_numpy()).max() / np.abs(got).max())
                say("      transpose route: smn_transpose %.3f ms + smn_gram %.3f ms = %.3f ms (%.2f x smn_lowrank_gram); "
                    "results differ by %.2e of the largest entry" % (tr, nt_ms, tr + nt_ms, (tr + nt_ms) / new, err))
                del Lt, K0, q
            except _lib.SmnError as e:
                say("      transpose route: not run (%s)" % e)
            del Ld, G


def gen(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d), dtype=np.float32) * np.exp(0.5 * rng.standard_normal((n, 1))).astype(np.float32)


def model_part():
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import LowRankSPR
    n, d, t = 16384, 3072, 2048
    x, xt = gen(n, d), gen(t, d, seed=1)
    rng = np.random.default_rng(2)
    y, yt = np.sin(x[:, 0]) + 0.1 * rng.standard_normal(n), np.sin(xt[:, 0])
    xd = ctx.to_device(x)
    for m in (256, 1024):
        kernel = NNGPKernel(lambda w, b, l: nt.get_mlp_kernel(4, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1e-4, 1.0)
        model = LowRankSPR(kernel, GaussianLikelihood(), xd, y, 0.0, 1.0, rank=m, correction="fitc", eps=1e-2)
        model.loss(); model.test_nll(xt, yt)                     # warm-up: code objects, workspaces
        res = model._factor()[1]
        _, fit_ms, _ = wall_ms(lambda: lowrank.woodbury_fit(res, y, 1e-2, True))

        def cold_loss():
            model._factor_cache = None
            return model.loss()

        def nll_after_loss():
            model._factor_cache[2].clear()
            return model.test_nll(xt, yt)

        loss, cold, cold_med = wall_ms(cold_loss)
        nll, pred, pred_med = wall_ms(nll_after_loss)
        fit = model._fit(True)[2]
        kzt = lowrank.kernel_cross(model.kernel.get_kernel_fn(), res._z, ctx.to_device(xt))
        ktt = ctx.to_device(np.ones(t, dtype=np.float32))
        ro = device_ms(lambda: fit.readout(kzt, ktt), 5)
        say("model N=%d d=%d f32 rank=%d fitc: loss() with the factor remade %.2f ms (median %.2f; woodbury_fit alone %.2f ms, the "
            "rest is pivoted_cholesky); test_nll on %d points with the factor kept %.2f ms (median %.2f; smn_lowrank_readout alone "
            "%.2f ms); loss %.6f nll %.6f rank made %d" % (n, d, m, cold, cold_med, fit_ms, t, pred, pred_med, ro, loss, nll, res.rank))


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("gram", "all"):
        gram_part()
    if which in ("model", "all"):
        model_part()
