"""Timings of smn_fit_append beside a refit and beside a cov = "full" prediction, for profiles/r22_fit_append.txt.

    python scratch/fit_append_probe.py [--out FILE] [--sizes 16384,4096] [--ks 1,64,2048] [--reps 3]

fp32, d = 3072, 4-layer ReLU MLP, capacity 2048, the state reserved for 2048 more points.  Per N and k, ms per call (median
[min, max] of --reps after one warm-up on a state of its own; host clock around a call that ends in a stream synchronise;
every timed append starts from a fresh state of N points, reserved, so the growth copy is not in it):
    smn_fit_append of k points
    smn_fit_create on N + k points                  (the refit an append replaces)
    smn_fit_predict with cov_d of k rows            (the operation count's expectation: this plus k^3 / 3)
    smn_fit_reserve(N + 2048)                       (the O(N^2) copy, once)
    the splice kernel alone                         (smn_profile_read category 6) against k (n_pad + N) * 4 bytes of HBM traffic
Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, LAYERS, CAP, EXTRA = 3072, 4, 2048, 2048
HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16384,4096")
    ap.add_argument("--ks", default="1,64,2048")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from smnngp import _lib as L
    ctx = L.default_context()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    hyp, eps = (1.0, 0.5, 1.0), 1e-2
    quad, logdet, info = (C.c_double * 1)(), C.c_double(), C.c_int()

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for n in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        x = rng.standard_normal((n + EXTRA, D)).astype(np.float32)
        y = np.sin(x[:, :8].sum(axis=1)).astype(np.float32)
        xd, yd = ctx.to_device(x), ctx.to_device(y)
        xn, yn = C.c_void_p(xd.ptr.value + 4 * n * D), C.c_void_p(yd.ptr.value + 4 * n)
        n_pad = (n + 127) // 128 * 128
        say("== N = %d, d = %d, fp32, %d-layer ReLU, ridge_rel %.0e, capacity %d, reserved for %d more, %d reps (median [min, max] ms)"
            % (n, D, LAYERS, eps, CAP, EXTRA, a.reps))

        def create(rows, reserve=True):
            h = C.c_void_p()
            ctx.call("smn_fit_create", L.F32, L.NET_MLP, L.ACT["relu"], LAYERS, *hyp, xd.ptr, rows, D, D, yd.ptr, 1, eps, 0.0, CAP,
                     C.byref(h), quad, C.byref(logdet), C.byref(info))
            if reserve:
                ctx.call_on("smn_fit_reserve", h, n + EXTRA)
            return h

        def append(h, k):
            ctx.call_on("smn_fit_append", h, xn, k, D, yn, quad, C.byref(logdet), C.byref(info))
            assert info.value == 0, info.value

        h = create(n, reserve=False)
        nbytes = C.c_size_t()
        ctx.call_on("smn_fit_info", h, None, None, None, C.byref(nbytes))
        before = nbytes.value
        t_res = clock(lambda: ctx.call_on("smn_fit_reserve", h, n + EXTRA))
        ctx.call_on("smn_fit_info", h, None, None, None, C.byref(nbytes))
        say("smn_fit_reserve(N + %d)             %8.3f ms once: state %.1f MB -> %.1f MB" % (EXTRA, t_res, before / 1e6, nbytes.value / 1e6))
        ctx.call_on("smn_fit_destroy", h)
        for k in [int(s) for s in a.ks.split(",")]:
            mean, cov = ctx.empty((k, 1), np.float32), ctx.empty((k, k), np.float32)
            t_app, t_fit, t_full = [], [], []
            for rep in range(a.reps + 1):                      # rep 0 warms the workspace up
                h = create(n)
                ms = clock(lambda: append(h, k))
                ctx.call_on("smn_fit_destroy", h)
                hh = []
                ms_fit = clock(lambda: hh.append(create(n + k, reserve=False)))
                ctx.call_on("smn_fit_destroy", hh[0])
                if rep:
                    t_app.append(ms)
                    t_fit.append(ms_fit)
            h = create(n)
            for rep in range(a.reps + 1):
                ms = clock(lambda: ctx.call_on("smn_fit_predict", h, xn, k, D, mean.ptr, None, cov.ptr, k))
                if rep:
                    t_full.append(ms)
            ctx.call("smn_profile_enable", 2 << 6)
            append(h, k)
            ctx.synchronize()
            ms_k, cnt = C.c_double(), C.c_int()
            ctx.call("smn_profile_read", 6, C.byref(ms_k), C.byref(cnt))
            ctx.call("smn_profile_enable", 0)
            ctx.call_on("smn_fit_destroy", h)
            per = ms_k.value / max(cnt.value, 1)
            nb = k * (n_pad + n) * 4
            app, fit, full = stats(t_app), stats(t_fit), stats(t_full)
            say("k = %4d  smn_fit_append %8.3f [%.3f, %.3f]   smn_fit_create(N + k) %8.3f [%.3f, %.3f]   predict cov=full of k rows "
                "%8.3f [%.3f, %.3f]   append / refit = %.3f   append / predict = %.2f"
                % ((k,) + app + fit + full + (app[0] / fit[0], app[0] / full[0])))
            say("          splice kernel alone %.4f ms per launch (%d launch(es)): %.2f MB read + written -> %.2f TB/s, %.0f %% of the "
                "%.0f TB/s HBM peak" % (per, cnt.value, nb / 1e6, nb / (per * 1e-3) / 1e12, 100 * nb / (per * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
