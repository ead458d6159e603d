"""Timings of smn_fit_remove beside the refit it replaces, for profiles/r23_fit_remove.txt.

    python scratch/fit_remove_probe.py [--out FILE] [--sizes 16384,4096] [--ks 1,64,33] [--reps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/fit_remove_probe.py --once --sizes 16384 --ks 33

fp32, d = 3072, 4-layer ReLU MLP, capacity 2048.  Per N and k, ms per call (median [min, max] of --reps after one warm-up; host
clock around a call that ends in a stream synchronise; every timed removal starts from a fresh state of N points):
    smn_fit_remove of the k OLDEST points     (the worst case: the window is the whole factor; k = KMAX + 1 = 33 is two passes)
    smn_fit_remove of the k NEWEST points     (the suffix path: no arithmetic touches L)
    smn_fit_create on the N - k kept points   (the refit a removal replaces)
--once: one removal of the k oldest points per size and nothing else, for a kernel trace (the panel and apply kernels are
remove_panel_kernel / remove_apply_kernel).  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, LAYERS, CAP = 3072, 4, 2048


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16384,4096")
    ap.add_argument("--ks", default="1,64,33")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
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
        x = rng.standard_normal((n, D)).astype(np.float32)
        y = np.sin(x[:, :8].sum(axis=1)).astype(np.float32)
        xd, yd = ctx.to_device(x), ctx.to_device(y)
        say("== N = %d, d = %d, fp32, %d-layer ReLU, ridge_rel %.0e, capacity %d, %d reps (median [min, max] ms)"
            % (n, D, LAYERS, eps, CAP, a.reps))

        def create(rows, first=0, **ridge):
            h = C.c_void_p()
            ctx.call("smn_fit_create", L.F32, L.NET_MLP, L.ACT["relu"], LAYERS, *hyp, C.c_void_p(xd.ptr.value + 4 * first * D), rows, D, D,
                     C.c_void_p(yd.ptr.value + 4 * first), 1, ridge.get("rel", eps), ridge.get("abs", 0.0), CAP, C.byref(h), quad,
                     C.byref(logdet), C.byref(info))
            assert info.value == 0, info.value
            return h

        def remove(h, idx):
            arr = (C.c_int64 * len(idx))(*idx)
            ctx.call_on("smn_fit_remove", h, arr, len(idx), quad, C.byref(logdet))

        for k in [int(s) for s in a.ks.split(",")]:
            if a.once:
                h = create(n)
                ms = clock(lambda: remove(h, list(range(k))))
                say("k = %4d  one smn_fit_remove of the oldest: %.3f ms" % (k, ms))
                ctx.call_on("smn_fit_destroy", h)
                continue
            t_old, t_new, t_fit = [], [], []
            for rep in range(a.reps + 1):                      # rep 0 warms the workspace up
                h = create(n)
                lam = C.c_double()
                ctx.call_on("smn_fit_stats", h, None, C.byref(lam), None, None)
                ms_old = clock(lambda: remove(h, list(range(k))))
                ld_removed = logdet.value
                ctx.call_on("smn_fit_destroy", h)
                h = create(n)
                ms_new = clock(lambda: remove(h, list(range(n - k, n))))
                ctx.call_on("smn_fit_destroy", h)
                hh = []
                ms_fit = clock(lambda: hh.append(create(n - k, first=k, rel=0.0, abs=lam.value)))     # the kept points, the frozen ridge
                ld_fresh = logdet.value
                ctx.call_on("smn_fit_destroy", hh[0])
                if rep:
                    t_old.append(ms_old)
                    t_new.append(ms_new)
                    t_fit.append(ms_fit)
            old, new, fit = stats(t_old), stats(t_new), stats(t_fit)
            say("k = %4d  remove oldest %9.3f [%.3f, %.3f]   remove newest %8.3f [%.3f, %.3f]   smn_fit_create(N - k) %9.3f [%.3f, %.3f]   "
                "oldest / refit = %.3f   newest / refit = %.4f   (logdet removed %.9g, refit %.9g)"
                % ((k,) + old + new + fit + (old[0] / fit[0], new[0] / fit[0], ld_removed, ld_fresh)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
