"""Times the pooled conv-NNGP kernel (smn_kernel_cnn_pool) beside the Flatten kernel (smn_kernel_cnn) on the same images:
median of 7 calls after 2 warm-up calls, each call ended by a synchronise.  Rates: entry-layers per second for the pooled
kernel (pairs x (H W)^2 x layers), pixel-layers per second for the Flatten kernel (pairs x H W x layers); their ratio is
the figure of interest.  Also a 1 x N cross call (one test image against N training images).

    python scratch/cnn_pool_probe.py [--big 1000] [--out FILE]      (profiles/r25_cnn_pool.txt keeps one run)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smnngp import _lib as L  # noqa: E402

LAYERS, HYP = 4, (1.0, 0.1, 1.0)


def median_ms(ctx, run, warm=2, reps=7):
    for _ in range(warm):
        run()
    ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ctx.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--big", type=int, default=0, help="also one symmetric build of this many 32x32x3 images (1000: ~10 s per dtype)")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = L.Context(0)
    rng = np.random.default_rng(0)
    say("smn_kernel_cnn_pool beside smn_kernel_cnn, %d ReLU layers, symmetric build, median (min .. max) of 7 calls after 2" % LAYERS)
    for n, h, w, c in ((256, 8, 8, 1), (64, 32, 32, 3)):
        for dt in (np.float32, np.float64):
            x = ctx.to_device(rng.uniform(0, 1, (n, h, w, c)).astype(dt))
            k = ctx.empty((n, n), dt)

            def run(entry):
                ctx.call(entry, L.dtype_code(dt), L.ACT["relu"], LAYERS, *HYP, x.ptr, n, None, 0, h, w, c, L.FILL_FULL, k.ptr, n)

            pairs, pix = n * (n + 1) // 2, h * w
            tp = median_ms(ctx, lambda: run("smn_kernel_cnn_pool"))
            tf = median_ms(ctx, lambda: run("smn_kernel_cnn"))
            rp, rf = pairs * pix * pix * LAYERS / (tp[0] * 1e-3), pairs * pix * LAYERS / (tf[0] * 1e-3)
            say("N=%d %dx%dx%d %s: pooled %.3f ms (%.3f .. %.3f) = %.3g entry-layers/s;  Flatten %.3f ms (%.3f .. %.3f) = %.3g "
                "pixel-layers/s;  rate ratio pooled / Flatten %.2f" % (n, h, w, c, np.dtype(dt).name, tp[0], tp[1], tp[2], rp,
                                                                      tf[0], tf[1], tf[2], rf, rp / rf))
    n, h, w, c = 256, 32, 32, 3
    for dt in (np.float32, np.float64):
        x = ctx.to_device(rng.uniform(0, 1, (n, h, w, c)).astype(dt))
        xt = ctx.to_device(rng.uniform(0, 1, (1, h, w, c)).astype(dt))
        k = ctx.empty((1, n), dt)
        tp = median_ms(ctx, lambda: ctx.call("smn_kernel_cnn_pool", L.dtype_code(dt), L.ACT["relu"], LAYERS, *HYP, xt.ptr, 1, x.ptr, n,
                                             h, w, c, L.FILL_FULL, k.ptr, n))
        say("1 x %d cross call %dx%dx%d %s: %.3f ms (%.3f .. %.3f) = %.3g entry-layers/s" % (
            n, h, w, c, np.dtype(dt).name, tp[0], tp[1], tp[2], n * (h * w) ** 2 * LAYERS / (tp[0] * 1e-3)))
    if args.big:
        n = args.big
        for dt in (np.float32, np.float64):
            x = ctx.to_device(rng.uniform(0, 1, (n, h, w, c)).astype(dt))
            k = ctx.empty((n, n), dt)
            pairs, pix = n * (n + 1) // 2, h * w
            res = {}
            for entry in ("smn_kernel_cnn_pool", "smn_kernel_cnn"):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.call(entry, L.dtype_code(dt), L.ACT["relu"], LAYERS, *HYP, x.ptr, n, None, 0, h, w, c, L.FILL_FULL, k.ptr, n)
                ctx.synchronize()
                res[entry] = time.perf_counter() - t0
            say("N=%d %dx%dx%d %s, ONE call each (kernels warm from the runs above): pooled %.3f s = %.3g entry-layers/s;  Flatten "
                "%.1f ms = %.3g pixel-layers/s;  rate ratio %.2f" % (
                    n, h, w, c, np.dtype(dt).name, res["smn_kernel_cnn_pool"], pairs * pix * pix * LAYERS / res["smn_kernel_cnn_pool"],
                    1e3 * res["smn_kernel_cnn"], pairs * pix * LAYERS / res["smn_kernel_cnn"],
                    (pairs * pix * pix * LAYERS / res["smn_kernel_cnn_pool"]) / (pairs * pix * LAYERS / res["smn_kernel_cnn"])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
