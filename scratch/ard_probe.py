"""smn_spr_loss_grad_inputs (loss_and_grad under input scales, d loss / d X) against smn_spr_loss_grad_multi on the same data;
kernel-level times of the two-sided pass and of the contraction from the seeded entry alone.

    python scratch/ard_probe.py [N D dtype] ...      default: 4096 3072 f32, 16384 3072 f32, 8192 3072 f64
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smnngp import _lib as L  # noqa: E402

ctx = L.default_context()
LAYERS, W, B, LW, EPS = 4, 1.3, 0.2, 1.0, 1e-2
PEAK = {np.float32: 157.3, np.float64: 78.6}    # TFLOP/s, dense MFMA (datasheet)
rng = np.random.default_rng(0)


def timed(fn, reps):
    fn(); ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ctx.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def prof(cat):
    ms, n = C.c_double(), C.c_int()
    ctx.call("smn_profile_read", cat, C.byref(ms), C.byref(n))
    return ms.value, n.value


def run(n, d, dtype):
    code = L.dtype_code(dtype)
    x = ctx.to_device(rng.standard_normal((n, d)).astype(dtype))
    y = ctx.to_device(rng.standard_normal((n, 1)).astype(dtype))
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms, cols, feat = (C.c_double * 4)(), (C.c_double * 1)(), np.zeros(d)
    head = (code, 0, 0, LAYERS, W, B, LW, x.ptr, n, d, d, y.ptr, 1, EPS, 0.0, 1.0, C.byref(quad), cols, C.byref(logdet), C.byref(info), terms)
    pf = feat.ctypes.data_as(C.POINTER(C.c_double))
    gx = ctx.empty((n, d), dtype)
    base = lambda: ctx.call("smn_spr_loss_grad_multi", *head)                                  # noqa: E731
    ard = lambda: ctx.call("smn_spr_loss_grad_inputs", *head, None, 0, pf)                     # noqa: E731
    dx = lambda: ctx.call("smn_spr_loss_grad_inputs", *head, gx.ptr, d, None)                  # noqa: E731
    reps = 3
    tb, ta, tx = timed(base, reps), timed(ard, reps), timed(dx, reps)
    name = np.dtype(dtype).name
    print("N=%d d=%d %s info=%d | smn_spr_loss_grad_multi min %.2f med %.2f ms | _inputs (feat) min %.2f med %.2f ms, ratio %.2f | "
          "_inputs (gx) min %.2f med %.2f ms, ratio %.2f" % (n, d, name, info.value, tb[0], tb[1], ta[0], ta[1], ta[0] / tb[0], tx[0],
                                                              tx[1], tx[0] / tb[0]), flush=True)
    # kernel level: the seeded entry alone on smn_spr_kinv's outputs (category 6: the pass; 5: the contraction; 1: its Gram build)
    ld = (n + 3) // 4 * 4
    ninv, alpha = ctx.empty((n, ld), dtype), ctx.empty((n, 1), dtype)
    ctx.call("smn_spr_kinv", code, 0, 0, LAYERS, W, B, LW, x.ptr, n, d, d, y.ptr, 1, EPS, ninv.ptr, ld, alpha.ptr, None, None)
    sym = lambda: ctx.call("smn_kernel_mlp_input_grad_sym", code, 0, 0, LAYERS, W, B, LW, x.ptr, n, d, d, ninv.ptr, ld, alpha.ptr, 1,  # noqa: E731
                           1.0, None, 0, pf)
    ts = timed(sym, reps)
    ctx.call("smn_profile_enable", 1)
    sym()
    (pas, _), (con, _), (gram, _) = prof(6), prof(5), prof(1)
    ctx.call("smn_profile_enable", 0)
    npad = (n + 127) // 128 * 128
    es = np.dtype(dtype).itemsize
    flops = 2.0 * npad * npad * ((d + 127) // 128 * 128)
    moved = es * (npad * npad * 2.0)        # K0 and -K~^-1 lower triangles read (half a matrix each), W written in full
    print("    seeded entry alone min %.2f med %.2f ms: two-sided pass %.3f ms (%.2f TB/s of K0 + K~^-1 read and W written, 8 TB/s HBM "
          "roofline) | contraction %.3f ms = %.1f TF/s = %.1f %% of the %.1f TF/s %s MFMA peak | Gram build %.3f ms | rest (padding, "
          "transpose, tables, row sums, column sums) %.3f ms" % (ts[0], ts[1], pas, moved / pas / 1e9, con, flops / con / 1e9,
                                                                100 * flops / con / 1e9 / PEAK[dtype], PEAK[dtype], name, gram,
                                                                ts[0] - pas - con - gram), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    cases = [(int(args[i]), int(args[i + 1]), args[i + 2]) for i in range(0, len(args), 3)] or [(4096, 3072, "f32"), (16384, 3072, "f32"),
                                                                                               (8192, 3072, "f64")]
    for n, d, dt in cases:
        run(n, d, np.float32 if dt == "f32" else np.float64)
