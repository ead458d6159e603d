"""predict_grad against predict(cov="diag") of the same state; kernel-level times of the hot kernel and the contraction."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smnngp import _lib as L  # noqa: E402

ctx = L.default_context()
D, T, CAP, LAYERS = 3072, 2048, 2048, 2
rng = np.random.default_rng(0)


def timed(fn, reps):
    fn(); ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ctx.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


for n in (4096, 16384):
    x = ctx.to_device(rng.standard_normal((n, D)).astype(np.float32))
    xt = ctx.to_device(rng.standard_normal((T, D)).astype(np.float32))
    for c in (1, 10):
        y = ctx.to_device(rng.standard_normal((n, c)).astype(np.float32))
        h, info = C.c_void_p(), C.c_int()
        ctx.call("smn_fit_create", L.F32, 0, 0, LAYERS, 1.3, 0.2, 1.0, x.ptr, n, D, D, y.ptr, c, 1e-2, 0.0, CAP, C.byref(h), None, None, C.byref(info))
        mean, var = ctx.empty((T, c), np.float32), ctx.empty((T,), np.float32)
        dm, dv = ctx.empty((T, c, D), np.float32), ctx.empty((T, D), np.float32)
        pred = lambda: ctx.call_on("smn_fit_predict", h, xt.ptr, T, D, mean.ptr, var.ptr, None, T)          # noqa: E731
        both = lambda: ctx.call_on("smn_fit_predict_grad", h, xt.ptr, T, D, dm.ptr, dv.ptr)                 # noqa: E731
        only_m = lambda: ctx.call_on("smn_fit_predict_grad", h, xt.ptr, T, D, dm.ptr, None)                # noqa: E731
        t0 = time.perf_counter(); both(); ctx.synchronize(); first = (time.perf_counter() - t0) * 1e3
        reps = 5 if n == 4096 else 3
        p, g, m = timed(pred, reps), timed(both, reps), timed(only_m, reps)
        print("N=%d c=%d info=%d  predict(diag) min %.2f med %.2f ms | predict_grad mean+var min %.2f med %.2f ms (first call %.1f ms) | mean only min %.2f med %.2f ms | ratio %.2f"
              % (n, c, info.value, p[0], p[1], g[0], g[1], first, m[0], m[1], g[0] / p[0]), flush=True)
        # kernel-level: a mean-only call launches the hot kernel once (category 1) and the contraction c times (category 5)
        ctx.call("smn_profile_enable", 1)
        only_m()
        hot, con, nh, nc = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        ctx.call("smn_profile_read", 1, C.byref(hot), C.byref(nh))
        ctx.call("smn_profile_read", 5, C.byref(con), C.byref(nc))
        ctx.call("smn_profile_enable", 0)
        npad = (n + 127) // 128 * 128
        gram_flops = 2.0 * T * npad * D
        print("    hot kernel %.3f ms (%d launch): Gram part %.1f TF/s = %.1f %% of the 157.3 TF/s f32 MFMA peak | contraction %.3f ms per launch (%d launches), %.1f TF/s"
              % (hot.value, nh.value, gram_flops / hot.value / 1e9, 100 * gram_flops / hot.value / 1e9 / 157.3, con.value / max(nc.value, 1),
                 nc.value, gram_flops / (con.value / max(nc.value, 1)) / 1e9), flush=True)
        ctx.call_on("smn_fit_destroy", h)
