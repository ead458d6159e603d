"""Conv-NNGP analytic gradient (SPR.loss_and_grad, csrc/cnn_grad.hip) against the path it replaces,
train.value_and_grad_fd(model.loss, train_vars(model)): same model, same process, runs alternated, per-call wall times
after a warm-up, random (not zero) images.

    python scratch/cnn_grad_probe.py n2048      32x32x3, L = 4, relu, fp64, N = 2048, both heads, five alternated repetitions
    python scratch/cnn_grad_probe.py c3         N = 10000, Student-t (BASELINE config C3), one run each
    python scratch/cnn_grad_probe.py small      8x8x1, N = 245, fp32 (latency)
    python scratch/cnn_grad_probe.py terms      the contraction alone (smn_kernel_cnn_grad_terms): pair-pixel-layers / s
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smnngp import _lib as L, nt_kernels, train  # noqa: E402
from smnngp.spax.kernels import NNGPKernel  # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR  # noqa: E402


def model_of(n, shape, layers, dtype, head, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n,) + shape).astype(dtype)
    y = rng.standard_normal(n).astype(dtype)
    k = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(layers, 1, act="relu", w_std=w, b_std=b, last_w_std=l),
                   1.0, 0.3, 1.0)
    lik = GaussianLikelihood() if head == "gp" else StudentTLikelihood(2.0, 2.0)
    return SPR(k, lik, x, y, 0.0, 1.0, eps=1e-2)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def compare(n, shape, layers, dtype, head, reps):
    m = model_of(n, shape, layers, dtype, head)
    tv = train.train_vars(m)
    tag = "N=%d %dx%dx%d L=%d %s %s" % ((n,) + shape + (layers, np.dtype(dtype).name, head))
    m.loss_and_grad(); m.loss()                                      # warm-up: workspaces, LDS attributes
    ta, tf, tl = [], [], []
    for r in range(reps):
        a, (la, ga) = timed(m.loss_and_grad)
        f, (lf, gf) = timed(lambda: train.value_and_grad_fd(m.loss, tv))
        l, _ = timed(m.loss)
        ta.append(a); tf.append(f); tl.append(l)
        print("%s rep %d: loss_and_grad %.2f ms, value_and_grad_fd (%d loss evaluations) %.2f ms, loss %.2f ms"
              % (tag, r, a, 1 + 2 * len(tv), f, l), flush=True)
    worst = max(abs(ga[k] - gf[k]) / max(max(abs(v) for v in gf.values()), 1e-300) for k in gf)
    med = lambda v: float(np.median(v))
    print("%s: medians loss_and_grad %.2f ms, FD %.2f ms, loss %.2f ms => %.2f loss evaluations per analytic call, "
          "%.1fx faster than FD; every analytic run faster than every FD run: %s; analytic vs FD gradients differ by %.2g of the largest"
          % (tag, med(ta), med(tf), med(tl), med(ta) / med(tl), med(tf) / med(ta), max(ta) < min(tf), worst), flush=True)


def terms_rate(n, shape, layers, dtype, reps=3):
    ctx = L.default_context()
    rng = np.random.default_rng(1)
    h, w, c = shape
    xd = ctx.to_device(rng.standard_normal((n,) + shape).astype(dtype))
    g = rng.standard_normal((n, n)).astype(dtype)
    gd, ad = ctx.to_device(g + g.T), ctx.to_device(rng.standard_normal(n).astype(dtype))
    terms = (C.c_double * 4)()
    call = lambda: ctx.call("smn_kernel_cnn_grad_terms", L.dtype_code(dtype), L.ACT["relu"], layers, 1.0, 0.3, 1.0, xd.ptr, n,
                            h, w, c, gd.ptr, n, ad.ptr, 1.0, terms)
    kd = ctx.empty((n, n), dtype)
    fwd = lambda: (ctx.call("smn_kernel_cnn", L.dtype_code(dtype), L.ACT["relu"], layers, 1.0, 0.3, 1.0, xd.ptr, n, None, 0,
                            h, w, c, L.FILL_LOWER, kd.ptr, n), ctx.synchronize())
    call(); fwd()
    ppl = n * (n + 1) / 2 * h * w * layers
    for r in range(reps):
        t, _ = timed(call)
        tf, _ = timed(fwd)
        print("N=%d %dx%dx%d L=%d %s rep %d: tangent contraction %.2f ms = %.3g pair-pixel-layers/s; forward build %.2f ms = "
              "%.3g pair-pixel-layers/s; ratio %.2f" % ((n,) + shape + (layers, np.dtype(dtype).name, r, t, ppl / t * 1e3, tf,
                                                                  ppl / tf * 1e3, t / tf), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["small"]
    if "n2048" in what:
        for head in ("gp", "tp"):
            compare(2048, (32, 32, 3), 4, np.float64, head, 5)
    if "c3" in what:
        compare(10000, (32, 32, 3), 4, np.float64, "tp", 1)
    if "small" in what:
        compare(245, (8, 8, 1), 4, np.float32, "tp", 5)
    if "terms" in what:
        terms_rate(2048, (32, 32, 3), 4, np.float64)
        terms_rate(2048, (32, 32, 3), 4, np.float32)
