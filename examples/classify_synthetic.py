#!/usr/bin/env python3
"""Evaluation of a sparse variational classifier (SVSP, svgp / svtp) on a synthetic image problem: class templates plus noise, inducing images drawn from the same classes, q_mu set to a noisy one-hot of the
inducing labels -- the problem of tests/test_gpu_svsp.py at a larger size.  Prints NLL, accuracy and the time of every
phase (cross kernel, per-image diagonal, posterior moments, Monte-Carlo softmax head).

    python examples/classify_synthetic.py [--method svgp|svtp] [--test 2000] [--inducing 100] [--hw 16] [--channels 1]
                                          [--classes 10] [--samples 10000] [--dtype float64|float32] [--layers 3]
    python examples/classify_synthetic.py --cifar-shape [--out FILE]   # T = 10000, I = 200, 32x32x3, 4 layers, C = 10,
                                                                       # S = 10000: svgp and svtp, head in fp32 and fp64
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smnngp import _lib, nt_kernels                                   # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.models import SVSP                                   # noqa: E402
from smnngp.spax.priors import GaussianPrior, InverseGammaPrior       # noqa: E402


def problem(num_inducing, num_test, num_class, hw, channels, seed=5):
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((num_class, hw, hw, channels))

    def images(n):
        lab = rng.integers(0, num_class, n)
        return templates[lab] + 1.6 * rng.standard_normal((n, hw, hw, channels)), lab.astype(np.int32)

    z, zl = images(num_inducing)
    x, y = images(num_test)
    q_mu = 2.0 * np.eye(num_class)[zl].T + 0.1 * rng.standard_normal((num_class, num_inducing))
    q_var = 0.01 + 0.05 * np.abs(rng.standard_normal((num_class, num_inducing)))
    return z, x, y, q_mu, q_var


def build(method, z, q_mu, q_var, layers, dtype, eps):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(layers, q_mu.shape[0], "relu", w_std=w, b_std=b, last_w_std=l),
                        1.2, 0.1, 1.0)
    prior = GaussianPrior() if method == "svgp" else InverseGammaPrior(2.0, 2.0)
    model = SVSP(prior, kernel, z, num_latent_gps=q_mu.shape[0], eps=eps, dtype=dtype)
    model.q_mu.assign(q_mu)
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(q_var))
    return model


def timed_phases(model, x, y, num_samples, seed=10, head_dtypes=(np.float32, np.float64), repeats=3):
    """One pass over the whole set in one batch, phase by phase, each phase `repeats` times between synchronisations
    (the minimum is reported; the first call of a phase also pays its one-time costs and is printed beside it)."""
    ctx = _lib.default_context()
    kernel_fn = model.kernel.get_kernel_fn()
    out = {}

    def clock(name, fn):
        times = []
        for _ in range(repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            res = fn()
            ctx.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        out[name] = (min(times), times[0])
        return res

    xd = ctx.to_device(np.ascontiguousarray(x, dtype=model.dtype))
    z, k_zz = clock("K(Z, Z), fp64", lambda: model.inducing_state(kernel_fn, ctx, refresh=True))
    k_zt = clock("cross kernel K(Z, x)", lambda: kernel_fn(z, xd, get="nngp"))
    t, (n_i, c) = xd.shape[0], (model.num_inducing, model.num_latent_gps)
    ktt = ctx.empty((t,), model.dtype)
    act, depth, w, b, lw = kernel_fn.params
    kind = 0 if kernel_fn.entry == "smn_kernel_cnn" else 1
    clock("diagonal K(x_t, x_t)", lambda: ctx.call("smn_kernel_conv_diag", xd.dcode, kind, act, depth, w, b, lw, xd.ptr, t,
                                                     xd.shape[1], xd.shape[2], xd.shape[3], ktt.ptr))
    mean, var = ctx.empty((t, c), model.dtype), ctx.empty((t, c), model.dtype)
    q_mu_d = ctx.to_device(np.asarray(model.q_mu.value, dtype=np.float64))
    q_var_d = ctx.to_device(np.asarray(model.q_sqrt.constraint(model.q_sqrt.value), dtype=np.float64))
    info, nonpos = C.c_int(), C.c_int64()
    clock("moments", lambda: ctx.call("smn_svsp_moments", xd.dcode, k_zz.ptr, k_zt.ptr, ktt.ptr, q_mu_d.ptr, q_var_d.ptr, n_i, t,
                                      c, model.eps.safe_value, mean.ptr, var.ptr, C.byref(info), C.byref(nonpos)))
    df, scale = model.prior.head_params()
    labels = np.ascontiguousarray(y, dtype=np.int32)
    results = {}
    pred_d = C.c_void_p()                                                               # [T] int32
    ctx.call("smn_malloc", max(4 * t, 16), C.byref(pred_d))
    for hd in head_dtypes:
        with np.errstate(invalid="ignore"):
            md = ctx.to_device(mean.numpy().astype(hd))
            sd = ctx.to_device(np.sqrt(scale * var.numpy()).astype(hd))
        ll = ctx.empty((t,), np.float64)
        name = "head, %s" % np.dtype(hd).name
        clock(name, lambda: ctx.call("smn_mc_softmax", md.dcode, md.ptr, sd.ptr, labels.ctypes.data_as(C.POINTER(C.c_int)), t, c,
                                     int(num_samples), df, seed, 0, None, ll.ptr, pred_d, None))
        p = np.empty(t, dtype=np.int32)
        ctx.call("smn_memcpy_d2h", p.ctypes.data_as(C.c_void_p), pred_d, 4 * t)
        results[name] = (float(-np.mean(ll.numpy())), 100.0 * float(np.mean(p == labels)),
                         t * c * num_samples / (out[name][0] * 1e-3))
    ctx.call("smn_free", pred_d)
    return out, results, info.value, nonpos.value


def cifar_shape(args):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t, n_i, c, s = 10000, 200, 10, 10000
    z, x, y, q_mu, q_var = problem(n_i, t, c, 32, 3)
    say("SVSP evaluation at the CIFAR-10 test shape: T = %d, I = %d, 32x32x3, 4-layer ReLU get_cnn_kernel, C = %d, S = %d" % (t, n_i, c, s))
    say("(synthetic images; kernel, moments and inputs in fp64; min of 3 runs per phase, first run in brackets; host wall clock")
    say(" between stream synchronisations)")
    for method in ("svgp", "svtp"):
        model = build(method, z, q_mu, q_var, 4, np.float64, 1e-6)
        phases, results, info, nonpos = timed_phases(model, x, y, s)
        say()
        say("%s   (info %d, non-positive variances %d)" % (method, info, nonpos))
        for name, (best, first) in phases.items():
            say("  %-24s %10.2f ms   (%.2f)" % (name, best, first))
        for name, (nll, acc, rate) in results.items():
            say("  %-24s NLL %.5f  ACC %.2f %%  %.3g variates / s" % (name, nll, acc, rate))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--method", default="svtp", choices=["svgp", "svtp"])
    ap.add_argument("--test", type=int, default=2000)
    ap.add_argument("--inducing", type=int, default=100)
    ap.add_argument("--hw", type=int, default=16)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--cifar-shape", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.cifar_shape:
        return cifar_shape(args)
    dtype = np.dtype(args.dtype).type
    z, x, y, q_mu, q_var = problem(args.inducing, args.test, args.classes, args.hw, args.channels)
    model = build(args.method, z, q_mu, q_var, args.layers, dtype, args.eps)
    t0 = time.perf_counter()
    nll, acc = model.evaluate(x, y, args.samples, seed=10, batch=args.batch)
    dt = time.perf_counter() - t0
    print("%s, %d test images %dx%dx%d, %d inducing, %d classes, %d draws, %s" % (args.method, args.test, args.hw, args.hw,
                                                                                args.channels, args.inducing, args.classes,
                                                                                args.samples, args.dtype))
    print("NLL: %.5f  ACC: %.2f   (evaluate: %.1f ms, first call)" % (nll, acc, 1e3 * dt))
    phases, results, _, _ = timed_phases(model, x, y, args.samples, head_dtypes=(dtype,))
    for name, (best, first) in phases.items():
        print("  %-24s %10.2f ms   (%.2f)" % (name, best, first))
    for name, (_, _, rate) in results.items():
        print("  %-24s %.3g variates / s" % (name, rate))


if __name__ == "__main__":
    main()
