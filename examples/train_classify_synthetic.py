#!/usr/bin/env python3
"""Training a sparse variational classifier (SVSP, svgp and svtp) on the synthetic image problem of classify_synthetic.py:
class templates plus noise, inducing images = a subset of the training set (fixed by default; --train-inducing trains them
too, as the reference does), q_mu = 0, q_sqrt = 1 as the constructor leaves them.  Prints the mean nELBO of every epoch, validation NLL and accuracy
before and after, and the time of every phase of a step.

    python examples/train_classify_synthetic.py [--train 1024] [--valid 512] [--inducing 64] [--hw 8] [--classes 4]
                                                [--epochs 6] [--batch 64] [--samples 32] [--lr 1e-2] [--dtype float64]
                                                [--train-inducing]
    python examples/train_classify_synthetic.py --reference-shape [--out FILE]
        # the reference's training shape: I = 200, B = 100, C = 10, S = 100, 32x32x3, 4 layers; both priors, fp32 and fp64
        # heads, kernel_grads and inducing_grad on and off; per-phase and whole-step times (device events of the context's timer)
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smnngp import _lib, nt_kernels, train_svsp                       # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.models import SVSP                                   # noqa: E402
from smnngp.spax.priors import GaussianPrior, InverseGammaPrior       # noqa: E402


def problem(num_train, num_valid, num_class, hw, channels, seed=5):
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((num_class, hw, hw, channels))

    def images(n):
        lab = rng.integers(0, num_class, n)
        return templates[lab] + 1.6 * rng.standard_normal((n, hw, hw, channels)), lab.astype(np.int32)

    return images(num_train) + images(num_valid)


def build(method, z, num_class, layers, dtype, eps):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(layers, num_class, "relu", w_std=w, b_std=b, last_w_std=l),
                        1.2, 0.1, 1.0)
    prior = GaussianPrior() if method == "svgp" else InverseGammaPrior(2.0, 2.0)
    return SVSP(prior, kernel, z, num_latent_gps=num_class, eps=eps, dtype=dtype)


def device_ms(ctx, fn, repeats=5, warmup=2):
    """Median and minimum time of fn() in ms between the context's device events (smn_timer_start / smn_timer_stop_ms)."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        ms = C.c_double()
        ctx.call("smn_timer_start")
        fn()
        ctx.call("smn_timer_stop_ms", C.byref(ms))
        times.append(ms.value)
    return float(np.median(times)), float(np.min(times))


def step_phases(model, x, y, num_train, num_samples, head_dtype, repeats=5):
    """The device phases of one SVSP.loss_and_grad, timed one by one: union build, ELBO forward + reverse, tangent pass,
    reverse pass for the inducing images."""
    ctx = _lib.default_context()
    kernel_fn = model.kernel.get_kernel_fn()
    n_i, c, n_b = model.num_inducing, model.num_latent_gps, len(y)
    n_u = n_i + n_b
    u = ctx.to_device(np.ascontiguousarray(np.concatenate([np.asarray(model.inducing_variable.value), x]), dtype=np.float64))
    out = {}
    hold = {}

    def build_k():
        hold["k"] = kernel_fn(u, None, get="nngp")

    out["union build K(U,U), fp64"] = device_ms(ctx, build_k, repeats)
    k = hold["k"]
    pp = model.prior.elbo_params()
    q_mu_d = ctx.to_device(np.asarray(model.q_mu.value, dtype=np.float64))
    q_var_d = ctx.to_device(np.asarray(model.q_sqrt.constraint(model.q_sqrt.value), dtype=np.float64))
    g_mu, g_var, gbar = ctx.empty((c, n_i), np.float64), ctx.empty((c, n_i), np.float64), ctx.empty((n_u, n_u), np.float64)
    sc = [C.c_double() for _ in range(6)]
    info = C.c_int()
    labels = np.ascontiguousarray(y, dtype=np.int32)

    def elbo():
        ctx.call("smn_svsp_elbo_grad", _lib.dtype_code(head_dtype), k.ptr, n_u, n_i, n_b, c, q_mu_d.ptr, q_var_d.ptr,
                 model.eps.safe_value, pp["s"], float(num_train), labels.ctypes.data_as(C.POINTER(C.c_int)), int(num_samples),
                 pp["df"], pp["scale"], 1, 0, None, None, C.byref(sc[0]), C.byref(sc[1]), g_mu.ptr, g_var.ptr, C.byref(sc[2]),
                 C.byref(sc[3]), C.byref(sc[4]), C.byref(sc[5]), gbar.ptr, n_u, C.byref(info))

    out["smn_svsp_elbo_grad, %s head" % np.dtype(head_dtype).name] = device_ms(ctx, elbo, repeats)
    act, depth, w, b, lw = kernel_fn.params
    zeros = ctx.to_device(np.zeros(n_u))
    terms = (C.c_double * 4)()

    def tangent():
        ctx.call("smn_kernel_cnn_grad_terms", _lib.F64, act, depth, w, b, lw, u.ptr, n_u, u.shape[1], u.shape[2], u.shape[3],
                 gbar.ptr, n_u, zeros.ptr, 0.0, terms)

    if u.shape[1] * u.shape[2] <= 1024:
        out["tangent pass (3 kernel gradients)"] = device_ms(ctx, tangent, repeats)
        gz = ctx.empty((n_i,) + tuple(u.shape[1:]), np.float64)

        def reverse():
            ctx.call("smn_kernel_cnn_input_grad", _lib.F64, act, depth, w, b, lw, u.ptr, n_u, u.shape[1], u.shape[2], u.shape[3],
                     gbar.ptr, n_u, n_i, gz.ptr)

        out["reverse pass (inducing-image gradient)"] = device_ms(ctx, reverse, repeats)
    return out, info.value, (k, gbar)


def reference_shape(args):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n_i, n_b, c, s, n_train = 200, 100, 10, 100, 50000
    xt, yt, _, _ = problem(n_i + n_b, 1, c, 32, 3)
    z, x, y = xt[:n_i], xt[n_i:], yt[n_i:]
    ctx = _lib.default_context()
    say("SVSP training step at the reference's shape: I = %d inducing, B = %d, C = %d, S = %d, 32x32x3, 4-layer ReLU get_cnn_kernel"
        % (n_i, n_b, c, s))
    say("(synthetic images; median [min] of 5 runs after 2 warm-up runs; device events of the context's timer around each phase;")
    say(" 'step' = SVSP.loss_and_grad as a user calls it, host arithmetic, uploads and downloads included)")
    for method in ("svgp", "svtp"):
        for hd in (np.float32, np.float64):
            model = build(method, z, c, 4, hd, 1e-6)
            rng = np.random.default_rng(1)
            model.q_mu.assign(0.1 * rng.standard_normal((c, n_i)))
            phases, info, _ = step_phases(model, x, y, n_train, s, hd)
            say()
            say("%s, %s head   (info %d)" % (method, np.dtype(hd).name, info))
            for name, (med, mn) in phases.items():
                say("  %-44s %9.3f ms  [%.3f]" % (name, med, mn))
            for kg in (True, False):
                med, mn = device_ms(ctx, lambda: model.loss_and_grad(1, x, y, n_train, s, kernel_grads=kg))
                say("  %-44s %9.3f ms  [%.3f]" % ("step, kernel_grads=%s" % kg, med, mn))
            med, mn = device_ms(ctx, lambda: model.loss_and_grad(1, x, y, n_train, s, inducing_grad=True))
            say("  %-44s %9.3f ms  [%.3f]" % ("step, kernel_grads=True, inducing_grad=True", med, mn))
    # for scale: the same algebra in fp64 NumPy on the host (the rules of the tests, fed the device's K and variates), and what
    # central differences over every scalar trainable would cost in calls of the new path
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    model = build("svgp", z, c, 4, np.float64, 1e-6)
    try:
        import _svsp_elbo_rules as E
    except ImportError as e:                                                       # the rules need scipy
        say("host rules not timed: %s" % e)
    else:
        _, _, (k, _) = step_phases(model, x, y, n_train, s, np.float64, repeats=1)
        kh = k.raw_numpy()
        xi = np.random.default_rng(2).standard_normal((c, n_b, s))
        t0 = time.perf_counter()
        E.elbo(kh, n_i, np.asarray(model.q_mu.value), np.ones((c, n_i)), 1e-6, 1.0, n_train, y, xi, 1.0)
        say()
        say("host rules (fp64 NumPy, K given: no kernel build)  %9.1f ms   one call, wall clock" % (1e3 * (time.perf_counter() - t0)))
    nvar = 2 * c * n_i + 1 + 3 + 2
    med, _ = device_ms(ctx, lambda: model.loss_and_grad(1, x, y, n_train, s, kernel_grads=False))
    say("central differences instead: 2 x %d scalar trainables (q_mu, q_sqrt, eps, 3 kernel, a, b) = %d calls of the build + ELBO path"
        % (nvar, 2 * nvar))
    say("  at %.3f ms each (svgp, fp64 head: step, kernel_grads=False, which also runs the reverse pass: an upper bound of a forward-only call)"
        " = %.1f s per step -- not run, extrapolated from that one timing" % (med, 2 * nvar * med * 1e-3))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train", type=int, default=1024)
    ap.add_argument("--valid", type=int, default=512)
    ap.add_argument("--inducing", type=int, default=64)
    ap.add_argument("--hw", type=int, default=8)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--eval-samples", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--train-inducing", action="store_true", help="the inducing images are trained too (classification/train.py:205)")
    ap.add_argument("--reference-shape", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reference_shape:
        return reference_shape(args)
    dtype = np.dtype(args.dtype).type
    xt, yt, xv, yv = problem(args.train, args.valid, args.classes, args.hw, args.channels)
    ok = True
    for method in ("svgp", "svtp"):
        model = build(method, xt[:args.inducing].copy(), args.classes, args.layers, dtype, args.eps)   # train.py:177-182
        step = train_svsp.build_svsp_train_step(model, train_svsp.svsp_train_vars(model, inducing=args.train_inducing),
                                                num_train=args.train, num_samples=args.samples)
        sched = train_svsp.PlateauSchedule(args.lr)
        nll0, acc0 = model.evaluate(xv, yv, args.eval_samples)
        print("%s: %d training images %dx%dx%d, %d inducing (%s), %d classes, batches of %d, S = %d, %s head" %
              (method, args.train, args.hw, args.hw, args.channels, args.inducing, "trained" if args.train_inducing else "fixed",
               args.classes, args.batch, args.samples, args.dtype))
        print("  before: validation NLL %.5f  ACC %.2f" % (nll0, acc0))
        for e in range(args.epochs):
            t0 = time.perf_counter()
            nelbo = train_svsp.train_epoch(step, xt, yt, args.batch, sched.lr, seed=1, epoch=e)
            dt = time.perf_counter() - t0
            nll, acc = train_svsp.valid_epoch(model, xv, yv, args.eval_samples, schedule=sched)
            print("  epoch %2d  nELBO %.5f  validation NLL %.5f  ACC %.2f  lr %.1e  (%.1f ms / step)" %
                  (e, nelbo, nll, acc, sched.lr, 1e3 * dt / (args.train // args.batch)))
        print("  after:  validation NLL %.5f  ACC %.2f" % (nll, acc))
        phases, _, _ = step_phases(model, xt[:args.batch], yt[:args.batch], args.train, args.samples, dtype)
        for name, (med, mn) in phases.items():
            print("  %-44s %9.3f ms  [%.3f]" % (name, med, mn))
        ok = ok and nll < nll0
    if not ok:
        raise SystemExit("validation NLL did not go down")


if __name__ == "__main__":
    main()
