"""Timings of the fitted posterior (csrc/fit.hip, posterior.py) beside the route it replaces, for profiles/r18_fit_predict.txt.

    python scratch/fit_probe.py [--out FILE] [--sizes 4096,16384] [--reps 5]

README's predictive shape: N training points, d = 3072, T = 2048 test points, fp32, 4-layer ReLU MLP.  Per N, ms per call
(median of --reps after one warm-up, host clock around a call that ends in a stream synchronise):
    smn_fit_create                              (build + factorisation + state allocation)
    smn_fit_predict, var_d only                 (cross build + solve + read-out)
    smn_fit_predict, var_d and cov_d            (+ K_tt build, Schur update, extraction)
    smn_spr_predict                             (the joint factorisation every call of the existing route pays)
    SPR.test_nll second call / post.test_nll    (gp and tp, same split, same session)
    read-out kernel alone                       (smn_profile_read category 6) against n_pad * T * 4 bytes
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

D, T, LAYERS, CAP = 3072, 2048, 4, 2048
HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def timed(ctx, fn, reps):
    fn()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from smnngp import _lib as L, nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR
    ctx = L.default_context()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for n in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        x = rng.standard_normal((n, D)).astype(np.float32)
        xt = rng.standard_normal((T, D)).astype(np.float32)
        y = np.sin(x[:, :8].sum(axis=1)).astype(np.float64)
        yt = np.sin(xt[:, :8].sum(axis=1)).astype(np.float64)
        xd, xtd, yd = ctx.to_device(x), ctx.to_device(xt), ctx.to_device(y.astype(np.float32))
        mean, var, cov = ctx.empty((T, 1), np.float32), ctx.empty((T,), np.float32), ctx.empty((T, T), np.float32)
        quad, logdet, info = (C.c_double * 1)(), C.c_double(), C.c_int()
        hyp = (1.0, 0.5, 1.0)
        eps = 1e-2
        say("== N = %d, d = %d, T = %d, fp32, %d-layer ReLU, ridge_rel %.0e, capacity %d, %d reps (median [min, max] ms)"
            % (n, D, T, LAYERS, eps, CAP, a.reps))
        handles = []

        def create():
            h = C.c_void_p()
            ctx.call("smn_fit_create", L.F32, L.NET_MLP, L.ACT["relu"], LAYERS, *hyp, xd.ptr, n, D, D, yd.ptr, 1, eps, 0.0, CAP,
                     C.byref(h), quad, C.byref(logdet), C.byref(info))
            handles.append(h)
            if len(handles) > 1:
                ctx.call_on("smn_fit_destroy", handles.pop(0))

        say("smn_fit_create                      %8.3f [%.3f, %.3f]" % timed(ctx, create, a.reps))
        h = handles[0]
        nbytes = C.c_size_t()
        ctx.call_on("smn_fit_info", h, None, None, None, C.byref(nbytes))
        say("  state: %.1f MB, info %d, logdet %.6g" % (nbytes.value / 1e6, info.value, logdet.value))
        diag = lambda: ctx.call_on("smn_fit_predict", h, xtd.ptr, T, D, mean.ptr, var.ptr, None, 0)      # noqa: E731
        full = lambda: ctx.call_on("smn_fit_predict", h, xtd.ptr, T, D, mean.ptr, var.ptr, cov.ptr, T)   # noqa: E731
        joint = lambda: ctx.call("smn_spr_predict", L.F32, L.NET_MLP, L.ACT["relu"], LAYERS, *hyp, xd.ptr, n, D, xtd.ptr, T, D,  # noqa: E731
                                 D, yd.ptr, 1, eps, 0.0, mean.ptr, cov.ptr, T, quad, C.byref(logdet), C.byref(info))
        t_diag = timed(ctx, diag, a.reps)
        say("smn_fit_predict var_d only          %8.3f [%.3f, %.3f]" % t_diag)
        v_fit = var.raw_numpy().astype(np.float64)
        say("smn_fit_predict var_d + cov_d       %8.3f [%.3f, %.3f]" % timed(ctx, full, a.reps))
        c_fit = np.diag(cov.raw_numpy()).astype(np.float64)
        t_joint = timed(ctx, joint, a.reps)
        say("smn_spr_predict (existing route)    %8.3f [%.3f, %.3f]" % t_joint)
        c_joint = np.diag(cov.raw_numpy()).astype(np.float64)
        say("  diag-only call / existing call = %.3f;  max |var - diag(cov_joint)| / max = %.2e (read-out), %.2e (Schur)"
            % (t_diag[0] / t_joint[0], np.abs(v_fit - c_joint).max() / c_joint.max(), np.abs(c_fit - c_joint).max() / c_joint.max()))
        # the read-out kernel alone
        ctx.call("smn_profile_enable", 2 << 6)
        for _ in range(a.reps):
            diag()
        ctx.synchronize()
        ms, cnt = C.c_double(), C.c_int()
        ctx.call("smn_profile_read", 6, C.byref(ms), C.byref(cnt))
        ctx.call("smn_profile_enable", 0)
        n_pad = (n + 127) // 128 * 128
        per = ms.value / max(cnt.value, 1)
        nb = n_pad * T * 4
        say("read-out kernel alone               %8.4f ms per launch (%d launches): %.1f MB of solved rows -> %.2f TB/s, %.0f %% of the "
            "%.0f TB/s HBM peak" % (per, cnt.value, nb / 1e6, nb / (per * 1e-3) / 1e12, 100 * nb / (per * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
        ctx.call_on("smn_fit_destroy", h)
        # wide Y (c = 48): the read-out kernel's six passes of eight columns, beside the mean through the NT tile engine
        # (smn_gram on operands of the solved rows' shape, [T, n_pad] x [48, n_pad]; kernel time = profile category 1)
        c48 = 48
        y48 = ctx.to_device(rng.standard_normal((n, c48)).astype(np.float32))
        mean48, quad48, h48 = ctx.empty((T, c48), np.float32), (C.c_double * c48)(), C.c_void_p()
        ctx.call("smn_fit_create", L.F32, L.NET_MLP, L.ACT["relu"], LAYERS, *hyp, xd.ptr, n, D, D, y48.ptr, c48, eps, 0.0, CAP,
                 C.byref(h48), quad48, C.byref(logdet), C.byref(info))
        wide = lambda: ctx.call_on("smn_fit_predict", h48, xtd.ptr, T, D, mean48.ptr, var.ptr, None, 0)   # noqa: E731
        say("smn_fit_predict var_d only, c = 48  %8.3f [%.3f, %.3f]" % timed(ctx, wide, a.reps))
        ctx.call("smn_profile_enable", 2 << 6)
        for _ in range(a.reps):
            wide()
        ctx.synchronize()
        ctx.call("smn_profile_read", 6, C.byref(ms), C.byref(cnt))
        ctx.call("smn_profile_enable", 0)
        per48 = ms.value / max(cnt.value, 1)
        ctx.call_on("smn_fit_destroy", h48)
        va = ctx.to_device(rng.standard_normal((T, n_pad)).astype(np.float32))
        vb = ctx.to_device(rng.standard_normal((c48, n_pad)).astype(np.float32))
        gram = lambda: ctx.call("smn_gram", L.F32, va.ptr, T, n_pad, vb.ptr, c48, n_pad, n_pad, mean48.ptr, c48, None, None)   # noqa: E731
        t_gram = timed(ctx, gram, a.reps)
        ctx.call("smn_profile_enable", 2 << 1)
        for _ in range(a.reps):
            gram()
        ctx.synchronize()
        ctx.call("smn_profile_read", 1, C.byref(ms), C.byref(cnt))
        ctx.call("smn_profile_enable", 0)
        per_gram = ms.value / max(cnt.value, 1)
        say("wide Y, c = 48: read-out kernel (mean + var, 6 passes) %.4f ms per launch;  alternative = sum of squares alone (the "
            "c = 1 launch above, %.4f ms) + NT tile engine [T, n_pad] x [48, n_pad]: %.4f ms kernel (smn_gram call with its "
            "operand padding: %.3f [%.3f, %.3f] ms) = %.4f ms" % (per48, per, per_gram, *t_gram, per + per_gram))
        # model level
        for method in ("gp", "tp"):
            kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(LAYERS, act="relu", w_std=w, b_std=b, last_w_std=l), *hyp)
            lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
            model = SPR(kernel, lik, xd, y, 0.0, 1.0, eps=eps)
            first = time.perf_counter()
            ref = model.test_nll(xtd, yt)
            first = (time.perf_counter() - first) * 1e3
            t_model = timed(ctx, lambda: model.test_nll(xtd, yt), a.reps)
            t0 = time.perf_counter()
            post = model.posterior(capacity=CAP)
            t_post0 = (time.perf_counter() - t0) * 1e3
            got = post.test_nll(xtd, yt)
            t_post = timed(ctx, lambda: post.test_nll(xtd, yt), a.reps)
            say("%s  SPR.test_nll first %.2f, later %8.3f [%.3f, %.3f]   posterior() %.2f, post.test_nll %8.3f [%.3f, %.3f]   "
                "ratio %.3f   nll %.6f / %.6f" % (method, first, *t_model, t_post0, *t_post, t_post[0] / t_model[0], ref, got))
            post.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
