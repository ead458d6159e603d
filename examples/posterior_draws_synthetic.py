#!/usr/bin/env python3
"""Joint posterior function draws (SPR.sample_posterior) on the reference's offline regression sets: 1000 draws of the
latent function at the held-out points under the Gaussian process (gp) and the Student-t process (tp), and what only a
joint draw can give -- the simultaneous credible band next to the pointwise one.

    python examples/posterior_draws_synthetic.py [syn-t|syn-normal]
    python examples/posterior_draws_synthetic.py --time [float32|float64]

--time: the fused smn_mvn_draws against the composition smn_rng_variates + smn_transpose + smn_gram (which stores the
[T,C,S] variates twice) at T = 2048, C = 10, S = 1000.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from regression_synthetic import dataset                              # noqa: E402
from smnngp import _lib, nt_kernels, train                            # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR                                    # noqa: E402


def bands(name, method, num_samples=1000, level=0.9):
    (xtr, ytr), _, (xte, yte), (ym, ys) = dataset(name)
    order = np.argsort(xte[:, 0])
    xte, yte = xte[order], yte[order]
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    model = SPR(kernel, likelihood, xtr, ytr, ym, ys, eps=1e-2)
    step = train.build_train_step(model)                              # analytic gradient + Adam, as regression_synthetic.py
    for _ in range(150):
        step(0.03)
    df_post, shape = model.predictive_params()
    f = model.sample_posterior(10, xte, num_samples).numpy() * ys + ym            # de-normalised, as test_nll does
    mean, cov = model.predict(xte)
    mean = np.asarray(mean, dtype=np.float64).ravel() * ys + ym
    sd = np.sqrt(shape * np.asarray(cov.diagonal(), dtype=np.float64)) * ys
    lo, med, hi = np.quantile(f, [(1 - level) / 2, 0.5, (1 + level) / 2], axis=0)
    # simultaneous band: the half-width in units of sd that holds level of the DRAWS over all points at once
    sup = np.max(np.abs(f - mean) / sd, axis=1)
    joint = np.quantile(sup, level)
    point = np.quantile(np.abs(f - mean) / sd, level)
    print("%s / %s: df_post %s, shape %.4f, test_nll %.5f" % (name, method, "inf" if df_post is None else "%.1f" % df_post,
                                                                shape, model.test_nll(xte, yte)))
    print("  %d draws at %d points; %.0f %% half-width in sd units: pointwise %.3f, simultaneous %.3f"
          % (num_samples, len(yte), 100 * level, point, joint))
    print("  %8s %9s %9s %9s %9s" % ("x", "q%02d" % round(50 * (1 - level)), "median", "q%02d" % round(50 * (1 + level)), "y"))
    for i in range(0, len(yte), max(1, len(yte) // 8)):
        print("  %8.3f %9.4f %9.4f %9.4f %9.4f" % (xte[i, 0], lo[i], med[i], hi[i], yte[i] * ys + ym))


def timing(dtype, t=2048, c=10, s=1000, reps=20):
    ctx = _lib.default_context()
    dtype = np.dtype(dtype)
    code = _lib.dtype_code(dtype)
    rng = np.random.default_rng(0)
    lo = ctx.to_device((np.tril(rng.standard_normal((t, t))) / np.sqrt(t)).astype(dtype))
    mean = ctx.to_device(np.zeros((t, c), dtype=dtype))
    out = ctx.empty((s, t, c), dtype)
    z, zt, prod = ctx.empty((t, c * s), dtype), ctx.empty((c * s, t), dtype), ctx.empty((c * s, t), dtype)

    def fused():
        ctx.call("smn_mvn_draws", code, mean.ptr, lo.ptr, t, t, c, s, 0.0, 1.0, 1, 0, None, None, out.ptr)

    def composed():
        ctx.call("smn_rng_variates", code, 1, 0.0, 0, t, c, s, z.ptr)
        ctx.call("smn_transpose", code, zt.ptr, t, z.ptr, c * s, t, c * s)
        ctx.call("smn_gram", code, zt.ptr, c * s, t, lo.ptr, t, t, t, prod.ptr, t, None, None)     # zt lo^T / t
        ctx.synchronize()

    # host clock around calls that end in a device synchronisation; both paths warmed up, then alternating
    paths = (("fused smn_mvn_draws", fused), ("smn_rng_variates + smn_transpose + smn_gram", composed))
    times = {name: [] for name, _ in paths}
    for rep in range(reps + 2):
        for name, fn in paths:
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            if rep >= 2:
                times[name].append(time.perf_counter() - t0)
    for name, _ in paths:
        print("%s T %d C %d S %d  %-46s %d calls: min %8.3f ms  median %8.3f ms"
              % (dtype.name, t, c, s, name, reps, 1e3 * min(times[name]), 1e3 * float(np.median(times[name]))))


if __name__ == "__main__":
    if "--time" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--time"]
        timing(rest[0] if rest else "float32")
    else:
        data = sys.argv[1] if len(sys.argv) > 1 else "syn-t"
        for m in ("gp", "tp"):
            bands(data, m)
