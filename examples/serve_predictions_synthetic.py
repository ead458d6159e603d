#!/usr/bin/env python3
"""Fit once, predict many: `SPR.posterior()` on the reference's offline regression dataset.

    python examples/serve_predictions_synthetic.py [syn-t|syn-normal] [--capacity 64] [--repeat 8]

The model is fitted once (`post = model.posterior(capacity=...)`: the Cholesky factor of the training kernel stays on the
device), then `test_nll` is evaluated over a test set several times the capacity -- the held-out points repeated --, for the
Gaussian (`gp`) and the Student-t (`tp`) likelihood.  Printed: both values and the time per call of `model.test_nll`, which
factors the joint kernel of [train; test] on every call and forms the whole T x T covariance, beside `post.test_nll`, which
streams the test set through the state in chunks of `capacity` rows and only ever forms the variances.  At this size (240
training points) every call is a handful of launches and the chunked one has more of them: the example shows the surface and
the agreement of the two values; what serving buys is measured at N = 4096 and 16384 (profiles/r18_fit_predict.txt)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.regression_synthetic import dataset                     # noqa: E402
from smnngp import nt_kernels                                         # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR                                    # noqa: E402


def per_call(fn, reps=5):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()                                                    # returns a host float: the call has synchronised
    return out, (time.perf_counter() - t0) / reps * 1e3


def main():
    argv = list(sys.argv[1:])

    def option(name, default):
        if name in argv:
            i = argv.index(name)
            value = int(argv[i + 1])
            del argv[i:i + 2]
            return value
        return default

    capacity, repeat = option("--capacity", 64), option("--repeat", 8)
    name = argv[0] if argv else "syn-t"
    (xtr, ytr), _, (xte, yte), (ym, ys) = dataset(name)
    x, y = np.tile(xte, (repeat, 1)), np.tile(yte, repeat)          # several times the capacity
    print("%s: %d training points, %d test points, capacity %d (%d chunks)" % (name, len(ytr), len(y), capacity, -(-len(y) // capacity)))
    for method in ("gp", "tp"):
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
        likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
        model = SPR(kernel, likelihood, xtr, ytr, ym, ys, eps=1e-2)
        t0 = time.perf_counter()
        with model.posterior(capacity=capacity) as post:
            fit_ms = (time.perf_counter() - t0) * 1e3
            ref, ref_ms = per_call(lambda: model.test_nll(x, y))
            got, got_ms = per_call(lambda: post.test_nll(x, y))
            print("%s  model.test_nll %.6f  %7.3f ms per call    post.test_nll %.6f  %7.3f ms per call    (posterior(): %.2f ms, "
                  "%.2f MB on the device, logdet %.4f)" % (method, ref, ref_ms, got, got_ms, fit_ms, post.nbytes / 1e6, post.logdet))


if __name__ == "__main__":
    main()
