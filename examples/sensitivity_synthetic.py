#!/usr/bin/env python3
"""Predictive gradients: `post.predict_grad` on the reference's offline regression dataset.

    python examples/sensitivity_synthetic.py [syn-t|syn-normal] [--capacity 64]

The model is fitted once (`post = model.posterior(capacity=...)`), then `post.predict_grad(x_test)` returns d mean / d x and
d var / d x for every test point in one pass over the state.  Printed, for the Gaussian (`gp`) and the Student-t (`tp`)
likelihood: per input feature the mean |d mean / d x| over the test set (a sensitivity ranking, in target units per unit of the
feature), and at one test point the direction of steepest decrease of the predictive variance -- where the next measurement
would teach the model most about that point.  Under `tp` the predictive scale^2 is shape * var (`post.predictive_params()`), so
its gradient is shape * dvar: the direction is the same, the length is not."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.regression_synthetic import dataset                     # noqa: E402
from smnngp import nt_kernels                                         # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR                                    # noqa: E402


def main():
    argv = list(sys.argv[1:])
    capacity = 64
    if "--capacity" in argv:
        i = argv.index("--capacity")
        capacity = int(argv[i + 1])
        del argv[i:i + 2]
    name = argv[0] if argv else "syn-t"
    (xtr, ytr), _, (xte, _), (ym, ys) = dataset(name)
    print("%s: %d training points, %d test points, %d features" % (name, len(ytr), len(xte), xte.shape[1]))
    for method in ("gp", "tp"):
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
        likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
        model = SPR(kernel, likelihood, xtr, ytr, ym, ys, eps=1e-2)
        with model.posterior(capacity=capacity) as post:
            dmean, dvar = post.predict_grad(xte)
            _, shape = post.predictive_params()
            dmean = np.asarray(dmean.raw_numpy(), dtype=np.float64)[:, 0, :] * post.y_std        # target units
            dscale2 = np.asarray(dvar.raw_numpy(), dtype=np.float64) * post.y_std ** 2 * shape
        sens = np.mean(np.abs(dmean), axis=0)
        step = -dscale2[0] / max(np.linalg.norm(dscale2[0]), 1e-300)
        print("%s  mean |d mean / d x_e| per feature: %s" % (method, " ".join("%.4f" % s for s in sens)))
        print("    steepest decrease of the predictive %s at test point 0 (|gradient| %.3e): %s"
              % ("scale^2" if method == "tp" else "variance", np.linalg.norm(dscale2[0]), " ".join("%+.3f" % s for s in step)))


if __name__ == "__main__":
    main()
