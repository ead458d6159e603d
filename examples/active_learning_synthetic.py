#!/usr/bin/env python3
"""Active learning on a growing fitted posterior: `FittedPosterior.append` on the reference's offline regression dataset.

    python examples/active_learning_synthetic.py [syn-t|syn-normal] [--budget 80] [--batch 1]

The model starts from 40 of the training points; the rest is the pool.  Each round takes the `--batch` pool points of largest
predictive variance (`post.predict(pool)`: uncertainty sampling), reads their targets and appends them to the state with
`post.append(x, y)` -- O(N^2 k), nothing is refitted and the ridge is the one frozen when the state was made (`post.ridge`).
Printed for the Gaussian (`gp`) and the Student-t (`tp`) likelihood: the test NLL after `--budget` acquisitions beside random
acquisition of the same budget, and the time of the acquisition loop beside the same loop done by refitting
(`model.posterior()` on the grown data every round).  At this size (at most a few hundred points) every call is a handful of
launches, so the two loops cost about the same: the example shows the surface; what appending buys is measured at N = 4096 and
16384 (profiles/r22_fit_append.txt).  Under `tp` the final test_nll recomputes the Student-t quadratic form over all the
points in fp64 once (see FittedPosterior.append)."""
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

START = 40


def make_model(method, x, y, ym, ys):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    return SPR(kernel, likelihood, x, y, ym, ys, eps=1e-2)


def pick(post, pool_x, free, batch, rng):
    """Indices (into the pool) of the next batch: largest predictive variance, or random when rng is given."""
    idx = np.flatnonzero(free)
    if rng is not None:
        return rng.choice(idx, size=min(batch, idx.size), replace=False)
    var = post.predict(pool_x[idx])[1].raw_numpy()
    return idx[np.argsort(-var, kind="stable")[:batch]]


def run_append(method, data, budget, batch, rng=None):
    (x0, y0), (px, py), (xte, yte), (ym, ys) = data
    free = np.ones(len(py), dtype=bool)
    t0 = time.perf_counter()
    with make_model(method, x0, y0, ym, ys).posterior(capacity=64, reserve=START + budget) as post:
        while post.num_data < START + budget and free.any():
            take = pick(post, px, free, min(batch, START + budget - post.num_data), rng)
            post.append(px[take], py[take])
            free[take] = False
        loop_ms = (time.perf_counter() - t0) * 1e3
        return post.test_nll(xte, yte), loop_ms, post.num_data


def run_refit(method, data, budget, batch):
    (x0, y0), (px, py), (xte, yte), (ym, ys) = data
    free = np.ones(len(py), dtype=bool)
    x, y = x0, y0
    t0 = time.perf_counter()
    post = make_model(method, x, y, ym, ys).posterior(capacity=64)
    while len(y) < START + budget and free.any():
        take = pick(post, px, free, min(batch, START + budget - len(y)), None)
        x, y = np.concatenate([x, px[take]]), np.concatenate([y, py[take]])
        free[take] = False
        post.close()
        post = make_model(method, x, y, ym, ys).posterior(capacity=64)     # the refit an append replaces
    loop_ms = (time.perf_counter() - t0) * 1e3
    nll = post.test_nll(xte, yte)
    post.close()
    return nll, loop_ms, len(y)


def main():
    argv = list(sys.argv[1:])

    def option(name, default):
        if name in argv:
            i = argv.index(name)
            value = int(argv[i + 1])
            del argv[i:i + 2]
            return value
        return default

    budget, batch = option("--budget", 80), max(1, option("--batch", 1))
    name = argv[0] if argv else "syn-t"
    (xtr, ytr), _, test, norm = dataset(name)
    budget = min(budget, len(ytr) - START)
    data = ((xtr[:START], ytr[:START]), (xtr[START:], ytr[START:]), test, norm)
    print("%s: %d starting points, pool of %d, budget %d in batches of %d" % (name, START, len(ytr) - START, budget, batch))
    for method in ("gp", "tp"):
        run_append(method, data, min(budget, 2 * batch), batch)                      # warm-up: workspaces, code objects
        nll_var, ms_var, n_var = run_append(method, data, budget, batch)
        nll_rnd, _, _ = run_append(method, data, budget, batch, rng=np.random.default_rng(0))
        nll_fit, ms_fit, n_fit = run_refit(method, data, budget, batch)
        print("%s  test NLL at N = %d: largest-variance %.6f   random %.6f   |   loop by append %8.2f ms   by refitting %8.2f ms "
              "(test NLL %.6f at N = %d: the refit recomputes the relative ridge at every N, the append keeps the first)"
              % (method, n_var, nll_var, nll_rnd, ms_var, ms_fit, nll_fit, n_fit))


if __name__ == "__main__":
    main()
