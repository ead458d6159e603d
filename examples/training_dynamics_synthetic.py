#!/usr/bin/env python3
"""Mean and 2-sigma band of the infinitely wide ensemble at one test point against training time, on the reference's offline
regression set: predict_fn(t=...) for get="nngp" (only the last layer trained) beside get="ntk" (every layer trained).

    python examples/training_dynamics_synthetic.py [syn-t|syn-normal]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from regression_synthetic import dataset                                  # noqa: E402  (the example beside this one)
from smnngp import nt_kernels, spectral                                   # noqa: E402
from smnngp.predict import gradient_descent_mse_ensemble                  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "syn-t"
    (x, y), _, (xt, yt), _ = dataset(name)
    kernel_fn = nt_kernels.get_mlp_kernel(2, act="relu", w_std=1.5, b_std=0.5, last_w_std=1.0)
    predict_fn = gradient_descent_mse_ensemble(kernel_fn, x, y[:, None], diag_reg=1e-3)
    times = np.concatenate([[0.0], np.logspace(0, 6, 13), [np.inf]])
    point = 0
    out = {}
    for get in ("nngp", "ntk"):
        res = predict_fn(t=times, x_test=xt, get=get, compute_cov=True)
        mean, cov = res
        out[get] = (mean[:, point, 0], 2.0 * np.sqrt(np.maximum(cov[:, point, point], 0.0)), res.evals)
    print("%s: N = %d, test point x* = %.3f, target %.3f" % (name, x.shape[0], xt[point, 0], yt[point]))
    for get in ("nngp", "ntk"):
        lam = out[get][2]
        print("  %-4s spectrum of the regularised train kernel: %.3e ... %.3e, largest stable learning rate %.3g"
              % (get, lam[0], lam[-1], spectral.max_learning_rate(lam, y.size)))
    print("%12s | %10s %10s | %10s %10s" % ("t", "nngp mean", "2 sigma", "ntk mean", "2 sigma"))
    for j, t in enumerate(times):
        print("%12g | %10.4f %10.4f | %10.4f %10.4f" % (t, out["nngp"][0][j], out["nngp"][1][j], out["ntk"][0][j], out["ntk"][1][j]))
    none = predict_fn(x_test=xt, get="nngp")
    print("t = None (the factorisation path), nngp mean at x*: %.4f" % float(np.asarray(none[0])[point, 0]))


if __name__ == "__main__":
    main()
