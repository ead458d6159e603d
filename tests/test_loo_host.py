"""Leave-one-out cross-validation, host side: the closed forms of tests/_loo_rules.py against the definition (deleting the
point), the seed G and every trainable's gradient against central differences, the C-ABI of the four new entries and the
routing of the Python layer.  No GPU."""
import os
import re

import numpy as np
import pytest

import _loo_rules as LR
import _multi_rules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scale-mixtures-of-neural-network-gaussian-processes_amd")
ENTRIES = ("smn_loo_head", "smn_loo_multi", "smn_spr_loo_grad", "smn_spr_cnn_loo_grad")
HEAD = dict(alpha=1.7, beta=2.4)


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_closed_forms_equal_deleting_the_point(n, c, method):
    kt, _, y, _ = LR.spd_case(n, c)
    r = LR.from_matrix(kt, y, method, **HEAD)
    want = LR.brute(kt, y, method, **HEAD)
    # both sides are fp64 evaluations of O(1) log-densities through a solve with cond <= 30: 1e-12 is ~100 roundings
    assert np.max(np.abs(r["lp"] - want)) < 1e-12 * max(1.0, np.max(np.abs(want)))
    assert abs(r["lam"] - want.sum()) < 1e-12 * max(1.0, abs(want.sum()))
    for i in range(n):
        mu, var = LR.brute_moments(kt, y, i)
        assert np.max(np.abs(r["mean"][i] - mu)) < 1e-12 * max(1.0, np.max(np.abs(y)))
        if method == "gp":
            assert abs(r["scale2"][i] - var) < 1e-12 * var
        else:                                    # the t conditional rescales the Gaussian variance by (nu + Q_-i / s) / nu'
            nu, s = 2.0 * HEAD["alpha"], HEAD["beta"] / HEAD["alpha"]
            keep = np.arange(n) != i
            q_rest = float(np.sum(y[keep] * np.linalg.solve(kt[np.ix_(keep, keep)], y[keep]))) if n > 1 else 0.0
            assert abs(r["scale2"][i] - (nu + q_rest / s) / (nu + (n - 1) * c) * s * var) < 1e-11 * var
    if method == "tp":
        assert r["df"] == 2.0 * HEAD["alpha"] + (n - 1) * c
        if n == 1:                               # the prior predictive: nothing is left to condition on
            assert abs(r["q"] - r["e"][0]) < 1e-14 * r["q"]


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3])
def test_seed_against_central_differences(c, method):
    n = 9
    kt, _, y, _ = LR.spd_case(n, c)
    rng = np.random.default_rng(5)
    e = rng.standard_normal((n, n))
    e = 0.5 * (e + e.T)
    h = 1e-5
    fd = (LR.from_matrix(kt + h * e, y, method, **HEAD)["lam"] - LR.from_matrix(kt - h * e, y, method, **HEAD)["lam"]) / (2 * h)
    r = LR.from_matrix(kt, y, method, **HEAD)
    got = float(np.sum(r["g"] * e))
    # central differences: truncation h^2 |f'''| ~ 1e-10 and rounding 1e-16 |Lambda| / h ~ 1e-10, relative to |got| = O(1..10)
    assert abs(got - fd) < 1e-7 * max(1.0, abs(fd))
    assert np.max(np.abs(r["g"] - r["g"].T)) < 1e-12 * np.max(np.abs(r["g"]))
    assert np.all(np.abs(r["g"]) <= r["g_abs"] * (1 + 1e-12))
    # d Lambda / d(df, scale)
    for k, (da, db) in enumerate(((1.0, 0.0), (0.0, 1.0))):
        if method == "gp":
            assert r["dhead"][k] == 0.0
            continue
        nu, s = 2.0 * HEAD["alpha"], HEAD["beta"] / HEAD["alpha"]

        def lam(nu_, s_):
            return LR.from_matrix(kt, y, "tp", alpha=nu_ / 2.0, beta=s_ * nu_ / 2.0)["lam"]
        fdh = (lam(nu + h * da, s + h * db) - lam(nu - h * da, s - h * db)) / (2 * h)
        assert abs(r["dhead"][k] - fdh) < 1e-7 * max(1.0, abs(fdh))


CASES = [("mlp", "relu", ("dense", 20, 3)), ("mlp", "erf", ("dense", 20, 1)), ("resnet", "relu", ("dense", 20, 3)),
         ("cnn", "relu", ("conv", 12, 3, 6, 6, 2))]


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,data_key", CASES)
def test_loss_gradients_against_central_differences(family, act, data_key, method):
    x, y = M.DATA[data_key[0]](*data_key[1:])[:2]
    _, grads, _, _ = LR.loss_grad(family, x, y, 2, act, method, **M.HYP)
    keys = LR.KEYS if method == "tp" else LR.KEYS[:4]
    fd, fd_2h, fd_h2 = (LR.loss_fd(family, x, y, 2, act, method, keys, h=h, **M.HYP) for h in (1e-4, 2e-4, 5e-5))
    assert set(grads) == set(keys)
    for k in keys:
        # the differences' own error is the floor: doubling the step moves the quotient by 3x its truncation error, halving
        # it shows its rounding noise (which only grows as the step shrinks).  Each is ONE sample of that error, not a bound
        # on it: four times the sample
        floor = 4.0 * abs(fd[k] - fd_2h[k]) + 4.0 * abs(fd[k] - fd_h2[k]) + 1e-12 * abs(fd[k])
        assert abs(grads[k] - fd[k]) <= floor, (k, grads[k], fd[k], floor)
        assert floor < 1e-4 * max(abs(v) for v in fd.values()), (k, floor)      # ... and that floor means something


def test_abi_declares_and_binds_the_entries():
    header = open(os.path.join(ROOT, "include", "smnngp.h")).read()
    lib_py = open(os.path.join(PKG, "_lib.py")).read()
    build_py = open(os.path.join(PKG, "build.py")).read()
    assert '"loo.hip"' in build_py and os.path.exists(os.path.join(PKG, "csrc", "loo.hip"))
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/smnngp.h" % name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        b = re.search(r'"%s":\s*\[([^\]]*)\]' % name, lib_py)
        assert b, "%s is not bound in _lib.py" % name
        assert len([a for a in b.group(1).split(",") if a.strip()]) == nargs, name
    from smnngp import _lib
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(_lib._lib, name)


class _NoDevice:
    """Stands in for a model in the routing tests: nothing here may reach the device."""

    def __init__(self, kernel_fn, likelihood):
        self._kernel_fn, self.likelihood = kernel_fn, likelihood
        self.kernel = self

    def get_kernel_fn(self):
        return self._kernel_fn


def test_conv_resnet_and_unknown_likelihood_raise_from_loo_loss_and_grad():
    from smnngp import nt_kernels
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    resnet = nt_kernels.get_conv_resnet_kernel(1, 10)
    for cls in (SPR, MultiSPR):
        with pytest.raises(NotImplementedError):
            cls.loo_loss_and_grad(_NoDevice(resnet, GaussianLikelihood()))
        with pytest.raises(NotImplementedError):
            cls.loo_loss_and_grad(_NoDevice(nt_kernels.get_mlp_kernel(2), object()))
        for name in ("loo_loss", "loo_loss_and_grad", "loo_predict"):
            assert callable(getattr(cls, name))
    assert callable(MultiSPR.loo_classify) and callable(MultiSPR.loo_accuracy)


def test_build_train_step_rejects_an_unknown_objective():
    from smnngp import train
    with pytest.raises(ValueError):
        train.build_train_step(object(), variables={}, optimizer=lambda lr, g: None, objective="elbo")
    for ok in ("lml", "loo"):
        assert callable(train.build_train_step(object(), variables={}, optimizer=lambda lr, g: None, objective=ok))
