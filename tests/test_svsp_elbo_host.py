"""Host-side checks of the SVSP training path (no GPU): every analytic gradient of the fp64 rules the GPU tests compare
against agrees with central differences of the rules' own loss; the names the evaluation tests pin still raise next to
a working loss_and_grad; the array-valued Adam of train_svsp takes the step objax's Adam takes."""
import numpy as np
import pytest

import _svsp_elbo_rules as E
import _svsp_rules as R

I, B, C, S, N = 12, 8, 3, 16, 500
TOL = 1e-6


def _problem(student):
    fx = R.fixture(num_inducing=I, num_test=B, num_class=C, hw=6, seed=9)
    kfn = R.kernel_fn("cnn", **fx["kernel"])
    K = kfn(np.concatenate([fx["z"], fx["x"]]))
    a, b = (1.7, 2.3) if student else (None, None)
    return dict(K=K, q_mu=fx["q_mu"], q_var=fx["q_var"], y=fx["y"], eps=1e-3, a=a, b=b, alpha=2.0, beta=3.0, fx=fx, kfn=kfn)


def _loss(p, K=None, q_mu=None, q_var=None, eps=None, a=None, b=None):
    a, b = (p["a"] if a is None else a), (p["b"] if b is None else b)
    pt = E.prior_terms(a, b, p["alpha"], p["beta"])
    xi, _ = E.variates(5, pt["df"], 3, B, C, S)
    nll, kl_n = E.forward(p["K"] if K is None else K, I, p["q_mu"] if q_mu is None else q_mu,
                          p["q_var"] if q_var is None else q_var, p["eps"] if eps is None else eps, pt["s"], N, p["y"], xi,
                          pt["scale"])
    return nll + kl_n + pt["kl_extra"] / N


def _grads(p):
    pt = E.prior_terms(p["a"], p["b"], p["alpha"], p["beta"])
    xi, dxi = E.variates(5, pt["df"], 3, B, C, S)
    return E.elbo(p["K"], I, p["q_mu"], p["q_var"], p["eps"], pt["s"], N, p["y"], xi, pt["scale"], dxi), pt


def _check(name, analytic, fd):
    err = abs(analytic - fd) / max(abs(fd), 1e-300)
    print("%-28s analytic % .12e  central % .12e  rel %.2e" % (name, analytic, fd, err))
    assert err <= TOL, name


@pytest.mark.parametrize("student", [False, True], ids=["svgp", "svtp"])
def test_rules_gradients_against_central_differences(student):
    p = _problem(student)
    res, pt = _grads(p)
    assert np.array_equal(res["gbar"], res["gbar"].T)
    for c, i in [(0, 0), (1, 5), (2, 11)]:
        for key, g, h in (("q_mu", res["g_q_mu"], 1e-5), ("q_var", res["g_q_var"], 1e-6)):
            up, dn = p[key].copy(), p[key].copy()
            up[c, i] += h; dn[c, i] -= h
            _check("%s[%d,%d]" % (key, c, i), g[c, i], (_loss(p, **{key: up}) - _loss(p, **{key: dn})) / (2 * h))
    h = 1e-7
    _check("eps", res["g_eps"], (_loss(p, eps=p["eps"] + h) - _loss(p, eps=p["eps"] - h)) / (2 * h))
    # entry-wise probes of K: both diagonals and all three blocks (a symmetric perturbation moves K_ij and K_ji)
    U = I + B
    probes = [(2, 2), (I + 3, I + 3), (7, 1), (I + 5, I + 2), (I + 1, 4), (I + 6, 10)]
    for (i, j) in probes:
        h = 1e-6
        d = np.zeros((U, U)); d[i, j] = h; d[j, i] = h
        want = (_loss(p, K=p["K"] + d) - _loss(p, K=p["K"] - d)) / (2 * h)
        _check("K[%d,%d]" % (i, j), res["gbar"][i, j] + (res["gbar"][j, i] if i != j else 0.0), want)
    # kernel hyper-parameters: sum Gbar * central-difference dK
    for name in ("w_std", "b_std", "last_w_std"):
        h = 1e-6
        kw = dict(p["fx"]["kernel"])
        u = np.concatenate([p["fx"]["z"], p["fx"]["x"]])
        ku = R.kernel_fn("cnn", **{**kw, name: kw[name] + h})(u)
        kd = R.kernel_fn("cnn", **{**kw, name: kw[name] - h})(u)
        _check(name, float(np.sum(res["gbar"] * (ku - kd) / (2 * h))), (_loss(p, K=ku) - _loss(p, K=kd)) / (2 * h))
    if student:
        g_a, g_b = E.prior_grads(res, pt, p["a"], p["b"], N)
        h = 1e-6
        _check("a", g_a, (_loss(p, a=p["a"] + h) - _loss(p, a=p["a"] - h)) / (2 * h))
        _check("b", g_b, (_loss(p, b=p["b"] + h) - _loss(p, b=p["b"] - h)) / (2 * h))


def test_bailey_derivative_and_limit():
    """d t / d df against a central difference at fixed (u, v); the bracket tends to 0 as w -> 1."""
    for draw in range(6):
        t, dt = E.bailey(11, 4, 1, draw, 4.0)
        h = 1e-5
        fd = (E.bailey(11, 4, 1, draw, 4.0 + h)[0] - E.bailey(11, 4, 1, draw, 4.0 - h)[0]) / (2 * h)
        assert abs(dt - fd) <= 1e-8 * max(abs(fd), 1e-3), (draw, dt, fd)


def test_cholesky_reverse_on_a_hand_case():
    """1 x 1: S = l^2, loss = g l  ->  d loss / d S = g / (2 l)."""
    assert E.cholesky_reverse(np.array([[2.0]]), np.array([[3.0]]))[0, 0] == pytest.approx(0.75, abs=1e-15)


def test_pinned_names_still_raise_next_to_loss_and_grad():
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.nt_kernels import get_cnn_kernel
    kernel = NNGPKernel(lambda w, b, l: get_cnn_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.1, 1.0)
    model = SVSP(InverseGammaPrior(2.0, 3.0), kernel, np.zeros((4, 6, 6, 1)), num_latent_gps=3)
    assert callable(getattr(model, "loss_and_grad"))
    with pytest.raises(NotImplementedError, match="loss_and_grad"):
        model.loss(0, None, None, 1, 1)
    with pytest.raises(NotImplementedError, match="loss_and_grad"):
        model.prior.sample_f(0, None, None, 1)
    with pytest.raises(NotImplementedError, match="loss_and_grad"):
        GaussianPrior().kl_divergence(None, None, None, None, 4, 3)


def test_prior_terms_of_the_package_equal_the_rules():
    """InverseGammaPrior.elbo_params (host arithmetic of SVSP.loss_and_grad) against the rules' scipy form."""
    from smnngp.spax.bijectors import positive
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    from smnngp.spax.utils import trigamma
    from scipy.special import polygamma
    for x in (0.05, 0.5, 1.0, 2.5, 9.99, 10.0, 123.4):
        assert abs(trigamma(x) - polygamma(1, x)) < 1e-12 * max(1.0, abs(polygamma(1, x)))
    prior = InverseGammaPrior(2.0, 3.0)
    prior.a.assign(positive().inverse(1.7)); prior.b.assign(positive().inverse(2.3))
    got, want = prior.elbo_params(), E.prior_terms(prior.a.safe_value, prior.b.safe_value, 2.0, 3.0)
    for k in ("df", "scale", "s", "kl_extra"):
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert got["d_extra"]["a"] == pytest.approx(want["d_extra_a"], rel=1e-11)
    assert got["d_extra"]["b"] == pytest.approx(want["d_extra_b"], rel=1e-11)
    assert GaussianPrior().elbo_params() == dict(df=0.0, scale=1.0, s=1.0, kl_extra=0.0, d_extra={})


def test_array_adam_takes_the_hand_computed_step():
    from smnngp.train_svsp import ArrayAdam
    opt = ArrayAdam(beta1=0.9, beta2=0.999, eps=1e-8)
    x = {"v": np.array([1.0, -2.0]), "s": 0.5}
    g = {"v": np.array([0.1, -0.4]), "s": 2.0}
    new = opt.step(x, g, lr=0.01)
    # first step: m = (1 - b1) g, v = (1 - b2) g^2; lr_t = lr sqrt(1 - b2) / (1 - b1); x -= lr_t m / (sqrt(v) + eps)
    for key in x:
        gg = np.asarray(g[key], dtype=np.float64)
        m, v = 0.1 * gg, 0.001 * gg * gg
        want = np.asarray(x[key]) - 0.01 * np.sqrt(0.001) / 0.1 * m / (np.sqrt(v) + 1e-8)
        assert np.allclose(new[key], want, rtol=1e-14, atol=0)
    new2 = opt.step(new, g, lr=0.01)
    m, v = 0.19 * 2.0, 0.001999 * 4.0
    want = new["s"] - 0.01 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.81) * m / (np.sqrt(v) + 1e-8)
    assert float(new2["s"]) == pytest.approx(float(want), rel=1e-14)
