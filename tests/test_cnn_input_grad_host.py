"""Host-side checks of the inducing-image gradient (no GPU): the reverse-mode rules the GPU tests compare
csrc/cnn_input_grad.hip against (tests/_cnn_input_grad_rules.py) agree with central differences of the fp64 reference kernel
and of the ELBO rules' own loss; the C-ABI entry exists and rejects a NULL context; train_svsp selects and accepts the
inducing images."""
import ctypes as C

import numpy as np
import pytest

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)

import _cnn_input_grad_rules as G  # noqa: E402
import _svsp_elbo_rules as E  # noqa: E402
import _svsp_rules as R  # noqa: E402

TOL = 1e-6           # of max|gradient|: the TOL of test_svsp_elbo_host.py
HYP = dict(w_std=1.3, last_w_std=0.9)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


def _probes(rng, shape, count=12):
    return [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(count)]


# ----------------------------------------------------------------------------- 1. the rules against the oracle kernel
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("n,h,w,c,layers,b_std", [(5, 5, 6, 2, 3, 0.4), (4, 4, 4, 1, 2, 0.0), (6, 8, 8, 3, 4, 0.1)])
def test_rules_against_central_differences_of_the_oracle_kernel(n, h, w, c, layers, b_std, act):
    """sum_ab g_ab K_ab(x) differentiated with respect to a dozen random pixels: step 1e-5, 1e-6 of max|gx|."""
    rng = np.random.default_rng([n, h, w, c, layers])
    x = rng.standard_normal((n, h, w, c))
    g = rng.standard_normal((n, n))
    g = g + g.T
    gx, s = G.input_grad(g, x, layers, act, HYP["w_std"], b_std, HYP["last_w_std"])
    assert gx.shape == x.shape and s.shape == x.shape and np.all(s >= np.abs(gx) * (1 - 1e-12))

    def f(xx):
        return float(np.sum(g * O.cnn_kernel(xx, None, layers, act, HYP["w_std"], b_std, HYP["last_w_std"])))

    step, worst = 1e-5, 0.0
    for idx in _probes(rng, x.shape):
        up, dn = x.copy(), x.copy()
        up[idx] += step; dn[idx] -= step
        fd = (f(up) - f(dn)) / (2 * step)
        worst = max(worst, abs(gx[idx] - fd) / np.max(np.abs(gx)))
    print("rules vs oracle %s %s: worst %.3e of max|gx| (tol %g)" % ((n, h, w, c, layers, b_std), act, worst, TOL))
    assert worst <= TOL


def test_rules_honour_n_grad_and_read_the_lower_triangle():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((7, 5, 5, 2))
    g = rng.standard_normal((7, 7))
    g = g + g.T
    full, s_full = G.input_grad(g, x, 2, "relu", 1.3, 0.2, 0.9)
    part, s_part = G.input_grad(np.tril(g) + 99.0 * np.triu(np.ones((7, 7)), 1), x, 2, "relu", 1.3, 0.2, 0.9, n_grad=3)
    assert part.shape == (3, 5, 5, 2)
    assert np.allclose(part, full[:3], rtol=1e-13, atol=0) and np.allclose(s_part, s_full[:3], rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------- 2. the rules against the ELBO rules
I, B, CLS, S, N = 12, 8, 3, 16, 500


@pytest.mark.parametrize("student", [False, True], ids=["svgp", "svtp"])
def test_rules_fed_gbar_against_central_differences_of_the_elbo(student):
    """d loss / d Z = the reverse-mode rules applied to the ELBO rules' Gbar, against central differences of the ELBO rules'
    own loss with K rebuilt from the perturbed inducing images: step 1e-4, 1e-6 of max|g|."""
    fx = R.fixture(num_inducing=I, num_test=B, num_class=CLS, hw=6, seed=9)
    kw = fx["kernel"]
    kfn = R.kernel_fn("cnn", **kw)
    a, b = (1.7, 2.3) if student else (None, None)
    pt = E.prior_terms(a, b, 2.0, 3.0)
    xi, dxi = E.variates(5, pt["df"], 3, B, CLS, S)
    eps = 1e-3

    def loss(z):
        nll, kl_n = E.forward(kfn(np.concatenate([z, fx["x"]])), I, fx["q_mu"], fx["q_var"], eps, pt["s"], N, fx["y"], xi,
                              pt["scale"])
        return nll + kl_n

    u = np.concatenate([fx["z"], fx["x"]])
    res = E.elbo(kfn(u), I, fx["q_mu"], fx["q_var"], eps, pt["s"], N, fx["y"], xi, pt["scale"], dxi)
    gz, _ = G.input_grad(res["gbar"], u, kw["num_hiddens"], kw["act"], kw["w_std"], kw["b_std"], kw["last_w_std"], n_grad=I)
    assert gz.shape == fx["z"].shape
    rng = np.random.default_rng(17)
    step, worst = 1e-4, 0.0
    for idx in _probes(rng, fx["z"].shape):
        up, dn = fx["z"].copy(), fx["z"].copy()
        up[idx] += step; dn[idx] -= step
        fd = (loss(up) - loss(dn)) / (2 * step)
        worst = max(worst, abs(gz[idx] - fd) / np.max(np.abs(gz)))
    print("rules vs ELBO %s: worst %.3e of max|g| (tol %g)" % ("svtp" if student else "svgp", worst, TOL))
    assert worst <= TOL


# ----------------------------------------------------------------------------- 3. exports and host wiring
def test_library_exports_the_input_gradient_entry_and_it_rejects_a_null_context(lib):
    raw = C.CDLL(lib.LIB_PATH)
    assert hasattr(raw, "smn_kernel_cnn_input_grad"), "libsmnngp.so does not export smn_kernel_cnn_input_grad"
    assert "smn_kernel_cnn_input_grad" in lib.PROTOTYPES
    rc = lib._lib.smn_kernel_cnn_input_grad(None, lib.F64, 0, 1, 1.0, 0.1, 1.0, None, 4, 4, 4, 1, None, 4, 2, None)
    assert rc == lib.EINVAL


def _tiny_model(lib, student):
    from smnngp.nt_kernels import get_cnn_kernel
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    kernel = NNGPKernel(lambda w, b, l: get_cnn_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.1, 1.0)
    return SVSP(InverseGammaPrior(2.0, 3.0) if student else GaussianPrior(), kernel, np.zeros((4, 6, 6, 1)), num_latent_gps=3)


@pytest.mark.parametrize("student", [False, True], ids=["svgp", "svtp"])
def test_train_vars_select_the_inducing_images_on_request(lib, student):
    from smnngp import train_svsp as TS
    model = _tiny_model(lib, student)
    default = TS.svsp_train_vars(model)
    chosen = TS.svsp_train_vars(model, inducing=True)
    assert not any("inducing_variable" in k for k in default)
    extra = set(chosen) - set(default)
    assert len(extra) == 1 and "inducing_variable" in next(iter(extra))
    assert chosen[next(iter(extra))] is model.inducing_variable
    assert any("last_w_std" in k for k in chosen) == (not student)


def test_train_step_accepts_the_inducing_images(lib):
    from smnngp import train_svsp as TS
    model = _tiny_model(lib, False)
    variables = TS.svsp_train_vars(model, inducing=True)
    step = TS.build_svsp_train_step(model, variables, num_train=100, num_samples=4)
    assert step.variables is variables and any("inducing_variable" in k for k in step.variables)
