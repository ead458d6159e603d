"""Host-side checks of the sparse variational classifier's evaluation path (no GPU): the fp64 rules the GPU tests compare
against are the reference's own sequence of operations; the rules' Philox4x32-10 reproduces the published vectors; NumPy's
generator passes the statistical thresholds the device generator is held to; classification run directories parse."""
import os

import numpy as np
import pytest

import _svsp_rules as R


@pytest.mark.parametrize("eps", [1e-3, 1e-6])
def test_diagonal_only_rules_equal_the_literal_sequence(eps):
    """The full [B,B] covariance, einsum("ij,cjk,kl->cil") and then the diagonal (spax/models.py:66-74) against the
    diagonal-only form the device computes: 1e-12."""
    fx = R.fixture(num_test=48)
    kfn = R.kernel_fn("cnn", **fx["kernel"])
    m0, v0 = R.moments_literal(kfn, fx["z"], fx["x"], fx["q_mu"], fx["q_var"], eps)
    m1, v1 = R.moments_diag(kfn, fx["z"], fx["x"], fx["q_mu"], fx["q_var"], eps)
    assert m0.shape == m1.shape == (48, 4) and v0.shape == v1.shape
    assert np.max(np.abs(m0 - m1)) <= 1e-12 * max(1.0, np.max(np.abs(m0)))
    assert np.max(np.abs(v0 - v1)) <= 1e-12 * max(1.0, np.max(np.abs(v0)))
    assert (v0 > 0).all()


def test_fixture_is_what_the_gpu_tests_assume():
    fx = R.fixture()
    kfn = R.kernel_fn("cnn", **fx["kernel"])
    k_zz = kfn(fx["z"])
    for eps in (1e-3, 1e-6):
        cond = np.linalg.cond(k_zz + eps * np.trace(k_zz) / 40 * np.eye(40))
        print("cond(K_rel) at eps = %g: %.1f" % (eps, cond))
        assert 50 < cond < 1000
    assert fx["z"].shape == (40, 8, 8, 1) and fx["x"].shape == (256, 8, 8, 1) and set(fx["y"]) == {0, 1, 2, 3}


def test_philox_known_answers():
    for ctr, key, out in R.PHILOX_KAT:
        assert tuple(R.philox4x32_10(ctr, key)) == out


@pytest.mark.parametrize("df", [0.0, 1.0, 4.0, 9.3])
def test_numpy_generator_passes_the_thresholds_of_the_device_generator(df):
    rng = np.random.default_rng(11)
    shape = (64, 4, 4096)
    xi = rng.standard_normal(shape) if df <= 0 else rng.standard_t(df, shape)
    n, d, cors = R.variate_statistics(xi, df)
    print("df %g: KS D sqrt(N) = %.3f" % (df, d * np.sqrt(n)), {k: round(v * np.sqrt(n), 3) for k, v in cors.items()})
    assert n == 2 ** 20 and d < 1.95 / np.sqrt(n)
    for name, c in cors.items():
        assert c < 5 / np.sqrt(n), (name, c)


def test_head_rules_on_a_hand_case():
    """C = 1: log-softmax is 0, so ll = 0 and score = log S; two classes, one draw: ll = log sigmoid."""
    ll, score, pred = R.head(np.zeros((3, 1)), np.ones((3, 1)), [0, 0, 0], np.random.default_rng(0).standard_normal((3, 1, 5)))
    assert np.all(ll == 0.0) and np.allclose(score, np.log(5)) and np.all(pred == 0)
    ll, score, pred = R.head(np.array([[1.0, -1.0]]), np.zeros((1, 2)), [0], np.zeros((1, 2, 1)))
    assert ll[0] == pytest.approx(-np.log1p(np.exp(-2.0)), abs=1e-15) and pred[0] == 0


def _write_run(d, method, with_last_w_std, index=12):
    """A classification run directory in the objax layout: `names` + "0", "1", ..., pickled meta.npy."""
    rng = np.random.default_rng(3)
    names = ["(SVSP).kernel(NNGPKernel).w_std", "(SVSP).kernel(NNGPKernel).b_std", "(SVSP).inducing_variable",
             "(SVSP).q_mu", "(SVSP).q_sqrt", "(SVSP).eps"]
    vals = [np.array(0.4, np.float32), np.array(-2.0, np.float32), rng.standard_normal((6, 8, 8, 1)).astype(np.float32),
            rng.standard_normal((3, 6)).astype(np.float32), rng.standard_normal((3, 6)).astype(np.float32),
            np.array(-3.0, np.float32)]
    if with_last_w_std:
        names.append("(SVSP).kernel(NNGPKernel).last_w_std"); vals.append(np.array(0.7, np.float32))
    if method == "svtp":
        names += ["(SVSP).prior(InverseGammaPrior).a", "(SVSP).prior(InverseGammaPrior).b"]
        vals += [np.array(1.1, np.float32), np.array(0.6, np.float32)]
    os.makedirs(d, exist_ok=True)
    np.savez(os.path.join(d, "%03d.npz" % index), names=np.array(names), **{str(i): v for i, v in enumerate(vals)})
    args = dict(method=method, network="cnn", num_hiddens=2, activation="relu", last_w_std=1.5, alpha=2.0, beta=3.0)
    np.save(os.path.join(d, "meta.npy"), args)             # classification/train.py:247: vars(args) itself, no "args" wrapper
    return dict(zip([n.split(".")[-1] for n in names], vals))


@pytest.mark.parametrize("method", ["svgp", "svtp"])
@pytest.mark.parametrize("with_last_w_std", [True, False])
def test_read_svsp_run(tmp_path, method, with_last_w_std):
    from smnngp import checkpoint as CK
    d = str(tmp_path / "run")
    stored = _write_run(d, method, with_last_w_std)
    raw, ctx = CK.read_svsp_run(d)
    assert ctx["method"] == method and ctx["network"] == "cnn"
    for k in ("w_std", "b_std", "inducing_variable", "q_mu", "q_sqrt", "eps"):
        assert np.array_equal(raw[k], stored[k]), k
    assert float(raw["last_w_std"]) == (pytest.approx(0.7) if with_last_w_std else 1.5)     # absent: from the run's arguments
    if method == "svtp":
        assert float(raw["a"]) == pytest.approx(1.1) and float(raw["b"]) == pytest.approx(0.6)
    else:
        assert raw["a"] is None and raw["b"] is None
    assert CK.read_svsp_run(d, 12)[0]["q_mu"].shape == (3, 6)
    assert "args" not in np.load(os.path.join(d, "meta.npy"), allow_pickle=True).item()   # the flat layout of test.py:84
    np.save(os.path.join(d, "meta.npy"), dict(args=ctx))                                  # the regression wrapper is accepted too
    assert CK.read_svsp_run(d)[1] == ctx
    with pytest.raises(FileNotFoundError):
        CK.read_svsp_run(d, 13)


def test_restore_svsp_builds_the_model_without_a_device(tmp_path):
    """Nothing in restore_svsp touches the GPU: the model holds host variables until it is evaluated.  eps: test.py never
    restores it (the constructor default 1e-6 is what it evaluates at); "stored" and a float override that."""
    from smnngp import checkpoint as CK
    from smnngp.spax.bijectors import positive
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    d = str(tmp_path / "run")
    stored = _write_run(d, "svtp", False)
    model, ctx = CK.restore_svsp(d)
    assert isinstance(model.prior, InverseGammaPrior) and model.num_latent_gps == 3 and model.num_inducing == 6
    assert model.eps.safe_value == pytest.approx(1e-6, rel=1e-9)                           # stored -3.0 is ignored
    assert model.prior.a.safe_value == pytest.approx(float(positive()(1.1)), rel=1e-6)
    assert model.prior.alpha == 2.0 and model.prior.beta == 3.0
    assert model.kernel.get_params()[2] == pytest.approx(float(positive()(1.5)))           # the argument, taken as raw
    assert np.array_equal(model.q_mu.value, stored["q_mu"].astype(np.float64))
    assert model.prior.head_params()[0] == pytest.approx(2 * model.prior.a.safe_value)
    assert CK.restore_svsp(d, eps="stored")[0].eps.safe_value == pytest.approx(float(positive()(-3.0)), rel=1e-6)
    assert CK.restore_svsp(d, eps=1e-3)[0].eps.safe_value == pytest.approx(1e-3, rel=1e-9)
    names = {n.split(".")[-1] for n in model.vars()}
    assert {"inducing_variable", "q_mu", "q_sqrt", "eps", "w_std", "b_std", "last_w_std", "a", "b"} <= names
    _write_run(str(tmp_path / "g"), "svgp", True)
    assert isinstance(CK.restore_svsp(str(tmp_path / "g"))[0].prior, GaussianPrior)
    with pytest.raises(NotImplementedError):
        model.loss(0, None, None, 1, 1)
    with pytest.raises(NotImplementedError):
        model.prior.sample_f(0, None, None, 1)
    with pytest.raises(NotImplementedError):
        model.prior.kl_divergence(None, None, None, None, 6, 3)
