"""Training step for SPR — the counterpart of experiments/regression/train.py:61-67
(`objax.GradValues(model.loss, vars)` + `objax.optimizer.Adam`) without autodiff.

The model has at most six trainable scalars (w_std, b_std, last_w_std, eps and, for the Student-t
likelihood, a, b — the names experiments/regression/test.py:38-43 matches checkpoints by), all stored
as softplus-inverse raw values (spax/base.py:15-25).  The gradient of the loss with respect to those raw
values is taken by central differences: 2 loss evaluations (= 2 fused build + Cholesky passes on the GPU)
per variable.  This is SURVEY.md section 8f.1's finite-difference fallback (use float64 data: in float32 the loss
carries ~1e-6 relative noise and the quotient is dominated by it).  The analytic form, 1/2 tr((c aa^T - K^-1)
dK/dtheta) with forward-mode dK/dtheta through the layer recursion, is SPR.loss_and_grad (csrc/grad.hip for the MLP
family, csrc/cnn_grad.hip for get_cnn_kernel); build_train_step prefers it when the model supports it.
"""
from __future__ import annotations

import math

import numpy as np

from .spax.base import TrainVar

__all__ = ["train_vars", "value_and_grad", "value_and_grad_fd", "Adam", "PlateauSchedule", "build_train_step",
           "BatchAdam", "MultiStartStep", "build_multistart_step"]


def train_vars(model):
    """Dotted-name -> TrainVar for every trainable of the model (kernel, likelihood, eps)."""
    return {k: v for k, v in model.vars().items() if isinstance(v, TrainVar)}


def value_and_grad(model, variables=None):
    """(loss, {name: dloss/draw}) from the analytic gradient (SPR.loss_and_grad): ONE augmented factorisation
    and one contraction pass instead of 2 loss evaluations per variable, and usable in float32."""
    value, grads = model.loss_and_grad()
    if variables is not None:
        grads = {k: g for k, g in grads.items() if k in variables}
    return value, grads


def value_and_grad_fd(loss_fn, variables, h=1e-4):
    """(loss, {name: dloss/draw}) by central differences on the raw (unconstrained) values; an array-valued variable
    (input_scales) component by component: 2 loss evaluations each."""
    value = float(loss_fn())
    grads = {}
    for name, var in variables.items():
        if np.ndim(var.value) > 0:
            base = np.array(var.value, dtype=np.float64)
            g = np.empty_like(base)
            for idx in np.ndindex(base.shape):
                step = h * max(1.0, abs(base[idx]))
                moved = base.copy()
                moved[idx] = base[idx] + step
                var.assign(moved)
                up = float(loss_fn())
                moved[idx] = base[idx] - step
                var.assign(moved)
                dn = float(loss_fn())
                g[idx] = (up - dn) / (2.0 * step)
            var.assign(base)
            grads[name] = g
            continue
        raw = float(var.value)
        step = h * max(1.0, abs(raw))
        var.assign(raw + step)
        up = float(loss_fn())
        var.assign(raw - step)
        dn = float(loss_fn())
        var.assign(raw)
        grads[name] = (up - dn) / (2.0 * step)
    return value, grads


class Adam:
    """objax.optimizer.Adam defaults (beta1=0.9, beta2=0.999, eps=1e-8), called as optimizer(lr, grads)."""

    def __init__(self, variables, beta1=0.9, beta2=0.999, eps=1e-8):
        self.vars, self.b1, self.b2, self.eps = variables, beta1, beta2, eps
        self.m = {k: 0.0 for k in variables}
        self.v = {k: 0.0 for k in variables}
        self.t = 0

    def __call__(self, lr, grads):
        self.t += 1
        lr_t = lr * math.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        for k, g in grads.items():
            if np.ndim(g) > 0:                    # an array-valued variable: element-wise moments, the arithmetic below
                g = np.asarray(g, dtype=np.float64)
                ok = np.isfinite(g)
                g0 = np.where(ok, g, 0.0)
                self.m[k] = np.where(ok, self.b1 * self.m[k] + (1 - self.b1) * g0, self.m[k])
                self.v[k] = np.where(ok, self.b2 * self.v[k] + (1 - self.b2) * g0 * g0, self.v[k])
                raw = np.asarray(self.vars[k].value, dtype=np.float64)
                self.vars[k].assign(np.where(ok, raw - lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps), raw))
                continue
            if not np.isfinite(g):
                continue
            self.m[k] = self.b1 * self.m[k] + (1 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1 - self.b2) * g * g
            self.vars[k].assign(float(self.vars[k].value) - lr_t * self.m[k] / (math.sqrt(self.v[k]) + self.eps))


def build_train_step(model, variables=None, optimizer=None, h=1e-4, method="auto", objective="lml"):
    """train_step(learning_rate) -> loss before the update  (regression/train.py:61-67).
    method: "analytic" (SPR.loss_and_grad), "fd" (central differences) or "auto" (analytic when the model's
    kernel / likelihood support it -- MLP, dense-ResNet and get_cnn_kernel kernels with images of up to 1024 pixels --
    else finite differences: the conv ResNet, the pooled conv kernel, larger images).  A LowRankSPR is trained analytically
    once its pivots are frozen (model.freeze_pivots(); the gradient holds them fixed, refresh_pivots() re-selects them between
    steps) and by central differences otherwise.
    objective: "lml" (the negative log-marginal likelihood: model.loss / model.loss_and_grad) or "loo" (the negative
    leave-one-out predictive log-probability: model.loo_loss / model.loo_loss_and_grad)."""
    if method not in ("auto", "analytic", "fd"):
        raise ValueError("method must be 'auto', 'analytic' or 'fd'")
    if objective not in ("lml", "loo"):
        raise ValueError("objective must be 'lml' or 'loo'")
    loo = objective == "loo"
    variables = variables if variables is not None else train_vars(model)
    optimizer = optimizer or Adam(variables)
    state = {"analytic": method != "fd" and hasattr(model, "loo_loss_and_grad" if loo else "loss_and_grad")}

    def train_step(learning_rate):
        if state["analytic"]:
            try:
                if loo:
                    value, grads = model.loo_loss_and_grad()
                    grads = {k: g for k, g in grads.items() if k in variables}
                else:
                    value, grads = value_and_grad(model, variables)
            except NotImplementedError:
                if method == "analytic":
                    raise
                state["analytic"] = False
        if not state["analytic"]:
            value, grads = value_and_grad_fd(model.loo_loss if loo else model.loss, variables, h=h)
        optimizer(learning_rate, grads)
        return value

    return train_step


class BatchAdam:
    """Adam over G independent starts: `raw` maps each variable name to an array of G raw values, updated in place
    element by element with the arithmetic of Adam above (same defaults, same order of operations, so start g moves
    exactly as a single-start run from the same value would).  Entries whose gradient is not finite are left alone, with
    their moments, as Adam leaves a variable with a non-finite gradient alone; the step count is shared."""

    def __init__(self, raw, beta1=0.9, beta2=0.999, eps=1e-8):
        self.raw, self.b1, self.b2, self.eps = raw, beta1, beta2, eps
        self.m = {k: np.zeros_like(v) for k, v in raw.items()}
        self.v = {k: np.zeros_like(v) for k, v in raw.items()}
        self.t = 0

    def __call__(self, lr, grads):
        self.t += 1
        lr_t = lr * math.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        for k, g in grads.items():
            ok = np.isfinite(g)
            g0 = np.where(ok, g, 0.0)
            m = self.b1 * self.m[k] + (1 - self.b1) * g0
            v = self.b2 * self.v[k] + (1 - self.b2) * g0 * g0
            self.m[k] = np.where(ok, m, self.m[k])
            self.v[k] = np.where(ok, v, self.v[k])
            self.raw[k][...] = np.where(ok, self.raw[k] - lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps), self.raw[k])


class MultiStartStep:
    """G training runs of one SPR model from G initialisations, advanced together: step(lr) makes ONE batched device call
    (sweeps.loss_and_grad_batch -> smn_spr_loss_grad_batch, grid.y = G) for all starts, turns each start's terms into
    d loss / d raw by the host arithmetic of SPR.loss_and_grad (spax.models.lml_value_and_grads, softplus chain rule;
    Student-t: df = 2a, scale = b/a per start) and applies Adam element-wise.  The log-marginal likelihood is not convex in
    the hyper-parameters; at the reference's problem sizes one start leaves the chip idle, so G starts cost about what one
    does.

    .raw       name -> array[G] of raw (unconstrained) values, names as in model.vars()
    .losses    the losses of the last step (before its update); NaN marks a start whose matrix was not positive definite:
               it is left where it is (and keeps reporting NaN) and does not disturb the others
    .best()    index of the lowest finite loss
    .assign_best()  writes that start into the model's variables, so that test_nll and Checkpointer work as before"""

    def __init__(self, model, starts, optimizer=None):
        from . import _lib
        from .spax.models import grad_route
        if getattr(model.kernel, "input_scales", None) is not None:
            raise NotImplementedError("multi-start training under input scales is not implemented: the batched gradient entry "
                                      "has no input-scale form; use build_train_step per start")
        kernel_fn = model.kernel.get_kernel_fn()
        if grad_route(kernel_fn, model.likelihood) != "smn_spr_loss_grad":
            raise NotImplementedError("multi-start training supports the MLP and dense-ResNet kernels only")
        self.model = model
        self.variables = train_vars(model)
        if set(starts) != set(self.variables):
            raise ValueError("starts must name every trainable of the model: %s" % sorted(self.variables))
        self.raw = {k: np.array(starts[k], dtype=np.float64).reshape(-1) for k in self.variables}
        sizes = {v.size for v in self.raw.values()}
        if len(sizes) != 1 or min(sizes) < 1:
            raise ValueError("every entry of starts needs the same number G >= 1 of raw values")
        self.num_starts = sizes.pop()
        net, act, self._layers = kernel_fn.params[:3]
        if net & _lib.NET_NTK:   # what smn_spr_loss_grad_batch answers with SMN_ENOTSUP (sweeps.loss_and_grad_batch, covariance="ntk")
            raise NotImplementedError("multi-start training on the tangent kernel (NTKKernel) is not implemented: the batched "
                                      "gradient entry has no SMN_NET_NTK form; use build_train_step per start")
        self._network = "mlp" if net == _lib.NET_MLP else "resnet"
        self._activation = {v: k for k, v in _lib.ACT.items()}[act]
        owners = {"w_std": model.kernel.w_std, "b_std": model.kernel.b_std, "last_w_std": model.kernel.last_w_std, "eps": model.eps}
        self._student = model.likelihood.lml_params()[0] > 0.0
        if self._student:
            owners.update(a=model.likelihood.a, b=model.likelihood.b)
        names = {id(v): k for k, v in model.vars().items()}
        self._name = {key: names[id(var)] for key, var in owners.items()}     # "w_std" -> "(SPR).kernel(NNGPKernel).w_std"
        self._var = owners
        self.optimizer = optimizer or BatchAdam(self.raw)
        self.losses = np.full(self.num_starts, np.nan)

    def _constrained(self, key):
        var = self._var[key]
        return np.asarray(var.constraint(self.raw[self._name[key]]), dtype=np.float64)

    def value_and_grad(self):
        """(losses[G], {name: d loss / d raw [G]}) at the current raw values: one batched device call."""
        from . import sweeps
        from .spax.models import lml_value_and_grads
        model, g, n = self.model, self.num_starts, self.model.num_data
        val = {key: self._constrained(key) for key in self._var}
        if self._student:
            df, scale = 2.0 * val["a"], val["b"] / val["a"]
        else:
            df, scale = np.zeros(g), np.ones(g)
        x = model.x_data
        _, quad, logdet, info, terms = sweeps.loss_and_grad_batch(
            x.ctx, x, model.y_data, network=self._network, num_hiddens=self._layers, activation=self._activation,
            w_std=val["w_std"], b_std=val["b_std"], last_w_std=val["last_w_std"], eps=val["eps"], df=df, scale=scale)
        losses = np.full(g, np.nan)
        grads = {name: np.full(g, np.nan) for name in self.raw}
        for s in range(g):
            if info[s] != 0:
                continue
            lp, dlp = lml_value_and_grads(terms[s], float(quad[s]), float(logdet[s]), n, float(df[s]), float(scale[s]),
                                          float(val["a"][s]) if self._student else None,
                                          float(val["b"][s]) if self._student else None)
            losses[s] = -lp / n
            for key, d in dlp.items():
                name = self._name[key]
                grads[name][s] = float(-d / n * self._var[key].constraint.grad(self.raw[name][s]))
        return losses, grads

    def step(self, learning_rate):
        """One step of every start; returns the G losses before the update."""
        self.losses, grads = self.value_and_grad()
        self.optimizer(learning_rate, grads)
        return self.losses

    __call__ = step

    def best(self):
        if not np.isfinite(self.losses).any():
            raise ValueError("no start has a finite loss (take a step first)")
        return int(np.nanargmin(np.where(np.isfinite(self.losses), self.losses, np.nan)))

    def assign_best(self):
        s = self.best()
        for name, var in self.variables.items():
            var.assign(float(self.raw[name][s]))
        return s


def build_multistart_step(model, starts, optimizer=None):
    """step(learning_rate) -> losses[G] before the update, for G starts of `model` trained side by side (MultiStartStep).
    starts: {name in model.vars(): array of G raw values}.  MLP and dense-ResNet kernels with a Gaussian or Student-t
    likelihood; conv kernels and NTKKernel models raise NotImplementedError (use build_train_step per start)."""
    return MultiStartStep(model, starts, optimizer)


class PlateauSchedule:
    """Learning-rate decay on a validation plateau, with the interface the regression run uses
    (experiments/regression/train.py:159,198,208-211; experiments/utils.py:153-231): `.lr` is the current rate,
    `.step(metric)` records one validation result and returns True when it just cut the rate by `factor`.
    A result counts as an improvement when it beats the best one by more than `threshold` (relative by default);
    after more than `patience` results without improvement the rate is multiplied by `factor`, not below `min_lr`."""

    def __init__(self, lr, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", min_lr=0.0,
                 eps=1e-8):
        if mode not in ("min", "max"):
            raise ValueError("mode " + str(mode) + " is unknown!")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError("threshold mode " + str(threshold_mode) + " is unknown!")
        self.lr, self.factor, self.patience, self.min_lr, self.eps = float(lr), factor, patience, min_lr, eps
        sign = 1.0 if mode == "min" else -1.0               # work on sign * metric: smaller is always better
        if threshold_mode == "rel":
            # min: a < best (1 - t);  max: a > best (1 + t)  <=>  -a < -best (1 + t)
            self._margin = lambda best: best * (1.0 - sign * threshold)
        else:
            self._margin = lambda best: best - threshold
        self._sign = sign
        self._best = float("inf")
        self.stale = 0
        self.calls = 0

    @property
    def best(self):
        return self._sign * self._best

    def step(self, metric):
        value = self._sign * float(metric)
        self.calls += 1
        if value < self._margin(self._best):
            self._best, self.stale = value, 0
            return False
        self.stale += 1
        if self.stale <= self.patience:
            return False
        self.stale = 0
        lowered = max(self.lr * self.factor, self.min_lr)
        if self.lr - lowered > self.eps:
            self.lr = lowered
        return True

