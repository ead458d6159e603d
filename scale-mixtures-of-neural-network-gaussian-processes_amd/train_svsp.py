"""Training loop of the sparse variational classifier (SVSP) -- the counterpart of experiments/classification/train.py:61-75
(`objax.GradValues(model.loss, train_vars)` + `objax.optimizer.Adam`) and :77-110 (train / valid epochs) without autodiff.

The gradient is SVSP.loss_and_grad: one fp64 kernel build over [inducing images; batch], one smn_svsp_elbo_grad, one
tangent pass for the kernel's hyper-parameters and, when the inducing images are among the variables, one reverse pass
of the conv kernel for them (smn_kernel_cnn_input_grad).  The reference trains them (train.py:205 puts model.vars() into
the optimiser) from a subset of the training set (train.py:177-182); here they are selected with
svsp_train_vars(model, inducing=True) and stay where they were initialised otherwise.  As there, svtp leaves
`last_w_std` out (train.py:204-216).
"""
from __future__ import annotations

import math

import numpy as np

from .spax.base import TrainVar
from .train import PlateauSchedule                      # noqa: F401  (re-exported: the schedule the epochs below take)

__all__ = ["ArrayAdam", "svsp_train_vars", "build_svsp_train_step", "train_epoch", "valid_epoch", "PlateauSchedule"]


class ArrayAdam:
    """objax.optimizer.Adam (beta1=0.9, beta2=0.999, eps=1e-8) over a dict of scalars and arrays:
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  x -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)
    step(values, grads, lr) -> new values.  An entry whose gradient holds a non-finite number is left alone, with its
    moments (as train.Adam does); the step count is shared."""

    def __init__(self, beta1=0.9, beta2=0.999, eps=1e-8):
        self.b1, self.b2, self.eps = beta1, beta2, eps
        self.m, self.v, self.t = {}, {}, 0

    def step(self, values, grads, lr):
        self.t += 1
        lr_t = lr * math.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        out = {}
        for k, x in values.items():
            x = np.asarray(x, dtype=np.float64)
            g = grads.get(k)
            if g is None or not np.all(np.isfinite(g)):
                out[k] = x
                continue
            g = np.asarray(g, dtype=np.float64)
            self.m[k] = self.b1 * self.m.get(k, 0.0) + (1 - self.b1) * g
            self.v[k] = self.b2 * self.v.get(k, 0.0) + (1 - self.b2) * g * g
            out[k] = x - lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps)
        return out


def svsp_train_vars(model, inducing=False):
    """The variables experiments/classification/train.py:204-216 trains: everything for svgp (GaussianPrior); everything
    but last_w_std for svtp (InverseGammaPrior).  The inducing images are among them with inducing=True only."""
    from .spax.priors import InverseGammaPrior
    skip = ("last_w_std",) if isinstance(model.prior, InverseGammaPrior) else ()
    if not inducing:
        skip += ("inducing_variable",)
    return {k: v for k, v in model.vars().items() if isinstance(v, TrainVar) and not any(s in k for s in skip)}


def build_svsp_train_step(model, variables=None, optimizer=None, *, num_train, num_samples):
    """train_step(key, x_batch, y_batch, lr) -> n_elbo before the update (classification/train.py:61-75).
    variables: name -> TrainVar to update (default: svsp_train_vars(model)); with `inducing_variable` among them every step
    also asks for the inducing-image gradient (loss_and_grad(inducing_grad=True))."""
    variables = variables if variables is not None else svsp_train_vars(model)
    need_inducing = any("inducing_variable" in k for k in variables)
    optimizer = optimizer or ArrayAdam()
    need_kernel = any(k.split(".")[-1] in ("w_std", "b_std", "last_w_std") for k in variables)

    def train_step(key, x_batch, y_batch, lr):
        value, grads = model.loss_and_grad(key, x_batch, y_batch, num_train, num_samples, kernel_grads=need_kernel,
                                           inducing_grad=need_inducing)
        new = optimizer.step({k: v.value for k, v in variables.items()}, {k: g for k, g in grads.items() if k in variables}, lr)
        for k, v in variables.items():
            v.assign(new[k])
        return value

    train_step.optimizer = optimizer
    train_step.variables = variables
    return train_step


def train_epoch(train_step, x, y, batch_size, lr, seed, epoch=0, shuffle=True):
    """One pass over the in-memory training set in batches of `batch_size` (classification/train.py:77-93; the last,
    smaller batch is dropped as the reference's loader does) -> mean n_elbo over the steps.  The variates of step i of epoch e
    are keyed (seed + e, i * batch_size): no two steps of a run share a variate."""
    n = len(y)
    order = np.random.default_rng((int(seed), int(epoch))).permutation(n) if shuffle else np.arange(n)
    total, steps = 0.0, 0
    for i0 in range(0, n - batch_size + 1, batch_size):
        idx = order[i0:i0 + batch_size]
        total += train_step((int(seed) + int(epoch), i0), x[idx], y[idx], lr)
        steps += 1
    if steps == 0:
        raise ValueError("batch_size %d is larger than the training set (%d)" % (batch_size, n))
    return total / steps


def valid_epoch(model, x, y, num_samples, seed=10, batch=None, schedule=None, checkpointer=None, index=0):
    """classification/train.py:95-110: (nll, accuracy in percent) of SVSP.evaluate on the validation set; steps `schedule`
    (a PlateauSchedule, on the nll) and `checkpointer` (a checkpoint.Checkpointer: saves model.vars() on a new best nll)."""
    nll, acc = model.evaluate(x, y, num_samples, seed=seed, batch=batch)
    if schedule is not None:
        schedule.step(nll)
    if checkpointer is not None:
        checkpointer.step(index, nll, model.vars())
    return nll, acc
