"""GSAM / SAM classification training step on gfx950 kernels, mirroring `big_vision/trainers/proj/gsam/train.py`
(config: configs/proj/gsam/vit_i1k_gsam_no_aug.py).

Reference: the trainer is `big_vision/train.py` with another step.  `assert not config.get("grad_accum_steps")` (:68),
the model registry (:147-149), `init_head_bias` (:161-164), `assert len(sched_fns) == 1` (:182), and `update_fn`
(:188-222): mixup once (:194-195), ONE dropout key per step and device used by both passes (:198-206),
`learning_rate = sched_fns[0](step) * config.lr` (:208), `gsam_gradient(..., **config.gsam)` on the LOCAL batch
(:209-210), `pmean((l, grads))` (:211), `tx.update` on the averaged GSAM gradient (:212-213) and the measurements
`l2_grads, l2_params, l2_updates` (:215-220).

Kept: names, `update_fn(train_state, rng, batch) -> (train_state, measurements)`, `training_loss` = the clean loss,
the config fields (`config.gsam`: rho_max, rho_min, alpha, lr_max, lr_min, eps, minimize_fp; otherwise those of
`big_vision_amd.train`, plus init_head_bias), the refusals.
New: no jit / pmap / autograd.  Model, train state, loss kernel, mixup, dropout, predict function and the finite
check are `big_vision_amd.train`'s; the step is two of its forward / backward passes and the vector stage of `gsam.py`.
Both passes normalise the loss by the LOCAL batch and run no gradient collective (the reference perturbs per worker,
before the pmean); the GSAM gradient is written times 1 / comm.size and summed over the ranks once, which is the
reference's pmean, so global-norm clipping sees the averaged gradient.

`make_grad_fn` is the step up to and including that all-reduce, `make_update_fn` adds `opt.step()`: a test (or a
caller that wants the gradient only) stops between the two.  `grad_fn.buffers()` is the trainer-owned `gsam.Buffers`
(g_clean among them) once a step has run.

Out of scope: `adaptive_perturbation`, `sharding_strategy` with fsdp (the reference's GSAM trainer is pmap-replicated;
here the perturbation needs the whole fp32 master on every rank), the input pipeline and the training loop.
"""
from __future__ import annotations

import torch

from big_vision_amd import dp
from big_vision_amd import optax as bv_optax
from big_vision_amd import train as bv_train
from big_vision_amd.train import check_finite, get_model, load_init, make_predict_fn  # noqa: F401  (the trainer's surface)
from big_vision_amd.trainers.proj.gsam import gsam

F32 = torch.float32


def check_config(config):
  """The refusals of the reference trainer and of this port; returns `config.gsam` as gsam_gradient's arguments."""
  assert not config.get("grad_accum_steps"), "Grad-acc not supported anymore."
  schedule = config.get("schedule", {})
  n_sched = sum(s is not None for _, s in schedule) if isinstance(schedule, (tuple, list)) else 1
  assert n_sched == 1, "Current GSAM supports one global learning-rate."      # len(sched_fns) == 1 (:182)
  return gsam.hparams(**config.gsam)


def make_train_state(model, config, image_shape, *, rng=0, comm=None, total_steps=None, device=None):
  """`train.make_train_state` with `config.init_head_bias` (:161-164: set at init, before a `model_init` load)."""
  check_config(config)

  def head_bias(store):
    if "init_head_bias" in config:
      store.leaf("head/bias").fill_(float(config["init_head_bias"]))

  state, sched_fns = bv_train.make_train_state(model, config, image_shape, rng=rng, comm=comm, total_steps=total_steps,
                                               device=device, after_init=head_bias)
  assert len(sched_fns) == 1, "Current GSAM supports one global learning-rate."
  if getattr(state["opt"], "sharded", False):
    raise NotImplementedError("config.sharding_strategy: the GSAM trainer is replicated (the reference's is a pmap); "
                              "its perturbation needs the whole fp32 master on every rank, fsdp is not supported")
  return state, sched_fns


def make_grad_fn(model, config, comm=None):
  """`grad_fn(train_state, rng, batch, stages=None)`: the gradient phase of the step.  Leaves the GSAM gradient,
  averaged over the ranks, in `store.grad` and returns the clean loss (f64 device scalar, averaged too).  `stages`:
  see gsam.gsam_gradient."""
  comm = comm or dp.Comm()
  loss_kernel = bv_train._loss_kernel(config)
  mix_p = bv_train.mixup_p(config)
  gsam_kw = check_config(config)
  base_lr = float(config["lr"])
  bufs = []

  def grad_fn(train_state, rng, batch, stages=None):
    params, opt = train_state["params"], train_state["opt"]
    assert len(opt.schedule_fns) == 1, "Current GSAM supports one global learning-rate."
    store = params.store
    if not bufs or bufs[0].store is not store:
      bufs[:] = [gsam.Buffers(store)]
    store.want_grads = True
    store.refresh_shadow()
    images, labels = bv_train.images_labels(batch, rng, opt, mix_p)     # mixup once, before both passes
    n = images.shape[0]
    ex = model.executor(store, "", model.grid(tuple(images.shape)))
    drop = bv_train.step_dropout(model, rng, opt, comm)                 # the same key in both passes

    def fwd_bwd():
      store.zero_grad()
      logits, _, ctx = ex.fwd(images, save=True, drop=drop)
      acc = torch.zeros(1, device=images.device, dtype=torch.float64)
      dlogits = loss_kernel(logits.contiguous(), labels, acc, want_grad=True, n_global=n)   # the LOCAL mean
      ex.bwd(ctx, dlogits)
      return acc

    lr = opt.schedule_fns[0](bv_optax.get_count(opt)) * base_lr
    acc = gsam.gsam_gradient(fwd_bwd, store, bufs[0], lr=float(lr), scale=1.0 / comm.size, stages=stages, **gsam_kw)
    if comm.size > 1:       # pmean((l, grads)): the gradient carries 1 / size already
      acc /= comm.size
      comm.all_reduce_sum_(store.grad)
      comm.all_reduce_scalars_(acc)
    return acc[0]

  grad_fn = bv_train.in_residual_stream(config, grad_fn)
  grad_fn.buffers = lambda: bufs[0] if bufs else None
  return grad_fn


def make_update_fn(model, config, comm=None):
  """Builds `update_fn(train_state, rng, batch)` (:188-222); `update_fn.grad_fn` is its gradient phase."""
  grad_fn = make_grad_fn(model, config, comm)

  def update_fn(train_state, rng, batch):
    measurements = {"training_loss": grad_fn(train_state, rng, batch)}
    measurements.update(train_state["opt"].step())
    return {"params": train_state["params"], "opt": train_state["opt"]}, measurements

  update_fn.grad_fn = grad_fn
  return update_fn
