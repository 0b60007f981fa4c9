"""Classification training step on gfx950 kernels + RCCL, mirroring `big_vision/train.py`.

Reference: big_vision/train.py — `update_fn` (:275-315): optional mixup
(`u.get_mixup`, utils.py:1146-1154), `loss_fn` = `getattr(u, config.get("loss",
"sigmoid_xent"))(logits, labels)` on the logits of `model.apply` (:295-300),
`jax.value_and_grad`, `tx.update` + `optax.apply_updates`, and the measurements
`training_loss, l2_grads, l2_params, l2_updates` (:307-313).  This is BASELINE
configs[0] (ViT-S/16 on ImageNet-1k, `configs/vit_s16_i1k.py`).

Kept: names and signatures (`update_fn(train_state, rng, batch) -> (train_state,
measurements)`), the config fields consumed (`model_name, model, num_classes, loss,
mixup, optax_name, optax, lr, wd, schedule, grad_clip_norm`), error behaviour.
New: forward, backward, loss and optimizer are explicit libbvhip kernel sequences
(big_vision_amd.models.vit.VitExec); no jit, no autograd.

Data parallelism (sharding.py:83-101, replicated parameters, batch split on dim 0):
every rank normalises its loss / dlogits by the GLOBAL batch size, so parameter
gradients are partial sums and one all-reduce(SUM) finishes them (dp.GradSync).
Mixup rolls the batch along dim 0 on every device independently, exactly like the
reference's shard_map (:283-289).

The host code around the kernels that every trainer shares lives here too (the SigLIP / contrastive, distillation and
GSAM trainers call it): `make_optimizer` (the tail of a `make_train_state`), `prepare_batch`, `step_dropout`,
`in_residual_stream`, `grad_sync`, `load_init`, `check_finite`.
"""
from __future__ import annotations

import importlib
import os

import torch

from big_vision_amd import dp
from big_vision_amd import engine as E
from big_vision_amd import ops
from big_vision_amd import optax as bv_optax
from big_vision_amd import sharding
from big_vision_amd import utils as u
from big_vision_amd.models import common

F32 = torch.float32
LOSSES = {"softmax_xent": ops.softmax_xent, "sigmoid_xent": ops.sigmoid_xent}


def get_model(config):
  """Model registry by module path (train.py:191-192)."""
  model_mod = importlib.import_module(f"big_vision_amd.models.{config.model_name}")
  return model_mod, model_mod.Model(num_classes=config.num_classes, **config.get("model", {}))


def _loss_kernel(config):
  name = config.get("loss", "sigmoid_xent")
  if name not in LOSSES:
    raise AttributeError(f"module 'big_vision.utils' has no loss '{name}' on the accelerated path "
                         f"(available: {sorted(LOSSES)})")
  return LOSSES[name]


def make_train_state(model, config, image_shape, *, rng=0, comm=None, total_steps=None, device=None, after_init=None):
  """Parameter store + optimizer laid out for `config` (replaces train.py:191-262).  after_init(store): edits of the
  random init that a checkpoint load may still overwrite (a trainer's `init_head_bias`)."""
  store = model.make_store(image_shape, device, bv_optax.frozen_leaves(config, model.leaf_names(image_shape)))
  store.init_random(E.seed_of(rng))
  if after_init is not None:
    after_init(store)
    store.mark_dirty()
  if config.get("model_init"):
    _load_model_init(model, config, store)
  store.refresh_shadow()
  store.want_grads = True
  opt, sched_fns = make_optimizer(config, store, image_shape[0], comm, total_steps)
  return {"params": store.tree(), "opt": opt}, sched_fns


def make_optimizer(config, store, n_local, comm=None, total_steps=None):
  """(opt, sched_fns) of `config` on `store`, the tail of every trainer's make_train_state (train.py:201-218): the
  parameter placement - replicated, or "fsdp" somewhere in config.sharding_strategy = sharded optimizer state / update;
  any other strategy is refused, not ignored - the global batch size (`n_local` per rank unless config.input says
  otherwise), the number of steps and `bv_optax.make`.  Take `store.tree()` only AFTER this call: the fsdp placement
  shards the fp32 master here, and a tree built before it would keep the whole unsharded master alive through stale
  views."""
  comm = comm or dp.Comm()
  fsdp = sharding.is_sharded(sharding.check_config(config, store.tree(), mesh=comm))
  batch_size = config.get("input", {}).get("batch_size", n_local * comm.size)
  total_steps = total_steps if total_steps is not None else u.steps("total", config, None, batch_size)
  return bv_optax.make(config, store, sched_kw=dict(total_steps=total_steps, batch_size=batch_size, data_size=None),
                       comm=comm, shard=fsdp)


def _load_model_init(model, config, store):
  """train.py:353-359: `model_mod.load(params, config.model_init, config.model, **config.model_load)` into the store.
  Runs before bv_optax.make: the fsdp placement shards the fp32 master there, and a load after it would leave the
  shadow and master views of the earlier layout behind."""
  load_init(model, store, config.model_init, config.get("model"), config.get("model_load", {}), key="model_init")


def load_init(model, store, init, model_cfg, load_kw, key):
  """`model_mod.load(params, init, model_cfg, **load_kw)` into `store`; `key` names the config field in the errors."""
  model_mod = importlib.import_module(type(model).__module__)
  if not hasattr(model_mod, "load"):
    raise NotImplementedError(f"config.{key}: {model_mod.__name__} has no load()")
  path = getattr(model_mod, "VANITY_NAMES", {}).get(init, init) if isinstance(init, str) else init
  common.refuse_remote(path, f"config.{key}={init!r}")
  if isinstance(path, str) and not any(os.path.isfile(p) for p in (path, path.rsplit(":", 1)[0])):
    raise FileNotFoundError(f"config.{key}={init!r}: no such checkpoint file (remote vanity names are not "
                            "fetched; pass the local .npz path)")
  params = model_mod.load(store.tree(), init, model_cfg, **load_kw)
  store.load_tree(params)


def loss_fn(model, params, images, labels, config, comm=None):
  """Forward-only loss, the `loss_fn(params)` closure of train.py:295-300 (no mixup)."""
  comm = comm or dp.Comm()
  store = params.store
  store.refresh_shadow()
  ex = model.executor(store, "", model.grid(tuple(images.shape)))
  logits, _, _ = ex.fwd(images, save=False)
  acc = torch.zeros(1, device=images.device, dtype=torch.float64)
  _loss_kernel(config)(logits.contiguous(), labels.to(F32).contiguous(), acc, want_grad=False,
                       n_global=images.shape[0] * comm.size)
  comm.all_reduce_scalars_(acc)
  return acc[0]


def mixup_p(config):
  """`config.mixup.p` (train.py:281), 0.0 without a mixup section."""
  return float(config.get("mixup", {}).get("p", 0.0) or 0.0) if config.get("mixup") else 0.0


def prepare_batch(batch, rng, opt, mix_p, keys=("image", "labels")):
  """`batch` with every one of `keys` that is present fp32 contiguous, and mixed up when `mix_p` (train.py:283-289):
  ONE coefficient per step for all of them (fold_in(rng, step), or the batch's own `mixup_a`), the roll is per
  device.  Returns a dict; its other entries are the batch's."""
  data = dict(batch)
  keys = [k for k in keys if k in data]
  for k in keys:
    data[k] = data[k].to(F32).contiguous()
  if mix_p:
    a = data.get("mixup_a")
    if a is None:
      a = u.get_mixup_coefficient(rng, bv_optax.get_count(opt), mix_p)
    for k in keys:
      data[k] = ops.mixup(data[k], a)
  return data


def images_labels(batch, rng, opt, mix_p):
  """`prepare_batch` of the classification trainers: the (images, labels) pair, both required."""
  data = prepare_batch(batch, rng, opt, mix_p)
  return data["image"], data["labels"]


def step_dropout(model, rng, opt, comm):
  """Dropout (vit.py:228,100,109,76; train.py:298 rngs={"dropout": rng_model}): one key per step and rank; None for a
  model without dropout."""
  if float(getattr(model, "dropout", 0.0) or 0.0) <= 0.0:
    return None
  if rng is None:
    raise ValueError("the model has dropout > 0: update_fn needs an rng")
  return E.Dropout(model.dropout, E.seed_of(rng)).fold("step", int(bv_optax.get_count(opt)), "rank", int(comm.rank))


def in_residual_stream(config, fn):
  """`fn` run on config.residual_stream ("float32" = the reference's arithmetic, "bfloat16"): set for the duration of
  each call and restored afterwards, so model.apply / other trainers in the process keep their own.  Without a config
  `fn` runs on whatever stream its caller has set: it is returned as it is."""
  if config is None:
    return fn
  stream = config.get("residual_stream", "float32")

  def wrapped(*args, **kw):
    old = E.set_residual_stream(stream)
    try:
      return fn(*args, **kw)
    finally:
      E.set_residual_stream(old)
  return wrapped


def grad_sync(opt, comm, store):
  """The overlapped gradient sum of one step: the sharded optimizer's own ("fsdp" placement: every range is summed
  onto its owner only, dp.GradShardSync), else the all-reduce of the whole gradient buffer (dp.GradSync)."""
  return opt.grad_sync() if getattr(opt, "sharded", False) else dp.GradSync(comm, store.grad)


def make_update_fn(model, config, comm=None):
  """Builds `update_fn(train_state, rng, batch)` (train.py:275-315)."""
  comm = comm or dp.Comm()
  loss_kernel = _loss_kernel(config)
  mix_p = mixup_p(config)

  def update_fn(train_state, rng, batch):
    params, opt = train_state["params"], train_state["opt"]
    store = params.store
    store.want_grads = True
    store.refresh_shadow()   # no-op when clean; picks up load_tree() / in-place master edits
    store.zero_grad()
    images, labels = images_labels(batch, rng, opt, mix_p)
    n = images.shape[0]
    ex = model.executor(store, "", model.grid(tuple(images.shape)))
    drop = step_dropout(model, rng, opt, comm)
    logits, _, ctx = ex.fwd(images, save=True, drop=drop)
    acc = torch.zeros(1, device=images.device, dtype=torch.float64)
    dlogits = loss_kernel(logits.contiguous(), labels, acc, want_grad=True, n_global=n * comm.size)
    sync = grad_sync(opt, comm, store) if comm.size > 1 else None
    ex.bwd(ctx, dlogits)
    if sync is not None:
      sync.finish()
    comm.all_reduce_scalars_(acc)
    measurements = {"training_loss": acc[0]}
    measurements.update(opt.step())
    return {"params": params, "opt": opt}, measurements

  return in_residual_stream(config, update_fn)


def make_predict_fn(model, config=None):
  """`predict_fn(train_state, batch) -> (logits, out)` (`eval_logits_fn`, train.py:380-382): the forward at train=False on the same
  kernels as the training step, for `evaluators.common.from_config(config, {"predict": predict_fn})`.  With `config`
  the forward runs on `config.residual_stream`, like `update_fn`; it reads the parameters and changes nothing."""
  def predict_fn(train_state, batch):
    return model.apply({"params": train_state["params"]}, batch["image"].to(F32).contiguous())
  return in_residual_stream(config, predict_fn)


def check_finite(measurements):
  """NaN/Inf abort of train.py:452-454 (synchronises)."""
  for k, v in measurements.items():
    if not torch.isfinite(torch.as_tensor(v)).all():
      raise RuntimeError(f"measurement '{k}' is not finite: {v}")
