"""Knowledge-distillation training step on gfx950 kernels, mirroring `big_vision/trainers/proj/distill/distill.py`
("Knowledge distillation: A good teacher is patient and consistent").

Reference: `getfirst` (:57-61), the model registry (:160-173), parameter init with `init_head_bias` (:178-197), the
optimizer on the student only (:205-215), `loss_fn` (:217-248: every model on `getfirst(data, name, "image")`, the
entropy / task-loss measurements, `dd.dist(student, teacher, config.distance, **config.distance_kw)` summed over
`config.teachers`), `update_fn` (:250-285: ONE mixup coefficient for image, labels and every per-model input), the
teacher loads (:287-294), student init (:320-327) and the predict functions (:338-359).

Kept: names, the config fields consumed (`student_name, student, <teacher>_name, <teacher>, <teacher>_init,
<teacher>_load, teachers, student_init, student_load, num_classes, init_head_bias, distance, distance_kw, mixup`, the
optimizer fields of train.py), the measurement names, `update_fn(train_state, rng, batch)`.
New: explicit kernel sequences instead of jit + autograd.  The teachers run forward-only (no saved activations, no
dropout, no gradient buffers); the student's dlogits is accumulated over the teachers by one `bv_distill_dist` launch
each (include/bvdistill.h), then the student's backward, gradient sync and optimizer step are those of
`big_vision_amd.train`.  train_state = {"params": {"student": ..., <teacher>: ...}, "opt": student optimizer};
checkpoints (`save_checkpoint`) hold the student and the optimizer only, as in the reference (:308-313).

Out of scope: the BiT / ResNet models of the reference's own distill configs, `flexi/distill.py`, the tf.data input
pipeline, and multi-process GPU runs of this trainer (the data-parallel path is the one of train.py and is exercised
on the host only).
"""
from __future__ import annotations

import importlib

import torch

from big_vision_amd import _lib
from big_vision_amd import dp
from big_vision_amd import engine as E
from big_vision_amd import ops
from big_vision_amd import optax as bv_optax
from big_vision_amd import train as bv_train
from big_vision_amd import utils as u

F32 = torch.float32


def getfirst(d, *keys):
  """Returns the first of `keys` that is in `d`."""
  for k in keys:
    if k in d:
      return d[k]
  raise KeyError(f"None of {keys} is in {list(d)}")


def get_model_mod(config, name):
  return importlib.import_module(f"big_vision_amd.models.{config[f'{name}_name']}")


def get_models(config):
  """{"student": model, <teacher>: model, ...} by module path, every one with `config.num_classes` outputs."""
  make = lambda name: get_model_mod(config, name).Model(num_classes=config.num_classes, **config.get(name, {}))
  return {"student": make("student"), **{t: make(t) for t in config.teachers}}


def _image_shape(image_shapes, name):
  """image_shapes: one shape for all models, or a dict keyed like the batch (`getfirst(shapes, name, "image")`)."""
  return tuple(getfirst(image_shapes, name, "image")) if isinstance(image_shapes, dict) else tuple(image_shapes)


def make_train_state(models, config, image_shapes, *, rng=0, comm=None, total_steps=None, device=None):
  """Student store + optimizer (as train.make_train_state) and one frozen, loaded store per teacher."""
  seed = E.seed_of(rng)
  for name in config.teachers:       # a teacher NEEDS an init: fail before anything is allocated
    config[f"{name}_init"]   # pylint: disable=pointless-statement
  # -- student
  model = models["student"]
  shape = _image_shape(image_shapes, "student")
  store = model.make_store(shape, device, bv_optax.frozen_leaves(config, model.leaf_names(shape)))
  store.init_random(seed)
  if "init_head_bias" in config:
    store.leaf("head/bias").fill_(float(config["init_head_bias"]))
    store.mark_dirty()
  if config.get("student_init"):
    bv_train.load_init(model, store, config.student_init, config.get("student"), config.get("student_load", {}),
                       key="student_init")
  store.refresh_shadow()
  store.want_grads = True
  params = {}
  # -- teachers: never optimised, never checkpointed
  for i, name in enumerate(config.teachers):
    m = models[name]
    ts = m.make_store(_image_shape(image_shapes, name), device)
    ts.init_random(seed + 1 + i)
    bv_train.load_init(m, ts, config[f"{name}_init"], config.get(name), config.get(f"{name}_load", {}),
                       key=f"{name}_init")
    ts.refresh_shadow()
    params[name] = ts.tree()
  opt, sched_fns = bv_train.make_optimizer(config, store, shape[0], comm, total_steps)
  return {"params": {"student": store.tree(), **params}, "opt": opt}, sched_fns     # (the tree only now: make_optimizer)


def _distance(config):
  kind = config.get("distance", "kl")
  assert kind in _lib.DISTILL_KINDS, f"Unknown kind of distance {kind}."
  assert kind != "agree", "the 'agree' distance has no derivative: it is an evaluator metric, not a training loss"
  kw = dict(config.get("distance_kw", {}))
  unknown = set(kw) - {"epsilon", "t", "ls", "k", "feat_axis"}
  if unknown:
    raise TypeError(f"dist() got unexpected keyword arguments {sorted(unknown)}")
  if kw.pop("feat_axis", -1) not in (-1, 1):
    raise NotImplementedError("distance_kw.feat_axis: the trainer's logits are [n, C], the feature axis is the last")
  if "epsilon" in kw:
    kw["eps"] = kw.pop("epsilon")
  return kind, kw


def _fwd(model, params, image, **kw):
  store = params.store
  store.refresh_shadow()   # no-op when clean
  image = image.to(F32).contiguous()
  return model.executor(store, "", model.grid(tuple(image.shape))).fwd(image, **kw)


def make_update_fn(models, config, comm=None):
  """Builds `update_fn(train_state, rng, batch)` (distill.py:250-285)."""
  comm = comm or dp.Comm()
  kind, dist_kw = _distance(config)
  teachers = tuple(config.teachers)
  mix_p = bv_train.mixup_p(config)

  def update_fn(train_state, rng, batch):
    params, opt = train_state["params"], train_state["opt"]
    student = models["student"]
    store = params["student"].store
    store.want_grads = True
    store.refresh_shadow()
    store.zero_grad()
    # distill.py:257-261: ONE coefficient for the images, the labels and every per-model input
    data = bv_train.prepare_batch(batch, rng, opt, mix_p, keys=("image", "labels") + tuple(models))
    n = getfirst(data, "student", "image").shape[0]
    n_global = n * comm.size
    dev = store.device
    meas = {}
    acc = lambda: torch.zeros(1, device=dev, dtype=torch.float64)

    def measure(name, logits):
      meas[f"entropy_{name}"] = acc()
      ops.distill_entropy(logits, sum=meas[f"entropy_{name}"], n_global=n_global)
      if "labels" in data:
        meas[f"task_loss_{name}"] = acc()
        ops.softmax_xent(logits, data["labels"], meas[f"task_loss_{name}"], want_grad=False, n_global=n_global)

    # teachers: eval mode, nothing kept for a backward
    t_logits = {}
    for name in teachers:
      t_logits[name] = _fwd(models[name], params[name], getfirst(data, name, "image"), save=False)[0].contiguous()
    # student: train mode, its own dropout key per step and rank (distill.py:264-267)
    drop = bv_train.step_dropout(student, rng, opt, comm)
    logits, _, ctx = _fwd(student, params["student"], getfirst(data, "student", "image"), save=True, drop=drop)
    logits = logits.contiguous()
    measure("student", logits)
    for name in teachers:
      measure(name, t_logits[name])
    # loss = sum over the teachers of mean_i dist(student_i, teacher_i); dlogits accumulates over them
    dlogits = None
    for name in teachers:
      meas[f"distill_loss_{name}"] = acc()
      _, g = ops.distill_dist(kind, logits, t_logits[name], loss_sum=meas[f"distill_loss_{name}"], dstudent=dlogits,
                              want_grad=True, n_global=n_global, **dist_kw)
      dlogits = g
    sync = bv_train.grad_sync(opt, comm, store) if comm.size > 1 else None
    student.executor(store, "", student.grid(tuple(getfirst(data, "student", "image").shape))).bwd(ctx, dlogits)
    if sync is not None:
      sync.finish()
    names = sorted(meas)
    packed = torch.cat([meas[k] for k in names])
    comm.all_reduce_scalars_(packed)
    measurements = {k: packed[i] for i, k in enumerate(names)}
    measurements["distill_loss"] = sum(measurements[f"distill_loss_{name}"] for name in teachers)
    measurements["training_loss"] = measurements["distill_loss"]
    measurements.update(opt.step())
    return {"params": params, "opt": opt}, measurements

  return bv_train.in_residual_stream(config, update_fn)


def make_predict_fns(models, config):
  """distill.py:338-359: `<name>_fwd` per model, `teacher_ensemble_fwd` (mean of the teachers' softmax, {}), and
  `student_<teacher>_fwd` / `student_teacher_ensemble_fwd` pairs for the distance evaluator.  A model reads
  `getfirst(batch, <name>, "image")` like in the training step, so a teacher of another resolution can be evaluated
  from its own batch key (the reference's predict functions read `batch["image"]` only)."""
  teachers = tuple(config.teachers)

  def single(name):
    return lambda train_state, batch: models[name].apply({"params": train_state["params"][name]},
                                                         getfirst(batch, name, "image"))

  def ensemble(train_state, batch):
    probs = None
    for t in teachers:
      logits = models[t].apply({"params": train_state["params"][t]}, getfirst(batch, t, "image"), collect=False)[0]
      probs = ops.distill_softmax_acc(logits.contiguous(), 1.0 / len(teachers), probs)
    return probs, {}

  def pair(other):
    return lambda train_state, batch: (fns["student_fwd"](train_state, batch), fns[f"{other}_fwd"](train_state, batch))

  fns = {f"{name}_fwd": single(name) for name in models}
  fns["teacher_ensemble_fwd"] = ensemble
  fns.update({f"student_{other}_fwd": pair(other) for other in teachers + ("teacher_ensemble",)})
  return fns


def save_checkpoint(fname, train_state):
  """The student and the optimizer only: the teachers never change and are loaded from their own files."""
  u.save_train_state(fname, {"params": train_state["params"]["student"], "opt": train_state["opt"]})


def load_checkpoint(fname, train_state):
  u.load_train_state(fname, {"params": train_state["params"]["student"], "opt": train_state["opt"]})
  return train_state
