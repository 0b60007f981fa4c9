"""Distillation trainer parity (big_vision/trainers/proj/distill/distill.py:217-285): the HIP `update_fn` of
big_vision_amd.trainers.proj.distill.distill vs the fp64 oracle (`bv_oracle.vit_forward` for the student and both
teachers + the restated distance of tests/_distill_bounds.py, autograd to the student's leaves) on identical weights
and a synthetic batch.  Student: ViT width 128, depth 2 at 64 px; teacher `prof_a`: the same shape, other weights;
teacher `prof_b`: depth 1 at 96 px, fed from its own batch key.  Teachers are loaded from .npz files written with the
existing checkpoint helpers.  Bounds as in test_train_step_gpu.py: loss rel <= 1e-2, logits max-abs <= 5e-2,
tests/_parity.py per-tensor gradient bounds with the measured bf16 floor reported."""
import math

import pytest
import torch

import _distill_bounds as D

pytestmark = pytest.mark.gpu

VIT = dict(width=128, depth=2, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="gap")
N = 6
RES = {"student": 64, "prof_a": 64, "prof_b": 96}
TEACHERS = ("prof_a", "prof_b")


def _setup(dev, tmp_path, num_classes, distance, distance_kw, mixup_a=None, **extra):
  from big_vision_amd import utils as u
  from big_vision_amd.compat.ml_collections import ConfigDict
  from big_vision_amd.trainers.proj.distill import distill
  c = ConfigDict()
  c.lr, c.wd = 1e-3, 1e-4
  c.schedule = dict(warmup_steps=2, decay_type="cosine")
  c.optax_name, c.optax = "scale_by_adam", dict(mu_dtype="bfloat16")
  c.grad_clip_norm, c.total_steps, c.num_classes = 1.0, 10, num_classes
  c.student_name, c.student = "vit", dict(VIT)
  c.teachers = list(TEACHERS)
  c.prof_a_name, c.prof_a = "vit", dict(VIT)
  c.prof_b_name, c.prof_b = "vit", dict(VIT, depth=1)
  c.distance, c.distance_kw = distance, dict(distance_kw)
  if mixup_a is not None:
    c.mixup = dict(p=0.2, fold_in=None)
  for k, v in extra.items():
    c[k] = v
  models = distill.get_models(c)
  g = torch.Generator().manual_seed(3)

  def perturb(store):   # break zero / unit inits (the head kernel is zero-init) so that all paths carry signal
    for name in store.leaf_names():
      leaf = store.leaf(name)
      std = 0.05 if name.endswith("kernel") and "head" in name else (0.05 if name.endswith(("bias", "scale")) else 0.0)
      if std:
        leaf.add_((std * torch.randn(leaf.shape, generator=g)).to(dev))
    store.mark_dirty(); store.refresh_shadow()

  for i, t in enumerate(TEACHERS):       # the teachers' checkpoints
    img = torch.zeros((N, RES[t], RES[t], 3), device=dev)
    tree = models[t].init(torch.Generator().manual_seed(11 + i), img)["params"]
    perturb(tree.store)
    f = str(tmp_path / f"{t}.npz")
    u.save_params_npz(f, {"params": tree})
    c[f"{t}_init"] = f
  shapes = {"image": (N, 64, 64, 3), "prof_b": (N, 96, 96, 3)}
  state, _ = distill.make_train_state(models, c, shapes, rng=0, total_steps=c.total_steps)
  perturb(state["params"]["student"].store)
  batch = {"image": torch.rand((N, 64, 64, 3), generator=g) * 2 - 1, "prof_b": torch.rand((N, 96, 96, 3), generator=g) * 2 - 1,
           "labels": torch.nn.functional.one_hot(torch.randint(0, num_classes, (N,), generator=g), num_classes).float()}
  return c, models, state, batch


def _oracle(state, batch, num_classes, distance, distance_kw, mixup_a):
  """fp64: (params64 of the student, loss closure, logits per model, measurements)."""
  import bv_oracle as O
  from big_vision_amd import utils as u
  to64 = lambda tree, grad: O.recover_tree([(k, v.detach().cpu().double().clone().requires_grad_(grad))
                                            for k, v in u.tree_flatten_with_names(tree)[0]])
  p64 = {n: to64(state["params"][n], n == "student") for n in ("student",) + TEACHERS}
  data = {k: v.double() for k, v in batch.items()}
  if mixup_a is not None:
    data = {k: O.mixup(mixup_a, v)[0] for k, v in data.items()}
  cfgs = {"student": VIT, "prof_a": VIT, "prof_b": dict(VIT, depth=1)}
  kw = dict(distance_kw)
  if "epsilon" in kw:
    kw["eps"] = kw.pop("epsilon")

  def forward(student_params):
    logits = {}
    for n in ("student",) + TEACHERS:
      params = student_params if n == "student" else p64[n]
      logits[n] = O.vit_forward(params, data.get(n, data["image"]), num_classes=num_classes, **cfgs[n])[0]
    return logits

  def loss(student_params):
    lg = forward(student_params)
    return sum(D.dist64(distance, lg["student"], lg[t].detach(), **kw).mean() for t in TEACHERS)

  with torch.no_grad():
    lg = forward(p64["student"])
    meas = {}
    for n, x in lg.items():
      meas[f"entropy_{n}"] = D.entropy64(x).mean().item()
      meas[f"task_loss_{n}"] = O.softmax_xent(x, data["labels"]).item()
    for t in TEACHERS:
      meas[f"distill_loss_{t}"] = D.dist64(distance, lg["student"], lg[t], **kw).mean().item()
    meas["distill_loss"] = meas["training_loss"] = sum(meas[f"distill_loss_{t}"] for t in TEACHERS)
  return p64, loss, lg, meas, data


def _run(dev, tmp_path, num_classes, distance, distance_kw, mixup_a=None, **extra):
  import _parity
  from big_vision_amd import utils as u
  from big_vision_amd.trainers.proj.distill import distill
  c, models, state, batch = _setup(dev, tmp_path, num_classes, distance, distance_kw, mixup_a, **extra)
  p64, loss, lg64, meas64, data64 = _oracle(state, batch, num_classes, distance, distance_kw, mixup_a)
  # forward-only paths on the (mixed) inputs of the step
  fns = distill.make_predict_fns(models, c)
  gbatch = {"image": data64["image"].float().to(dev), "prof_b": data64["prof_b"].float().to(dev)}
  for n in ("student",) + TEACHERS:
    logits, out = fns[f"{n}_fwd"](state, gbatch)
    assert (logits.cpu().double() - lg64[n]).abs().max() <= 5e-2, n
    assert out["logits"] is logits
  teachers_before = {t: state["params"][t].store.master.clone() for t in TEACHERS}
  step_batch = {k: v.to(dev) for k, v in batch.items()}
  if mixup_a is not None:
    step_batch["mixup_a"] = mixup_a
  state, meas = distill.make_update_fn(models, c)(state, 0, step_batch)
  # every measurement, by name and value
  assert set(meas) == set(meas64) | {"l2_grads", "l2_params", "l2_updates"}
  for k, want in meas64.items():
    print(f"[distill] {distance} {k}: {meas[k].item():.6f} vs fp64 {want:.6f}")
    assert abs(meas[k].item() - want) <= 1e-2 * abs(want), (k, meas[k].item(), want)
  # gradients of the student's leaves
  ref = loss(p64["student"])
  ref.backward()
  gref = {k: v.grad for k, v in u.tree_flatten_with_names(p64["student"])[0]}
  store = state["params"]["student"].store
  gours = {k: v.detach().cpu().double() for k, v in u.tree_flatten_with_names(store.tree("grad"))[0]}
  fl = _parity.bf16_floor(loss, p64["student"])
  gnorm, _ = _parity.compare_grads(f"distill {distance} {distance_kw} classes={num_classes}", gref, gours, floor=fl)
  assert abs(meas["l2_grads"].item() - gnorm) <= 2e-2 * gnorm
  for t in TEACHERS:     # the teachers are bit-identical after the step, and never got a gradient buffer
    assert torch.equal(state["params"][t].store.master, teachers_before[t]), t
    assert state["params"][t].store.grad is None
  for k, v in meas.items():
    assert math.isfinite(float(v)), k
  return c, models, state, fns, gbatch, lg64


def test_kl_t2_with_mixup(dev, tmp_path):
  """The reference's default distance at t = 2; image, labels and prof_b's own 96 px input mixed under one given a."""
  _run(dev, tmp_path, 10, "kl", dict(t=2.0), mixup_a=0.8)


def test_hard_with_label_smoothing(dev, tmp_path):
  _run(dev, tmp_path, 24, "hard", dict(ls=0.1))


def test_euclidean(dev, tmp_path):
  _run(dev, tmp_path, 24, "euclidean", {})


def test_kl_on_the_bf16_residual_stream(dev, tmp_path):
  _run(dev, tmp_path, 24, "kl", dict(t=1.0), mixup_a=0.7, residual_stream="bfloat16")


def test_predict_fns_evaluator_and_checkpoint(dev, tmp_path):
  import numpy as np
  from big_vision_amd import utils as u
  from big_vision_amd.evaluators.proj.distill import distance
  from big_vision_amd.trainers.proj.distill import distill
  c, models, state, batch = _setup(dev, tmp_path, 10, "kl", dict(t=2.0))
  p64, _, lg64, _, _ = _oracle(state, batch, 10, "kl", dict(t=2.0), None)
  fns = distill.make_predict_fns(models, c)
  gbatch = {k: v.to(dev) for k, v in batch.items()}
  # teacher ensemble: mean softmax.  A logit error of 5e-2 moves a probability by at most a factor exp(+-0.1)
  probs, out = fns["teacher_ensemble_fwd"](state, gbatch)
  assert out == {}
  want = sum(torch.softmax(lg64[t], -1) for t in TEACHERS) / len(TEACHERS)
  assert (probs.double().sum(-1).cpu() - 1).abs().max() <= 1e-5
  assert ((probs.cpu().double() - want).abs() <= (math.exp(0.1) - 1) * want + 1e-7).all()
  (_, out_s), (p_t, out_t) = fns["student_teacher_ensemble_fwd"](state, gbatch)
  assert torch.equal(p_t, probs) and "logits" in out_s
  # evaluator: two batches, the second with a partial mask
  g = torch.Generator().manual_seed(5)
  b2 = {"image": (torch.rand((N, 64, 64, 3), generator=g) * 2 - 1).to(dev), "prof_b": (torch.rand((N, 96, 96, 3), generator=g) * 2 - 1).to(dev)}
  masks = [torch.ones(N), torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0, 0.0])]
  batches = [{**{k: v for k, v in gbatch.items() if k != "labels"}, "_mask": masks[0]}, {**b2, "_mask": masks[1]}]
  dists = [dict(kind="kl", t=2), dict(kind="agree", k=3), dict(kind="euclidean")]
  ev = distance.Evaluator(fns["student_prof_b_fwd"], batches, dists)
  got = dict(ev.run(state))
  assert list(got)[:4] == ["kind=kl_t=2/all", "kind=kl_t=2/avg", "kind=kl_t=2/min", "kind=kl_t=2/max"]
  assert set(got) == {f"{n}/{s}" for n in ("kind=kl_t=2", "kind=agree_k=3", "kind=euclidean") for s in ("all", "avg", "min", "max")}
  # reference: the fp64 distance on the logits the two models produce for these batches
  ref = {n: [] for n in ("kind=kl_t=2", "kind=agree_k=3", "kind=euclidean")}
  for b, m in zip(batches, masks):
    (ls_, _), (lt_, _) = fns["student_prof_b_fwd"](state, {k: v for k, v in b.items() if k != "_mask"})
    keep = m.bool()
    ref["kind=kl_t=2"].append(D.dist64("kl", ls_.cpu(), lt_.cpu(), t=2.0)[keep])
    ref["kind=agree_k=3"].append(D.dist64("agree", ls_.cpu(), lt_.cpu(), k=3)[keep])
    ref["kind=euclidean"].append(D.dist64("euclidean", ls_.cpu(), lt_.cpu())[keep])
  for n, parts in ref.items():
    want = torch.cat(parts)
    all_ = got[f"{n}/all"]
    assert all_.shape == (N + 3,)
    if "agree" in n:
      assert np.array_equal(all_, want.numpy())
    else:      # the kernel's own tolerance on the masked rows (legacy rtol 1e-5 / atol 1e-6 of a loss value)
      np.testing.assert_allclose(all_, want.numpy(), rtol=1e-5, atol=1e-6)
    assert (got[f"{n}/avg"], got[f"{n}/min"], got[f"{n}/max"]) == (np.mean(all_), np.min(all_), np.max(all_))
  # checkpoint: the student and the optimizer, no teacher leaf; it resumes
  f = str(tmp_path / "ckpt.npz")
  distill.save_checkpoint(f, state)
  keys = set(u.npload(f))
  assert all(k.startswith(("params/", "opt/")) for k in keys) and not [k for k in keys if "prof_" in k]
  assert len([k for k in keys if k.startswith("params/")]) == len(state["params"]["student"].store.leaf_names())
  before = state["params"]["student"].store.master.clone()
  state["params"]["student"].store.master.zero_()
  distill.load_checkpoint(f, state)
  assert torch.equal(state["params"]["student"].store.master, before)
