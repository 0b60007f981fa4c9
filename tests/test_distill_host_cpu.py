"""Dry run of the distillation trainer's HOST logic on the CPU (the recorder of test_host_dryrun_cpu.py, copied: every
kernel entry point of both libraries is replaced by a recorder, tensors live on the CPU, values are garbage): what is
launched per step, how `bv_distill_dist` is told to accumulate over the teachers, the data-parallel normaliser, and the
errors a wrong config raises before anything runs."""
import collections
import importlib

import pytest
import torch

from big_vision_amd import _lib, dp, ops
from big_vision_amd import utils as u
from big_vision_amd.compat.ml_collections import ConfigDict
from big_vision_amd.params import ParamStore
from big_vision_amd.trainers.proj.distill import distill

VIT = dict(width=128, depth=2, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="gap")
N, CLASSES = 4, 10


@pytest.fixture()
def dry(monkeypatch):
  calls, args = collections.Counter(), []

  def record(name, *a):
    calls.update([name])
    args.append((name, a))
  monkeypatch.setattr(_lib, "call", record)
  monkeypatch.setattr(ops, "_chk", lambda t, dtype, name: t)
  monkeypatch.setattr(ops, "_stream", lambda: 0)
  monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (1 << 40, 1 << 40))
  monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a: 0)
  monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a: 0)
  return calls, args


def _cfg(tmp_path, teachers=("prof_a", "prof_b"), **kw):
  c = ConfigDict()
  c.lr, c.wd, c.optax_name, c.total_steps, c.grad_clip_norm = 1e-3, 1e-2, "scale_by_adam", 10, 1.0
  c.schedule = dict(decay_type="cosine", warmup_steps=2)
  c.num_classes = CLASSES
  c.student_name, c.student = "vit", dict(VIT)
  c.teachers = list(teachers)
  for i, t in enumerate(teachers):
    c[f"{t}_name"] = "vit"
    c[t] = dict(VIT, depth=1 + i)
  for k, v in kw.items():
    c[k] = v
  models = distill.get_models(c)
  for t in teachers:                      # a checkpoint per teacher, written with the existing helpers
    m = models[t]
    store = ParamStore(m.entries("", m.grid((N, 32, 32, 3))), "cpu")
    store.init_random(7)
    f = str(tmp_path / f"{t}.npz")
    u.save_params_npz(f, {"params": store.tree()})
    c[f"{t}_init"] = f
  return c, models


def _batch(**extra):
  return {"image": torch.zeros((N, 32, 32, 3)), "labels": torch.zeros((N, CLASSES)), **extra}


def _dist_args(args):
  keys = ("kind", "student", "teacher", "per_row", "loss_sum", "dstudent", "accumulate", "n", "C", "n_global", "t", "ls",
          "eps", "k", "stream")
  return [dict(zip(keys, a)) for name, a in args if name == "bv_distill_dist"]


def test_one_step_launch_multiset(dry, tmp_path):
  calls, args = dry
  cfg, models = _cfg(tmp_path, mixup=dict(p=0.2, fold_in=None), distance="kl", distance_kw=dict(t=2.0))
  state, _ = distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, total_steps=10, device="cpu")
  fn = distill.make_update_fn(models, cfg)
  calls.clear(); args.clear()
  state, meas = fn(state, 0, _batch())
  assert calls["bv_mixup"] == 2                                   # image and labels, one coefficient
  mix = [a[2] for name, a in args if name == "bv_mixup"]
  assert mix[0] == mix[1]
  assert calls["bv_distill_dist"] == 2 and calls["bv_distill_entropy"] == 3 and calls["bv_softmax_xent"] == 3
  assert calls["bv_attn_fwd"] == 2 + 1 + 2 and calls["bv_attn_bwd"] == 2   # student + two teachers forward, student backward
  assert calls["bv_adam_step"] == 1 and calls["bv_sqnorm"] == 1
  d = _dist_args(args)
  assert [x["accumulate"] for x in d] == [0, 1]
  assert d[0]["dstudent"] == d[1]["dstudent"] and d[0]["dstudent"] is not None
  assert d[0]["student"] == d[1]["student"] and d[0]["teacher"] != d[1]["teacher"]
  assert all(x["kind"] == _lib.DISTILL_KINDS["kl"] and x["t"] == 2.0 and x["n"] == N and x["C"] == CLASSES
             and x["n_global"] == N and x["per_row"] is None for x in d)
  assert d[0]["loss_sum"] != d[1]["loss_sum"]
  xent = [a for name, a in args if name == "bv_softmax_xent"]
  assert all(a[3] is None for a in xent)                          # forward only
  assert set(meas) == {"distill_loss", "distill_loss_prof_a", "distill_loss_prof_b", "training_loss", "entropy_student",
                       "entropy_prof_a", "entropy_prof_b", "task_loss_student", "task_loss_prof_a", "task_loss_prof_b",
                       "l2_grads", "l2_params", "l2_updates"}
  assert set(state["params"]) == {"student", "prof_a", "prof_b"}


def test_per_model_inputs_are_mixed_with_the_same_coefficient_and_labels_are_optional(dry, tmp_path):
  calls, args = dry
  cfg, models = _cfg(tmp_path, teachers=("prof_b",), mixup=dict(p=0.2, fold_in=None), distance="hard",
                     distance_kw=dict(ls=0.1))
  shapes = {"image": (N, 32, 32, 3), "prof_b": (N, 48, 48, 3)}
  state, _ = distill.make_train_state(models, cfg, shapes, rng=0, total_steps=10, device="cpu")
  fn = distill.make_update_fn(models, cfg)
  calls.clear(); args.clear()
  batch = {"image": torch.zeros((N, 32, 32, 3)), "prof_b": torch.zeros((N, 48, 48, 3)), "mixup_a": 0.75}
  _, meas = fn(state, 0, batch)
  mix = [a for name, a in args if name == "bv_mixup"]
  assert len(mix) == 2 and all(a[2] == 0.75 for a in mix)
  assert sorted(a[4] for a in mix) == [32 * 32 * 3, 48 * 48 * 3]   # the teacher runs on its own, larger input
  assert calls["bv_softmax_xent"] == 0 and "task_loss_student" not in meas
  d = _dist_args(args)
  assert len(d) == 1 and d[0]["kind"] == _lib.DISTILL_KINDS["hard"] and abs(d[0]["ls"] - 0.1) < 1e-7 and d[0]["accumulate"] == 0


class _FakeComm(dp.Comm):
  """Two 'ranks' without a process group (test_host_dryrun_cpu.py)."""

  def __init__(self, log):
    self.enabled, self.group, self.rank, self.size, self.log, self.active = False, None, 1, 2, log, True

  def all_reduce_sum_(self, flat, bucket_bytes=0):
    self.log.append(("all_reduce", flat.storage_offset(), flat.numel()))

  def all_reduce_scalars_(self, t):
    self.log.append(("scalars", t.numel()))

  def all_gather_flat_(self, flat, lo, hi, S):       # the fsdp exchange of the updated slices: recorded only
    self.log.append(("all_gather_flat", lo, hi))

  def broadcast_ranges_(self, flat, bounds):
    self.log.append(("broadcast_ranges", tuple(bounds)))

  def barrier(self):
    pass


def test_two_ranks_normalise_by_the_global_batch(dry, tmp_path):
  calls, args = dry
  log = []
  comm = _FakeComm(log)
  cfg, models = _cfg(tmp_path)
  state, _ = distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, comm=comm, total_steps=10, device="cpu")
  fn = distill.make_update_fn(models, cfg, comm=comm)
  calls.clear(); args.clear(); log.clear()
  fn(state, 0, _batch())
  assert all(x["n"] == N and x["n_global"] == 2 * N for x in _dist_args(args))
  assert all(a[5] == 2 * N for name, a in args if name == "bv_distill_entropy")
  assert all(a[6] == 2 * N for name, a in args if name == "bv_softmax_xent")
  assert ("scalars", 2 + 3 + 3) in log                            # every measurement in ONE all-reduce
  reduced = sum(e[2] for e in log if e[0] == "all_reduce")
  assert reduced == state["params"]["student"].store.trainable_count   # the student's gradients, nothing of a teacher


def test_config_errors(dry, tmp_path):
  cfg, models = _cfg(tmp_path)
  del cfg["prof_b_init"]
  with pytest.raises(KeyError):
    distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, total_steps=10, device="cpu")
  cfg, models = _cfg(tmp_path, distance="cosine")
  with pytest.raises(AssertionError, match="Unknown kind of distance cosine"):
    distill.make_update_fn(models, cfg)
  cfg, models = _cfg(tmp_path)
  cfg["prof_a_init"] = "gs://bucket/teacher.npz"
  with pytest.raises(FileNotFoundError, match="remote checkpoints cannot be opened"):
    distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, total_steps=10, device="cpu")
  cfg["prof_a_init"] = str(tmp_path / "missing.npz")
  with pytest.raises(FileNotFoundError, match="no such checkpoint file"):
    distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, total_steps=10, device="cpu")


def test_unknown_distance_in_dist_raises_like_the_reference():
  from big_vision_amd.evaluators.proj.distill import distance
  with pytest.raises(AssertionError, match="Unknown kind of distance"):
    distance.dist(torch.zeros(2, 4), torch.zeros(2, 4), "cosine")
  assert distance.get_dist_fn(kind="kl", t=2) is distance.get_dist_fn(kind="kl", t=2)


def test_head_bias_init_and_student_only_checkpoint(dry, tmp_path):
  cfg, models = _cfg(tmp_path, init_head_bias=-6.9)
  state, _ = distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, total_steps=10, device="cpu")
  store = state["params"]["student"].store
  assert torch.allclose(store.leaf("head/bias"), torch.full((CLASSES,), -6.9))
  f = str(tmp_path / "ckpt.npz")
  distill.save_checkpoint(f, state)
  keys = set(u.npload(f))
  assert keys and all(k.startswith(("params/", "opt/")) for k in keys)
  assert "params/head/bias" in keys and not [k for k in keys if "prof_" in k]
  n_student = len(store.leaf_names())
  assert len([k for k in keys if k.startswith("params/")]) == n_student


def test_getfirst_takes_the_first_key_present():
  d = {"image": 1, "prof": 2}
  assert distill.getfirst(d, "prof", "image") == 2 and distill.getfirst(d, "student", "image") == 1
  with pytest.raises(KeyError):
    distill.getfirst(d, "x", "y")


def test_fsdp_on_two_ranks_shards_the_student_and_its_tree_follows_the_store(dry, tmp_path, monkeypatch):
  """config.sharding_strategy = fsdp under the fake two-rank Comm: the optimizer is the sharded one, the student's
  fp32 master is sharded (no whole flat master stays alive behind the tree handed out in train_state), the tree's
  leaves are the store's current views, and the step hands the gradients to the sharded sync, not to an all-reduce."""
  calls, args = dry
  log = []
  comm = _FakeComm(log)
  cfg, models = _cfg(tmp_path, sharding_strategy=[(".*", "fsdp(axis='data', min_size_to_shard_mb=0)")])
  state, _ = distill.make_train_state(models, cfg, (N, 32, 32, 3), rng=0, comm=comm, total_steps=10, device="cpu")
  store = state["params"]["student"].store
  assert state["opt"].sharded and store.master_sharded and store.master is None
  fresh = dict(u.tree_flatten_with_names(store.tree())[0])
  held = dict(u.tree_flatten_with_names(state["params"]["student"])[0])
  assert set(held) == set(fresh)
  for k, v in held.items():       # the same storage as a tree taken now: nothing of the unsharded master is referenced
    assert v.data_ptr() == fresh[k].data_ptr() and v.dtype == fresh[k].dtype, k
  for t in ("prof_a", "prof_b"):  # teachers stay whole and replicated
    assert not state["params"][t].store.master_sharded
  fn = distill.make_update_fn(models, cfg, comm=comm)
  # the sharded sync sums every gradient range onto its owner with torch.distributed.reduce: recorded, not run
  monkeypatch.setattr(torch.distributed, "reduce", lambda t, dst, group=None: log.append(("reduce", t.numel(), dst)))
  calls.clear(); args.clear(); log.clear()
  fn(state, 0, _batch())
  assert calls["bv_distill_dist"] == 2 and calls["bv_adam_step"] == 1
  # every student gradient is summed onto its owner, once; what is all-reduced is the packed small replicated
  # entries (ParamStore.exchange_small_), never the gradient buffer
  assert sum(e[1] for e in log if e[0] == "reduce") == store.trainable_count
  assert all(e[2] == store.master_small.numel() for e in log if e[0] == "all_reduce")
  assert [e for e in log if e[0] == "all_gather_flat"]                           # the owners' updated slices go round


def test_alias_imports_resolve():
  t = importlib.import_module("big_vision.trainers.proj.distill.distill")
  e = importlib.import_module("big_vision.evaluators.proj.distill.distance")
  from big_vision_amd.evaluators.proj.distill import distance
  assert t is distill and e is distance
  fns = distill.make_predict_fns({"student": None, "a": None, "b": None}, ConfigDict(dict(teachers=["a", "b"])))
  assert set(fns) == {"student_fwd", "a_fwd", "b_fwd", "teacher_ensemble_fwd", "student_a_fwd", "student_b_fwd",
                      "student_teacher_ensemble_fwd"}
