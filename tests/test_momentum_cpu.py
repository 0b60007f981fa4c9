"""SGD-momentum (big_vision.momentum_hp) and SGD (big_vision.sgd) on the host side, and checkpoint init for fine-tuning:
hyper-parameter parsing, the reference's optimizer-state names, the launch the step makes (dry run: every libbvhip
entry point replaced by a recorder), configs/transfer.py as the reference resolves it, and `make_train_state` with
`config.model_init`.  No GPU."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_vision_amd import _lib, ops
from big_vision_amd import optax as bv_optax
from big_vision_amd import utils as u
from big_vision_amd.compat.ml_collections import ConfigDict
from big_vision_amd.params import Entry, ParamStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("BV_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "big_vision")),
                                     reason="the reference checkout is not available")
SCHED_KW = dict(total_steps=10, batch_size=8, data_size=100)


@pytest.fixture()
def dry(monkeypatch):
  calls = collections.Counter()
  monkeypatch.setattr(_lib, "call", lambda name, *a: calls.update([name]))
  monkeypatch.setattr(ops, "_chk", lambda t, dtype, name: t)
  monkeypatch.setattr(ops, "_stream", lambda: 0)
  return calls


def _store(shapes, frozen=(), leaf_init=None):
  init0 = lambda gen, shape: torch.zeros(shape)
  return ParamStore([Entry(n, tuple(s), init0) for n, s in shapes.items()], "cpu", frozen=set(frozen))


SHAPES = {"img/kernel": (32, 48), "img/bias": (48,), "txt/kernel": (16, 64), "t": (1,)}


def _opt(optax_name, optax=None, **kw):
  cfg = ConfigDict(dict(lr=0.01, optax_name=optax_name, schedule=dict(decay_type="cosine"), **kw))
  if optax is not None:
    cfg.optax = optax
  return bv_optax.make(cfg, _store(SHAPES), sched_kw=SCHED_KW)[0]


def test_momentum_hp_defaults_are_the_references():
  opt = _opt("big_vision.momentum_hp")
  assert opt.kind == "trace" and opt.momentum == 0.9 and opt.nesterov is False
  assert opt.mu.dtype == torch.bfloat16 and opt.mu.numel() == opt.store.trainable_count and opt.nu is None


@pytest.mark.parametrize("dtype", ["float32", torch.float32, "bfloat16", torch.bfloat16])
def test_momentum_hp_arguments(dtype):
  opt = _opt("big_vision.momentum_hp", dict(momentum=0.8, dtype=dtype, nesterov=True))
  assert opt.momentum == pytest.approx(0.8) and opt.nesterov is True
  assert opt.mu.dtype == (torch.float32 if "float32" in str(dtype) else torch.bfloat16)


def test_sgd_keeps_no_state():
  opt = _opt("big_vision.sgd")
  assert opt.kind == "identity" and opt.mu is None and opt.nu is None


@pytest.mark.parametrize("name,optax", [("big_vision.momentum_hp", dict(b1=0.9)),
                                        ("big_vision.momentum_hp", dict(decay=0.9)),
                                        ("big_vision.sgd", dict(momentum=0.9))])
def test_unknown_arguments_are_refused(name, optax):
  with pytest.raises(TypeError, match="unexpected keyword"):
    _opt(name, optax)


def test_unsupported_accumulator_dtype_is_refused():
  with pytest.raises(ValueError, match="dtype"):
    _opt("big_vision.momentum_hp", dict(dtype="float16"))


def test_per_example_clip_keeps_raising():
  with pytest.raises(NotImplementedError, match="grad_clip_per_example"):
    _opt("big_vision.momentum_hp", grad_clip_per_example=1.0)


def _names_case(case):
  fix, cfg = case["fixture"], ConfigDict(case["config"])
  z = np.load(os.path.join(GOLDEN, f"{fix}.npz"))
  shapes = {k[len("param/"):]: z[k].shape for k in z.files if k.startswith("param/")}
  frozen = bv_optax.frozen_leaves(cfg, list(shapes))
  return cfg, _store(shapes, frozen)


@pytest.mark.parametrize("case", sorted(json.load(open(os.path.join(GOLDEN, "refmomentum_state_names.json")))))
def test_state_tree_names_are_the_references(case):
  want = json.load(open(os.path.join(GOLDEN, "refmomentum_state_names.json")))[case]
  cfg, store = _names_case(want)
  opt, _ = bv_optax.make(cfg, store, sched_kw=SCHED_KW)
  got = [[k, list(np.shape(np.asarray(v.float() if torch.is_tensor(v) else v)))]
         for k, v in u.tree_flatten_with_names(opt.state_tree())[0]]
  assert sorted(got) == sorted(want["state"])


def test_state_dict_and_tree_round_trip():
  opt = _opt("big_vision.momentum_hp", dict(dtype="float32"))
  g = torch.Generator().manual_seed(0)
  opt.mu.copy_(torch.randn(opt.mu.shape, generator=g))
  opt.count = 5
  tree, sd = opt.state_tree(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
  flat = lambda o: {k: np.asarray(v) for k, v in u.tree_flatten_with_names(o.state_tree())[0]}
  want = flat(opt)
  assert len(want) == len(SHAPES) + 1        # the trace of every leaf + the schedule's count
  other = _opt("big_vision.momentum_hp", dict(dtype="float32"))
  other.load_state_tree(tree)
  got = flat(other)
  assert other.count == 5 and set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
  third = _opt("big_vision.momentum_hp", dict(dtype="float32"))
  third.load_state_dict(sd)
  assert third.count == 5 and torch.equal(third.mu, opt.mu)
  sgd = _opt("big_vision.sgd")
  sgd.count = 3
  sgd2 = _opt("big_vision.sgd")
  sgd2.load_state_tree(sgd.state_tree())
  assert sgd2.count == 3 and bv_optax.get_count(sgd2) == 3


@pytest.mark.parametrize("name", ["big_vision.momentum_hp", "big_vision.sgd"])
def test_dry_step_launches_the_trace_kernel_once(dry, name):
  from big_vision_amd.models.proj.image_text import two_towers
  from big_vision_amd.trainers.proj.image_text import siglip
  img = dict(width=128, depth=2, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="map")
  txt = dict(width=128, depth=2, mlp_dim=256, num_heads=2, vocab_size=50)
  model = two_towers.Model(image=img, text=txt, out_dim=(None, 64), temperature_init=10.0, bias_init=-10.0)
  c = ConfigDict(dict(lr=0.01, optax_name=name, total_steps=10, grad_clip_norm=1.0,
                      schedule=dict(decay_type="cosine", warmup_steps=2)))
  image, text = torch.zeros((8, 32, 32, 3)), torch.ones((8, 8), dtype=torch.int32)
  state, _ = siglip.make_train_state(model, c, tuple(image.shape), tuple(text.shape), rng=0, total_steps=10,
                                     device="cpu")
  fn = siglip.make_update_fn(model, c)
  dry.clear()
  fn(state, None, {"image": image, "labels": text})
  assert dry["bv_trace_step"] == 1 and dry["bv_adam_step"] == 0 and dry["bv_sqnorm"] == 1


@needs_reference
def test_transfer_config_loads_unchanged():
  from big_vision_amd.configs.loader import load_config
  want = json.load(open(os.path.join(GOLDEN, "transfer_configs.json")))
  path = os.path.join(REFERENCE, "big_vision", "configs", "transfer.py")
  for arg, cfg in want.items():
    got = json.loads(json.dumps(load_config(f"{path}:{arg}", reference_root=REFERENCE).to_dict()))
    assert got == cfg, arg
    assert cfg["optax_name"] == "big_vision.momentum_hp" and cfg["grad_clip_norm"] == 1.0


@needs_reference
def test_committed_fixtures_equal_a_fresh_generator_run(tmp_path):
  subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_momentum_golden.py"), str(tmp_path)], check=True,
                 cwd=ROOT, timeout=600, capture_output=True)
  names = sorted(os.listdir(tmp_path))
  assert names == ["refmomentum_frozen_bit.npz", "refmomentum_nesterov_f32.npz", "refmomentum_state_names.json",
                   "refmomentum_transfer.npz", "transfer_configs.json"]
  for n in names:
    if n.endswith(".json"):
      assert json.load(open(tmp_path / n)) == json.load(open(os.path.join(GOLDEN, n))), n
      continue
    a, b = np.load(tmp_path / n), np.load(os.path.join(GOLDEN, n))
    assert sorted(a.files) == sorted(b.files), n
    for k in a.files:
      assert np.array_equal(a[k], b[k]), (n, k)


VIT = dict(width=32, depth=2, mlp_dim=64, num_heads=2, patch_size=(8, 8), pool_type="tok")


def _pretrained(tmp_path, hw=16, classes=1000):
  from big_vision_amd.models import vit
  m = vit.Model(classes, **VIT)
  st = ParamStore(m.entries("", m.grid((1, hw, hw, 3))), "cpu")
  st.init_random(7)
  f = str(tmp_path / "pretrained.npz")
  u.save_params_npz(f, dict(st.tree()))
  return f, {k: v.detach().clone() for k, v in u.tree_flatten_with_names(st.tree())[0]}


def test_make_train_state_loads_model_init(dry, tmp_path):
  from big_vision_amd import train
  from big_vision_amd.models import vit
  f, pre = _pretrained(tmp_path)
  c = ConfigDict(dict(lr=0.01, optax_name="big_vision.momentum_hp", grad_clip_norm=1.0, wd=None, total_steps=10,
                      schedule=dict(decay_type="cosine", warmup_steps=2), model_name="vit", num_classes=10, model=VIT,
                      model_init=f, model_load=dict(dont_load=["head/kernel", "head/bias"])))
  model_mod, model = train.get_model(c)
  shape = (2, 32, 32, 3)
  plain, _ = train.make_train_state(model, ConfigDict({k: v for k, v in c.items() if k not in ("model_init", "model_load")}),
                                    shape, device="cpu", total_steps=10)
  state, _ = train.make_train_state(model, c, shape, device="cpu", total_steps=10)
  got = {k: v.detach() for k, v in u.tree_flatten_with_names(state["params"])[0]}
  init = {k: v.detach() for k, v in u.tree_flatten_with_names(plain["params"])[0]}
  assert set(got) == set(pre)
  for k, v in got.items():
    if k.startswith("head/"):
      assert torch.equal(v, init[k]), k                     # dont_load: the new head keeps its init
    elif k == "pos_embedding":
      assert pre[k].shape == (1, 4, 32) and v.shape == (1, 16, 32)
      want = vit.resample_posemb(pre[k].numpy(), v)
      np.testing.assert_allclose(v.numpy(), want, rtol=0, atol=1e-6)
      assert not torch.equal(v, init[k])
    else:
      assert torch.equal(v, pre[k]), k


@pytest.mark.parametrize("init", ["howto-i21k-B/16", "gs://bucket/ckpt.npz", "/nonexistent/ckpt.npz"])
def test_unreachable_model_init_fails_clearly(dry, init):
  from big_vision_amd import train
  c = ConfigDict(dict(lr=0.01, optax_name="big_vision.sgd", total_steps=10, schedule=dict(decay_type="cosine"),
                      model_name="vit", num_classes=10, model=VIT, model_init=init))
  _, model = train.get_model(c)
  with pytest.raises(FileNotFoundError, match="model_init"):
    train.make_train_state(model, c, (2, 32, 32, 3), device="cpu", total_steps=10)
