"""SGD-momentum (big_vision.momentum_hp = optax.trace) and SGD (big_vision.sgd = optax.identity) through the fused
optimizer kernel (bv_trace_step), and fine-tuning from a checkpoint (config.model_init):

- the executed reference's fixtures (tests/golden/refmomentum_*.npz from tools/make_momentum_golden.py, and
  refoptax_sgd.npz): three steps, parameters, frozen leaves, bf16 shadow and the final state tree;
- the "fsdp" placement on 2 and 4 ranks against the single-process step;
- checkpoint resume: 2 steps + save + load + 1 step is bit-identical to 3 steps, replicated and sharded;
- a configs/transfer.py step: a small tok ViT against the fp64 oracle, and a real B/32 at 384 px."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import _bounds as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("refmomentum_") and f.endswith(".npz")) + ["refoptax_sgd"]
FSDP_STRATEGY = [(".*", "fsdp(axis='data', min_size_to_shard_mb=0)")]


@pytest.mark.parametrize("fixture", FIXTURES)
def test_momentum_follows_the_executed_reference(dev, fixture):
  from big_vision_amd import optax as bv_optax
  from big_vision_amd import utils as u
  from big_vision_amd.compat.ml_collections import ConfigDict
  from big_vision_amd.params import Entry, ParamStore
  z = np.load(os.path.join(GOLDEN, f"{fixture}.npz"))
  meta = json.loads(bytes(z["meta"]).decode())
  cfg = ConfigDict(meta["config"])
  names = [k[len("param/"):] for k in z.files if k.startswith("param/")]
  frozen = set(bv_optax.frozen_leaves(cfg, names))
  store = ParamStore([Entry(n, z[f"param/{n}"].shape, lambda gen, shape: torch.zeros(shape)) for n in names], dev,
                     frozen=frozen)
  store.load_tree({n: torch.from_numpy(np.asarray(z[f"param/{n}"], np.float32)) for n in names})
  store.refresh_shadow()
  opt, sched_fns = bv_optax.make(cfg, store, sched_kw=dict(meta["sched_kw"]))
  assert len(sched_fns) == meta["n_schedules"]
  okw = meta["config"].get("optax") or {}
  bf16_acc = meta["config"]["optax_name"] == "big_vision.momentum_hp" and str(okw.get("dtype", "bfloat16")) == "bfloat16"
  assert opt.kind == ("trace" if meta["config"]["optax_name"] == "big_vision.momentum_hp" else "identity")
  ref = {n: np.asarray(z[f"param/{n}"], np.float64) for n in names}
  n_tr = store.trainable_count
  store.want_grads = True
  store.ensure_grad()
  for step in range(meta["steps"]):
    store.zero_grad()
    for n in names:
      if n not in frozen:
        store.leaf(n, "grad").copy_(torch.from_numpy(np.asarray(z[f"grad/{step}/{n}"], np.float32)))
    snap = B.snapshot_opt(opt)
    opt.step()
    torch.cuda.synchronize()
    assert bv_optax.get_count(opt) == step + 1
    # this step per element (parameters, accumulators, statistics) from the state the kernel stored before it, on the
    # fixture's gradients and configuration (tests/_bounds.py); the fixture tolerances below cap the model bounds
    B.check_opt_step(opt, snap, f"{fixture} step {step}")
    for n in names:
      upd = np.asarray(z[f"update/{step}/{n}"], np.float64)
      ref[n] = ref[n] + upd
      got = store.leaf(n).detach().cpu().double().numpy()
      if n in frozen:
        assert np.array_equal(got, np.asarray(z[f"param/{n}"], np.float32).astype(np.float64)), f"frozen leaf {n} moved"
        continue
      # fp32 against float64, plus one bf16 rounding of the trace per step (tests/test_reference_optax_gpu.py's bound)
      tol = 2e-6 * max(1.0, float(np.max(np.abs(ref[n])))) + (2.0 ** -8 * float(np.max(np.abs(upd))) * (step + 1) if bf16_acc else 0.0)
      assert float(np.max(np.abs(got - ref[n]))) <= tol, (step, n, float(np.max(np.abs(got - ref[n]))), tol)
    assert torch.equal(store.shadow[:n_tr], store.master[:n_tr].to(torch.bfloat16)), "shadow != bf16(master)"
  got_state = {k: np.asarray(v.detach().cpu().float().numpy() if torch.is_tensor(v) else v, np.float64)
               for k, v in u.tree_flatten_with_names(opt.state_tree())[0]}
  assert set(got_state) == set(meta["state_names"]), sorted(set(got_state) ^ set(meta["state_names"]))[:8]
  for k in meta["state_names"]:
    want = np.asarray(z[f"state/{k}"], np.float64)
    assert got_state[k].shape == want.shape, (k, got_state[k].shape, want.shape)
    scale = max(1e-30, float(np.max(np.abs(want))))
    assert float(np.max(np.abs(got_state[k] - want))) <= (1e-2 if bf16_acc else 2e-5) * scale, k


@pytest.mark.parametrize("world", [2, 4])
def test_fsdp_momentum_matches_single_process(dev, world):
  sys.path.insert(0, os.path.join(ROOT, "tests"))
  import test_dp_two_ranks_gpu as T
  T.test_two_ranks_match_single_process(dev, world, {**T.FSDP, "optax_name": "big_vision.momentum_hp"})


# ------------------------------------------------------------------------------------------------ resume --
TINY = dict(width=64, depth=2, mlp_dim=128, num_heads=2, patch_size=(16, 16), pool_type="tok")


def _tiny_cfg(**kw):
  from big_vision_amd.compat.ml_collections import ConfigDict
  c = ConfigDict(dict(lr=0.05, wd=None, grad_clip_norm=1.0, optax_name="big_vision.momentum_hp", total_steps=10,
                      schedule=dict(decay_type="cosine", warmup_steps=0), model_name="vit", model=TINY,
                      num_classes=10, loss="softmax_xent"))
  for k, v in kw.items():
    c[k] = v
  return c


def _bits(state):
  from big_vision_amd import utils as u
  st = state["params"].store
  tree = {k: v.detach().cpu().clone() for k, v in u.tree_flatten_with_names(st.full_tree())[0]}
  opt = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else np.asarray(v))
         for k, v in u.tree_flatten_with_names(state["opt"].state_tree())[0]}
  return tree, opt, st.shadow.detach().cpu().clone()


def _grad_steps(state, first, count):
  """`count` optimizer steps on seeded gradients (a fixed function of the step index, so that the arithmetic is the
  same whichever process runs the step)."""
  st, opt = state["params"].store, state["opt"]
  st.want_grads = True
  st.ensure_grad()
  for k in range(first, first + count):
    gen = torch.Generator().manual_seed(100 + k)
    st.zero_grad()
    for n in st.leaf_names():
      gl = st.leaf(n, "grad")
      gl.copy_((0.05 * torch.randn(gl.shape, generator=gen)).to(gl.device))
    opt.step()
  torch.cuda.synchronize()
  return state


@pytest.mark.parametrize("fsdp", [False, True], ids=["replicated", "sharded"])
def test_checkpoint_resume_is_bit_identical(dev, tmp_path, fsdp):
  """2 steps, save_train_state, load_train_state into a fresh train state, 1 step == 3 uninterrupted steps, bit for
  bit: parameters, bf16 shadow and the optimizer state (bf16 trace, schedule count)."""
  from big_vision_amd import train
  from big_vision_amd import utils as u
  cfg = _tiny_cfg(**({"sharding_strategy": FSDP_STRATEGY} if fsdp else {}))
  _, model = train.get_model(cfg)
  shape = (4, 64, 64, 3)

  def fresh():
    s, _ = train.make_train_state(model, cfg, shape, rng=0, total_steps=cfg.total_steps)
    assert s["opt"].sharded == fsdp and s["opt"].kind == "trace" and s["opt"].mu.dtype == torch.bfloat16
    return s
  a = _grad_steps(fresh(), 0, 3)
  b = _grad_steps(fresh(), 0, 2)
  f = str(tmp_path / "ckpt.npz")
  u.save_train_state(f, b)
  c = u.load_train_state(f, fresh())
  assert c["opt"].count == 2
  c = _grad_steps(c, 2, 1)
  pa, oa, sa = _bits(a)
  pc, oc, sc = _bits(c)
  assert not torch.equal(pa["head/kernel"], _bits(fresh())[0]["head/kernel"])      # the steps did move the weights
  assert set(pa) == set(pc) and all(torch.equal(pa[k], pc[k]) for k in pa), "parameters differ after resume"
  assert set(oa) == set(oc) and any(k.startswith("1/0/0/") for k in oa)
  for k in oa:
    va, vc = oa[k], oc[k]
    assert (torch.equal(va, vc) if torch.is_tensor(va) else np.array_equal(va, vc)), k
  n_tr = a["params"].store.trainable_count
  assert torch.equal(sa[:n_tr], sc[:n_tr])


# -------------------------------------------------------------------------------------------- fine-tune --
def _transfer_cfg(model, model_init, num_classes=10):
  from big_vision_amd.compat.ml_collections import ConfigDict
  want = json.load(open(os.path.join(GOLDEN, "transfer_configs.json")))["model=vit-i21k-augreg-b/32,dataset=cifar10"]
  cfg = {k: want[k] for k in ("optax_name", "optax", "grad_clip_norm", "wd", "loss", "lr", "schedule", "total_steps",
                              "model_name", "model_load") if k in want}
  cfg.update(model=model, model_init=model_init, num_classes=num_classes)
  assert cfg["optax_name"] == "big_vision.momentum_hp" and cfg["model_load"]["dont_load"] == ["head/kernel", "head/bias"]
  return ConfigDict(cfg), want


def _save_pretrained(path, model_cfg, res=224, classes=1000, seed=11):
  from big_vision_amd import utils as u
  from big_vision_amd.models import vit
  from big_vision_amd.params import ParamStore
  m = vit.Model(classes, **model_cfg)
  st = ParamStore(m.entries("", m.grid((1, res, res, 3))), "cpu")
  st.init_random(seed)
  g = torch.Generator().manual_seed(seed)
  head = st.leaf("head/kernel")
  head.copy_(0.02 * torch.randn(head.shape, generator=g))      # a "trained" head: not the zero init
  u.save_params_npz(path, dict(st.tree()))


def test_transfer_step_small_tok_vit_matches_fp64(dev, tmp_path):
  """configs/transfer.py (B/32 -> cifar10) with a small-width tok ViT of the same patch size: pretrained at 224 px
  with a 1000-class head, fine-tuned at 384 px (12 x 12 + cls = 145 tokens) with a new 10-class head."""
  import bv_oracle as O
  import _parity
  from big_vision_amd import train
  from big_vision_amd import utils as u
  mcfg = dict(width=64, depth=2, mlp_dim=128, num_heads=2, patch_size=(32, 32), pool_type="tok")
  f = str(tmp_path / "pretrained.npz")
  _save_pretrained(f, mcfg)
  config, want = _transfer_cfg(mcfg, f)
  _, model = train.get_model(config)
  g = torch.Generator().manual_seed(3)
  n, res = 4, 384
  image = torch.rand((n, res, res, 3), generator=g) * 2 - 1
  labels = torch.nn.functional.one_hot(torch.randint(0, 10, (n,), generator=g), 10).float()
  state, sched_fns = train.make_train_state(model, config, tuple(image.shape), rng=0, total_steps=config.total_steps)
  store, opt = state["params"].store, state["opt"]
  assert store.leaf("pos_embedding").shape == (1, 144, 64) and opt.kind == "trace" and opt.mu.dtype == torch.bfloat16
  # dont_load keeps the new head at its zero init, which leaves every other gradient at zero on step 0: give it a
  # value so that the parity below carries signal through the whole network
  head = store.leaf("head/kernel")
  head.copy_((0.02 * torch.randn(head.shape, generator=g)).to(dev))
  store.mark_dirty(); store.refresh_shadow()
  pre = u.load_params(f)
  assert torch.equal(store.leaf("Transformer/encoder_norm/scale").cpu(),
                     torch.as_tensor(np.asarray(pre["Transformer"]["encoder_norm"]["scale"], np.float32)))
  params64 = O.recover_tree([(k, v.detach().cpu().double().clone().requires_grad_(True))
                             for k, v in u.tree_flatten_with_names(state["params"])[0]])
  p0 = {k: v.detach().clone() for k, v in u.tree_flatten_with_names(state["params"])[0]}
  loss_ref, _ = O.classification_step_loss(params64, image.double(), labels.double(), model_cfg=mcfg, num_classes=10,
                                           loss="softmax_xent")
  state, meas = train.make_update_fn(model, config)(state, 0, {"image": image.to(dev), "labels": labels.to(dev)})
  torch.cuda.synchronize()
  train.check_finite(meas)
  assert abs(meas["training_loss"].item() - loss_ref.item()) <= 1e-2 * abs(loss_ref.item())
  loss_ref.backward()
  gref = {k: v.grad for k, v in u.tree_flatten_with_names(params64)[0]}
  gours = {k: v.detach().cpu().double() for k, v in u.tree_flatten_with_names(store.tree("grad"))[0]}
  gnorm, _ = _parity.compare_grads("transfer tok 384", gref, gours)
  assert abs(meas["l2_grads"].item() - gnorm) <= 2e-2 * gnorm
  # fp64 restatement of the first momentum step: t = c g (c = min(1, clip / |g|)), stored as bf16; the update is
  # sched(0) * lr * t - transfer's warm-up starts at 0, so the parameters must not move at all on step 0
  s0 = sched_fns[0](0)
  c = min(1.0, want["grad_clip_norm"] / meas["l2_grads"].item())
  trace = {k: torch.as_tensor(np.asarray(v, np.float32)).double() if not torch.is_tensor(v) else v.detach().cpu().double()
           for k, v in u.tree_flatten_with_names(opt.state_tree()["1"]["0"]["0"])[0]}
  assert set(trace) == set(gours)
  for k, t in trace.items():
    t64 = c * gours[k]
    assert (t - t64).abs().max().item() <= 2.0 ** -8 * t64.abs().max().item() + 1e-30, k
  for k, v in u.tree_flatten_with_names(state["params"])[0]:
    upd = s0 * config.lr * trace[k]
    assert (v.detach().cpu().double() - (p0[k].cpu().double() - upd)).abs().max().item() <= 1e-6 + 2e-6 * p0[k].abs().max().item(), k


def test_transfer_step_b32_at_384(dev, tmp_path):
  """The real configs/transfer.py model: ViT-B/32 pretrained at 224 px with a 1000-class head, one step at 384 px
  (L = 145) with batch 8: finite measurements, and the step's loss is the forward-only train.loss_fn's."""
  from big_vision_amd import train
  config, want = _transfer_cfg(None, None)
  f = str(tmp_path / "b32.npz")
  _save_pretrained(f, want["model"])
  config.model, config.model_init = want["model"], f
  _, model = train.get_model(config)
  g = torch.Generator().manual_seed(4)
  image = (torch.rand((8, 384, 384, 3), generator=g) * 2 - 1).to(dev)
  labels = torch.nn.functional.one_hot(torch.randint(0, 10, (8,), generator=g), 10).float().to(dev)
  state, _ = train.make_train_state(model, config, tuple(image.shape), rng=0, total_steps=config.total_steps)
  assert state["params"].store.leaf("pos_embedding").shape == (1, 144, 768)
  lf = train.loss_fn(model, state["params"], image, labels, config).item()
  state, meas = train.make_update_fn(model, config)(state, 0, {"image": image, "labels": labels})
  torch.cuda.synchronize()
  train.check_finite(meas)
  assert abs(meas["training_loss"].item() - lf) <= 1e-3 * abs(lf), (meas["training_loss"].item(), lf)
  assert meas["l2_grads"].item() > 0 and state["opt"].count == 1
