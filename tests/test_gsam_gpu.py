"""GSAM / SAM trainer parity (big_vision/trainers/proj/gsam/{gsam,train}.py): the HIP step of
`big_vision_amd.trainers.proj.gsam.train` vs `oracle/bv_oracle.py::classification_step_loss` under fp64 autograd,
called at the clean and at the perturbed weights, with an fp64 restatement of gsam.py:69-122 on top.

The case is the smallest model of tests/test_train_step_gpu.py (width 128, depth 2, mlp 256, 2 heads, patch 16, gap
pooling, 64 x 64 images, n = 6, 24 classes, sigmoid_xent), its zero inits broken the same way.  rho_max = 0.6,
rho_min = 0.1, alpha = 0.6; the step runs at optimizer count 5 of a 10-step linear schedule, so sam_rho = 0.35 lies
strictly between the two.  Bounds: loss rel <= 1e-2 and tests/_parity.py's fixed per-tensor bounds (cosine >= 0.999,
rel-L2 <= 3e-2) where two forward / backward passes meet the fp64 oracle; rounding-error bounds, derived at each
check, where the product's vector stage meets fp64 arithmetic on the product's own buffers."""
import math
import os
import socket
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODEL = dict(width=128, depth=2, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="gap")
N, RES, CLASSES, LOSS = 6, 64, 24, "sigmoid_xent"
COUNT, TOTAL = 5, 10
LR, LR_END = 1e-3, 0.01
GSAM = dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=LR, lr_min=LR_END * LR)
SAM = dict(GSAM, rho_max=0.3, rho_min=0.3, alpha=0.0)
EPS32 = 2.0 ** -23            # fp32 machine epsilon; one rounding is at most EPS32 / 2 relative
TINY32 = 2.0 ** -126          # smallest normal fp32: what a product flushed to zero loses at most


def _cfg(gsam_kw):
  from big_vision_amd.compat.ml_collections import ConfigDict
  c = ConfigDict()
  c.lr, c.wd = LR, 1e-4
  c.schedule = dict(decay_type="linear", linear_end=LR_END)
  c.optax_name = "scale_by_adam"
  c.optax = dict(mu_dtype="float32")
  c.grad_clip_norm = 1.0
  c.total_steps = TOTAL
  c.model_name, c.model, c.num_classes, c.loss = "vit", dict(MODEL), CLASSES, LOSS
  c.gsam = dict(gsam_kw)
  return c


def _batch(seed=3, n=N):
  g = torch.Generator().manual_seed(seed)
  image = torch.rand((n, RES, RES, 3), generator=g) * 2 - 1
  labels = torch.nn.functional.one_hot(torch.randint(0, CLASSES, (n,), generator=g), CLASSES).float()
  return image, labels


def _make(dev, gsam_kw, comm=None):
  """(config, model, state) with the weights every test of this file runs at, at optimizer count COUNT."""
  from big_vision_amd.trainers.proj.gsam import train
  config = _cfg(gsam_kw)
  _, model = train.get_model(config)
  state, _ = train.make_train_state(model, config, (N, RES, RES, 3), rng=0, comm=comm, total_steps=TOTAL)
  store = state["params"].store
  g = torch.Generator().manual_seed(4)
  for name in store.leaf_names():   # break zero / unit inits, as tests/test_train_step_gpu.py::_run does
    leaf = store.leaf(name)
    std = 0.02 if name.endswith("kernel") and "head" in name else (0.05 if name.endswith(("bias", "scale")) else 0.0)
    if std:
      leaf.add_((std * torch.randn(leaf.shape, generator=g)).to(dev))
  store.mark_dirty(); store.refresh_shadow()
  state["opt"].count = COUNT
  return config, model, state


def _named(store, flat):
  """{leaf name: fp64 cpu tensor} of a flat buffer laid out like `store.grad`."""
  from big_vision_amd import utils as u
  store.ensure_grad()
  out = {}
  for k, v in u.tree_flatten_with_names(store.tree("grad"))[0]:
    out[k] = torch.as_strided(flat, tuple(v.shape), v.stride(), v.storage_offset()).detach().cpu().double().clone()
  return out


def _ocfg():
  import bv_oracle as O
  return {**O.decode_variant(MODEL.get("variant")), **MODEL}


def _oracle_grads(params, image, labels, bf16=False):
  """(loss, {name: grad}) of classification_step_loss at `params` ({name: fp64 tensor}) under fp64 autograd."""
  import contextlib
  import bv_oracle as O
  p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
  with (O.bf16_operands() if bf16 else contextlib.nullcontext()):
    loss, _ = O.classification_step_loss(O.recover_tree(list(p.items())), image.double(), labels.double(),
                                         model_cfg=_ocfg(), num_classes=CLASSES, loss=LOSS)
    loss.backward()
  return loss.item(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}


def _sqnorm(g):
  return sum((v ** 2).sum().item() for v in g.values())


def _oracle_gsam(params, image, labels, gsam_kw, bf16=False):
  """fp64 restatement of gsam.py:69-122 around the oracle's two gradients."""
  import bv_oracle as O
  kw = dict(eps=1e-12, minimize_fp=True)
  kw.update(gsam_kw)
  lr = O.create_learning_rate_schedule(TOTAL, decay_type="linear", linear_end=LR_END)(COUNT) * LR
  if kw["lr_max"] == kw["lr_min"]:
    rho = kw["rho_max"]
  else:
    rho = kw["rho_min"] + (kw["rho_max"] - kw["rho_min"]) * (lr - kw["lr_min"]) / (kw["lr_max"] - kw["lr_min"])
  loss, gc = _oracle_grads(params, image, labels, bf16)
  length = math.sqrt(_sqnorm(gc))
  p_sam = {k: params[k] + rho * gc[k] / (length + kw["eps"]) for k in params}
  _, gr = _oracle_grads(p_sam, image, labels, bf16)
  dot, alpha = sum((gr[k] * gc[k]).sum().item() for k in gc), kw["alpha"]
  if kw["minimize_fp"]:
    proj = dot / math.sqrt(_sqnorm(gr))
    g = {k: gr[k] - alpha * (gc[k] - proj * gr[k] / math.sqrt(_sqnorm(gr))) for k in gc}
  else:
    proj = dot / length
    g = {k: gc[k] + alpha * (gr[k] - proj * gc[k] / length) for k in gc}
  return dict(loss=loss, rho=rho, g_clean=gc, p_sam=p_sam, g_robust=gr, g_gsam=g)


@pytest.fixture(scope="module")
def ref(dev):
  """Everything shared and computed once: the batch, the fp64 weights and the oracle's GSAM and SAM chains."""
  from big_vision_amd import utils as u
  _, _, state = _make(dev, GSAM)
  params = {k: v.detach().cpu().double().clone() for k, v in u.tree_flatten_with_names(state["params"])[0]}
  image, labels = _batch()
  return dict(params=params, image=image, labels=labels, gsam=_oracle_gsam(params, image, labels, GSAM),
              sam=_oracle_gsam(params, image, labels, SAM))


def _grad_phase(dev, gsam_kw, image, labels, stages=None):
  from big_vision_amd.trainers.proj.gsam import train
  config, model, state = _make(dev, gsam_kw)
  grad_fn = train.make_grad_fn(model, config)
  loss = grad_fn(state, 0, {"image": image.to(dev), "labels": labels.to(dev)}, stages=stages)
  torch.cuda.synchronize()
  return state, grad_fn, loss.item()


def _floor_at(params, image, labels):
  import _parity
  import bv_oracle as O
  p64 = O.recover_tree([(k, v.detach().clone().requires_grad_(True)) for k, v in params.items()])
  closure = lambda p: O.classification_step_loss(p, image.double(), labels.double(), model_cfg=_ocfg(),
                                                 num_classes=CLASSES, loss=LOSS)[0]
  closure(p64).backward()
  return _parity.bf16_floor(closure, p64)


def test_clean_gradient_and_clean_loss(dev, ref):
  """1. `training_loss` is the CLEAN loss and the kept `g_clean` the clean (local-mean) gradient."""
  import _parity
  stages = {}
  state, grad_fn, loss = _grad_phase(dev, GSAM, ref["image"], ref["labels"], stages)
  o = ref["gsam"]
  print(f"[gsam] clean loss {loss:.6f} oracle {o['loss']:.6f}; sam_rho {stages['sam_rho']:.6f} oracle {o['rho']:.6f}")
  assert abs(loss - o["loss"]) <= 1e-2 * abs(o["loss"])
  store, buf = state["params"].store, grad_fn.buffers()
  assert buf.g_clean.numel() == store.trainable_count and buf.g_clean.dtype == torch.float32
  _parity.compare_grads("gsam clean gradient", o["g_clean"], _named(store, buf.g_clean),
                        floor=_floor_at(ref["params"], ref["image"], ref["labels"]))
  # the rho schedule: strictly inside (rho_min, rho_max) at this count, and the oracle's value
  assert GSAM["rho_min"] < stages["sam_rho"] < GSAM["rho_max"]
  assert abs(stages["sam_rho"] - o["rho"]) <= 1e-6 * o["rho"]
  assert abs(math.sqrt(stages["sq_clean"]) - math.sqrt(_sqnorm(o["g_clean"]))) <= 2e-2 * math.sqrt(_sqnorm(o["g_clean"]))


def test_sam_gradient_is_a_gradient_at_the_perturbed_weights(dev, ref):
  """2. alpha = 0, rho_max = rho_min = 0.3: `store.grad` after the gradient phase (`make_grad_fn`: the step without
  opt.step()) is the gradient at the ORACLE's perturbed weights, the floor measured at those weights."""
  import _parity
  stages = {}
  state, _, _ = _grad_phase(dev, SAM, ref["image"], ref["labels"], stages)
  o = ref["sam"]
  assert stages["sam_rho"] == 0.3 and (stages["a"], stages["b"]) == (1.0, 0.0) and stages["dot"] is None
  store = state["params"].store
  _parity.compare_grads("gsam SAM gradient at the perturbed weights", o["g_robust"], _named(store, store.grad),
                        floor=_floor_at(o["p_sam"], ref["image"], ref["labels"]))
  # ... and not the clean one: the two differ by far more than the bound
  far = max((o["g_robust"][k] - o["g_clean"][k]).norm().item() / o["g_clean"][k].norm().item() for k in o["g_clean"])
  assert far > 10 * _parity.REL_MAX, far


def _reduction_bound(n, threads, per_iter):
  """fp32 partial sums of bv_sqnorm / bv_dot_f32: a thread adds `per_iter` products per iteration over
  ceil(n / (threads * per_iter)) iterations, a workgroup tree of 8 levels follows, the rest is fp64.  Every term
  passes through at most d = per_iter * iterations + 8 fp32 additions and one product rounding, each at most
  EPS32 / 2 relative: |error| <= (d + 1) * EPS32 / 2 * sum |terms| (first order)."""
  d = per_iter * math.ceil(n / (threads * per_iter)) + 8
  return (d + 1) * EPS32 / 2


@pytest.mark.parametrize("minimize_fp", [True, False])
def test_vector_stage_on_the_products_own_gradients(dev, ref, minimize_fp):
  """3. With the product's own g_clean and g_robust: its reductions, coefficients, perturbed master, shadow and
  g_gsam against fp64 arithmetic on those same buffers; master and shadow are back bit for bit before opt.step()."""
  from big_vision_amd.trainers.proj.gsam import gsam, train
  kw = dict(GSAM, minimize_fp=minimize_fp)
  config, model, state = _make(dev, kw)
  store = state["params"].store
  master0, shadow0 = store.master.clone(), store.shadow.clone()
  stages = {}
  grad_fn = train.make_grad_fn(model, config)
  grad_fn(state, 0, {"image": ref["image"].to(dev), "labels": ref["labels"].to(dev)}, stages=stages)
  torch.cuda.synchronize()
  n = store.trainable_count
  gc, gr, out = grad_fn.buffers().g_clean.double(), stages["g_robust"].double(), store.grad.double()
  # -- restored bit for bit (the whole buffers, the frozen tail and padding included)
  assert torch.equal(store.master, master0) and torch.equal(store.shadow.view(torch.int16), shadow0.view(torch.int16))
  # -- the reductions (bounds: _reduction_bound with the launch shapes of csrc/loss_optim.hip)
  sq_threads = 256 * min(2048, max(1, (n // 4 + 255) // 256))
  dot_threads = 256 * min(1024, (n + 1023) // 1024)
  sq_c, sq_r, dot, dot_abs = (gc * gc).sum().item(), (gr * gr).sum().item(), (gr * gc).sum().item(), (gr * gc).abs().sum().item()
  e_sq, e_dot = _reduction_bound(n, sq_threads, 4), _reduction_bound(n, dot_threads, 1)
  print(f"[gsam] reductions rel err: |gc|^2 {abs(stages['sq_clean'] - sq_c) / sq_c:.2e} |gr|^2 "
        f"{abs(stages['sq_robust'] - sq_r) / sq_r:.2e} (bound {e_sq:.2e}); dot {abs(stages['dot'] - dot) / dot_abs:.2e} "
        f"of sum|terms| (bound {e_dot:.2e})")
  assert abs(stages["sq_clean"] - sq_c) <= e_sq * sq_c and abs(stages["sq_robust"] - sq_r) <= e_sq * sq_r
  assert abs(stages["dot"] - dot) <= e_dot * dot_abs
  # -- the coefficients: the host's fp64 formulas on the product's reductions
  rho = ref["gsam"]["rho"]
  c = rho / (math.sqrt(stages["sq_clean"]) + 1e-12)
  if minimize_fp:
    a, b = 1 + 0.6 * stages["dot"] / stages["sq_robust"], -0.6
  else:
    a, b = 0.6, 1 - 0.6 * stages["dot"] / stages["sq_clean"]
  for name, want in (("c", c), ("a", a), ("b", b)):
    assert abs(stages[name] - want) <= 1e-12 * abs(want) + 1e-6 * abs(want) * (name == "c"), (name, stages[name], want)
  # -- y <- a_y y + a_x x on bv_sgemm_strided (gsam.axpby_): fl(fl(a_x) * x) + fl(fl(a_y) * y), rounded once more.
  # Roundings per term: the coefficient to fp32, the product; then the sum, whose magnitude is at most the sum of the
  # terms' magnitudes.  Each is at most EPS32 / 2 relative, so |error| <= 3 * EPS32 / 2 * (|a_x x| + |a_y y|) to first
  # order; 2 * EPS32 covers the second-order terms, and 2 * TINY32 a term flushed to zero below the normal range.
  terms = (stages["a"] * gr).abs() + (stages["b"] * gc).abs()
  err = (out - (stages["a"] * gr + stages["b"] * gc)).abs()
  print(f"[gsam] g_gsam max err / (eps32 * terms) = {(err / (EPS32 * terms + TINY32)).max().item():.3f} (bound 2)")
  assert (err <= 2 * EPS32 * terms + 2 * TINY32).all()
  m0, mp = master0[:n].double(), stages["master_perturbed"].double()
  terms = m0.abs() + (stages["c"] * gc).abs()
  err = (mp - (m0 + stages["c"] * gc)).abs()
  print(f"[gsam] perturbed master max err / (eps32 * terms) = {(err / (EPS32 * terms + TINY32)).max().item():.3f} (bound 2)")
  assert (err <= 2 * EPS32 * terms + 2 * TINY32).all()
  assert abs((mp - m0).norm().item() - rho) <= 1e-5 * rho            # a step of length sam_rho
  # -- the shadow the robust pass read: the bf16 rounding (nearest even) of the perturbed master
  assert torch.equal(stages["shadow_perturbed"].view(torch.int16),
                     stages["master_perturbed"].to(torch.bfloat16).view(torch.int16))
  assert not torch.equal(stages["shadow_perturbed"].view(torch.int16), shadow0[:n].view(torch.int16))


@pytest.mark.parametrize("n,rows", [(64, None), (63 * 64, None), (1024 * 16, 96), (512 * 128 * 64 + 1024, None)],
                         ids=["one_row", "under_a_tile", "row_ranges", "128_tiles_ragged"])
def test_axpby_every_kernel_path(dev, n, rows):
  """gsam.axpby_ at the sizes where bv_sgemm_strided takes another kernel (csrc/loss_optim.hip): fewer than 64 rows of
  64 (VALU kernel), 64-wide matrix-pipe tiles, 128-wide ones from 512 tiles on with a ragged last tile (what a
  B/32-sized buffer runs), and the loop over row ranges with a ragged last range.  Bound: as derived in
  test_vector_stage_on_the_products_own_gradients; a_y = 0 must not read y (NaN in, finite out)."""
  from big_vision_amd.trainers.proj.gsam import gsam
  g = torch.Generator().manual_seed(n)
  x, y = (torch.randn(n, generator=g) * 10 ** torch.randint(-6, 3, (n,), generator=g).float() for _ in range(2))
  eye = torch.eye(gsam.AXPBY_COLS, device=dev)
  a_x, a_y = -0.6, 1.3019
  out = gsam.axpby_(y.to(dev), a_y, x.to(dev), a_x, eye, **({} if rows is None else dict(rows=rows)))
  terms = (a_x * x.double()).abs() + (a_y * y.double()).abs()
  err = (out.cpu().double() - (a_x * x.double() + a_y * y.double())).abs()
  assert (err <= 2 * EPS32 * terms + 2 * TINY32).all(), (err / (EPS32 * terms + TINY32)).max()
  out = gsam.axpby_(torch.full((n,), float("nan"), device=dev), 0.0, x.to(dev), 1.0, eye)
  assert torch.equal(out.cpu(), x)


def test_gsam_gradient_end_to_end(dev, ref):
  """4. The full GSAM gradient at alpha = 0.6, sam_rho = 0.35 vs the oracle's, _parity's fixed bounds (cosine >= 0.999,
  rel-L2 <= 3e-2).  g_gsam = 1.30 g_robust - 0.6 g_clean subtracts vectors at cosine 0.79, so its floor is not a plain
  gradient's: the same oracle chain with bf16-rounded contraction operands, measured on the CPU on this case, stays
  at worst rel-L2 0.0125 / cosine 0.999922 per tensor (0.0108 / 0.999942 for the SAM case), inside the bounds; the
  test measures it again and holds it to them before it uses them."""
  import _parity
  state, _, _ = _grad_phase(dev, GSAM, ref["image"], ref["labels"])
  o = ref["gsam"]
  floor = _oracle_gsam(ref["params"], ref["image"], ref["labels"], GSAM, bf16=True)["g_gsam"]
  _, rows = _parity.compare_grads("gsam oracle with bf16 operands vs fp64 oracle", o["g_gsam"], floor)
  fl = {k: (rel, cos) for rel, cos, k, _, _, _ in rows}
  store = state["params"].store
  _parity.compare_grads("gsam gradient end to end", o["g_gsam"], _named(store, store.grad), floor=fl)


def test_full_steps(dev, ref):
  """5. update_fn: parameters move, the measurements are finite, a second step runs, the count advances by ONE."""
  from big_vision_amd.trainers.proj.gsam import train
  config, model, state = _make(dev, GSAM)
  store, opt = state["params"].store, state["opt"]
  update_fn = train.make_update_fn(model, config)
  batch = {"image": ref["image"].to(dev), "labels": ref["labels"].to(dev)}
  before = store.master.clone()
  state, meas = update_fn(state, 0, batch)
  torch.cuda.synchronize()
  train.check_finite(meas)
  assert set(meas) == {"training_loss", "l2_grads", "l2_params", "l2_updates"}
  assert opt.count == COUNT + 1
  assert meas["l2_updates"].item() > 0 and not torch.equal(store.master, before)
  assert abs(meas["training_loss"].item() - ref["gsam"]["loss"]) <= 1e-2 * abs(ref["gsam"]["loss"])
  gnorm = math.sqrt(_sqnorm(ref["gsam"]["g_gsam"]))
  assert abs(meas["l2_grads"].item() - gnorm) <= 2e-2 * gnorm           # opt.step() saw the GSAM gradient
  assert torch.equal(store.shadow[:store.trainable_count].view(torch.int16),
                     store.master[:store.trainable_count].to(torch.bfloat16).view(torch.int16))
  state, meas2 = update_fn(state, 0, batch)
  torch.cuda.synchronize()
  train.check_finite(meas2)
  assert opt.count == COUNT + 2
  assert meas2["training_loss"].item() != meas["training_loss"].item()
  logits, out = train.make_predict_fn(model, config)(state, batch)
  assert tuple(logits.shape) == (N, CLASSES) and "pre_logits" in out


def test_init_head_bias_and_fsdp_refusal(dev):
  from big_vision_amd.trainers.proj.gsam import train
  config = _cfg(GSAM)
  config.init_head_bias = -10.0
  _, model = train.get_model(config)
  state, _ = train.make_train_state(model, config, (N, RES, RES, 3), rng=0, total_steps=TOTAL)
  store = state["params"].store
  assert (store.leaf("head/bias") == -10.0).all() and (store.leaf("head/bias", "shadow").float() == -10.0).all()
  config.sharding_strategy = [(".*", "fsdp(axis='data', min_size_to_shard_mb=0)")]
  with pytest.raises(NotImplementedError, match="fsdp"):
    train.make_train_state(model, config, (N, RES, RES, 3), rng=0, total_steps=TOTAL)


# ------------------------------------------------------------------------------------------------------ two ranks --
def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _rank_step(dev, comm, image, labels):
  from big_vision_amd.trainers.proj.gsam import train
  config, model, state = _make(dev, GSAM, comm=comm)
  grad_fn = train.make_grad_fn(model, config, comm=comm)
  loss = grad_fn(state, 0, {"image": image.to(dev), "labels": labels.to(dev)})
  torch.cuda.synchronize()
  store = state["params"].store
  return loss.item(), store.grad.detach().cpu().numpy(), grad_fn.buffers().g_clean.detach().cpu().numpy()


def _worker(rank, world, port, out):
  sys.path.insert(0, ROOT)
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                    LOCAL_RANK="0")
  from big_vision_amd import dp
  torch.cuda.set_device(0)
  comm = dp.init_from_env(backend="gloo")
  image, labels = _batch(seed=7, n=world * N)
  out.put((rank,) + _rank_step(torch.device("cuda:0"), comm, image[rank * N:(rank + 1) * N], labels[rank * N:(rank + 1) * N]))
  comm.barrier()
  torch.distributed.destroy_process_group()


def test_two_ranks_average_their_own_gsam_gradients(dev):
  """6. Two rank processes on one GPU over gloo (as tests/test_dp_two_ranks_gpu.py), each with its own batch: each
  perturbs along its OWN local-mean gradient, and the gradient both end with is the mean of the two per-rank GSAM
  gradients, each computed by running that rank's batch alone on one rank.  A pass differs from its repetition by the
  order of fp32 sums at most (~1e-6 of a tensor's norm); 1e-3 leaves that two orders of room and is a tenth of the
  bf16 level, while the ranks' own gradients differ by order one."""
  import numpy as np
  import torch.multiprocessing as mp
  from big_vision_amd import dp
  world = 2
  image, labels = _batch(seed=7, n=world * N)
  alone = [_rank_step(dev, dp.Comm(), image[r * N:(r + 1) * N], labels[r * N:(r + 1) * N]) for r in range(world)]
  ctx = mp.get_context("spawn")
  out = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
  for p in procs:
    p.start()
  res = {}
  for _ in range(world):
    r = out.get(timeout=300)
    res[r[0]] = r[1:]
  for p in procs:
    p.join(60)
    assert p.exitcode == 0, f"rank process failed (exit {p.exitcode})"
  close = lambda x, y: np.linalg.norm(x.astype(np.float64) - y) <= 1e-3 * np.linalg.norm(y)
  assert np.array_equal(res[0][1], res[1][1]), "the ranks hold different gradients after the all-reduce"
  want = 0.5 * (alone[0][1].astype(np.float64) + alone[1][1])
  assert close(res[0][1], want), np.linalg.norm(res[0][1] - want) / np.linalg.norm(want)
  for r in range(world):
    assert close(res[r][2], alone[r][2].astype(np.float64)), f"rank {r} did not perturb along its own gradient"
    assert abs(res[r][0] - 0.5 * (alone[0][0] + alone[1][0])) <= 1e-6 * abs(alone[0][0]), "the loss is not the ranks' mean"
  apart = np.linalg.norm(alone[0][2].astype(np.float64) - alone[1][2]) / np.linalg.norm(alone[1][2])
  assert apart > 0.1 and not close(res[0][1], alone[0][1].astype(np.float64)), apart
