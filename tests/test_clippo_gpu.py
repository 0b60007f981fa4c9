"""CLIPPO (`models.proj.clippo.one_tower`) on the GPU against an fp64 composition of the oracle.

Expected values never come from the product: oracle/bv_oracle.py's ViT forward is applied in fp64 to the images and to
the rendered captions WITH THE SAME parameter tensors, followed by the z / (|z| + 1e-8) normalisation and the oracle's
softmax (CLIP) loss; torch autograd sums the two uses of every weight.  Bounds are the standing ones:
  embeddings (unit norm)      max-abs <= 2e-2     (tests/test_siglip_step_gpu.py: the two_towers cases, `tol_z`)
  loss                        rel     <= 1e-2     (same file)
  parameter gradients         per tensor cosine >= 0.999, rel-L2 <= 3e-2, small-tensor branch (tests/_parity.py)
A shared weight's gradient is the sum of two bf16-operand products of the same noise level: the same relative bound.

Tower: width 64, depth 2, 2 heads, mlp 128, patch 16, 48 x 48 images (9 tokens, 10 with the cls token); pool_type map /
gap / tok; n = 4 and n = 5 pairs (odd: the split of the 2n batch is not tile aligned).
"""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RES, EMB = 48, 32
TOL_Z, TOL_LOSS = 2e-2, 1e-2
CASES = [(pool, n) for pool in ("map", "gap", "tok") for n in (4, 5)]
_CACHE = {}


def _tower(pool):
  return dict(width=64, depth=2, num_heads=2, mlp_dim=128, patch_size=(16, 16), pool_type=pool, head_zeroinit=False)


def _config(**kw):
  from big_vision_amd.compat.ml_collections import ConfigDict
  c = ConfigDict()
  c.lr, c.wd = 1e-3, 1e-2
  c.schedule = dict(decay_type="cosine", warmup_steps=2)
  c.optax_name = "scale_by_adam"
  c.grad_clip_norm = 1.0
  c.total_steps = 10
  c.loss_fn = "softmax"
  for k, v in kw.items():
    c[k] = v
  return c


def _batch(n, seed=1):
  """(photos, rendered captions): two independent U(-1, 1) image batches - the tower cannot tell them apart."""
  import bv_oracle as O
  return O.synthetic_batch(seed, n, RES, 8, 100)[0], O.synthetic_batch(seed + 100, n, RES, 8, 100)[0]


def _make_state(dev, pool, n, comm=None, **cfg_kw):
  from big_vision_amd.models.proj.clippo import one_tower
  from big_vision_amd.trainers.proj.image_text import contrastive
  model = one_tower.Model(image=_tower(pool), out_dim=EMB, temperature_init=10.0)
  config = _config(**cfg_kw)
  shape = (n, RES, RES, 3)
  kw = {} if comm is None else {"comm": comm}
  state, _ = contrastive.make_train_state(model, config, shape, shape, rng=0, total_steps=config.total_steps, **kw)
  store = state["params"].store
  g = torch.Generator().manual_seed(7)
  for name in store.leaf_names():        # break the symmetric inits (zero biases, unit scales, zero cls)
    if name.endswith(("bias", "scale", "cls")):
      leaf = store.leaf(name)
      leaf.add_((0.05 * torch.randn(leaf.shape, generator=g)).to(dev))
  store.mark_dirty()
  store.refresh_shadow()
  return model, config, state


def oracle_forward(params64, image, text, pool):
  """The fp64 composition: one parameter tree, two applications of the oracle's ViT."""
  import bv_oracle as O
  zs = []
  for x in (image, text):
    z, _ = O.vit_forward(params64["img"], x.double(), num_classes=EMB, **_tower(pool))
    zs.append(z / (torch.linalg.norm(z, dim=1, keepdim=True) + 1e-8))
  return zs[0], zs[1], torch.exp(params64["t"])


def _case(dev, pool, n):
  """Model, state (before any step), batch and the fp64 reference of one (pool, n) case; computed once, never changed."""
  key = (pool, n)
  if key not in _CACHE:
    import bv_oracle as O
    from big_vision_amd import utils as u
    model, config, state = _make_state(dev, pool, n)
    image, text = _batch(n)
    flat = u.tree_flatten_with_names(state["params"])[0]
    params64 = O.recover_tree([(k, v.detach().cpu().double().clone().requires_grad_(True)) for k, v in flat])
    zi, zt, t = oracle_forward(params64, image, text, pool)
    loss = O.softmax_loss_per_device(zi, zt, [zi], [zt], 0, t)
    loss.backward()
    gref = {k: v.grad for k, v in O.tree_flatten_with_names(params64) if v.grad is not None}
    _CACHE[key] = dict(model=model, config=config, state=state, image=image.to(dev), text=text.to(dev),
                       zi=zi.detach(), zt=zt.detach(), t=t.detach(), loss=loss.detach(), gref=gref)
  return _CACHE[key]


def _grads(store):
  from big_vision_amd import utils as u
  return {k: v.detach().cpu().double().clone() for k, v in u.tree_flatten_with_names(store.tree("grad"))[0]}


@pytest.mark.parametrize("pool,n", CASES)
def test_forward_matches_the_fp64_composition(dev, pool, n):
  c = _case(dev, pool, n)
  zimg, ztxt, out = c["model"].apply({"params": c["state"]["params"]}, c["image"], c["text"])
  ei = (zimg.cpu().double() - c["zi"]).abs().max().item()
  et = (ztxt.cpu().double() - c["zt"]).abs().max().item()
  et_ = abs(out["t"].item() - c["t"].item())
  print(f"[clippo] {pool} n={n}: max-abs zimg {ei:.3e} ztxt {et:.3e} (<= {TOL_Z}), t err {et_:.2e}")
  assert zimg.shape == ztxt.shape == (n, EMB)
  assert ei <= TOL_Z and et <= TOL_Z
  assert et_ <= 1e-5 * c["t"].item()                      # exp of one fp32 number
  assert abs(out["t/parameter"].item() - math.log(10.0)) < 1e-6
  # the out dict: every tower key under both prefixes, the normalisation, t; no bias
  from big_vision_amd.models import vit
  tower_keys = set(vit.Model(num_classes=EMB, **_tower(pool)).apply(
      {"params": c["state"]["params"]["img"]}, c["image"])[1])
  want = {f"{p}/{k}" for p in ("img", "txt") for k in tower_keys | {"norm", "normalized"}} | {"t", "t/parameter"}
  assert set(out) == want, set(out) ^ want
  assert out["img/norm"].shape == out["txt/norm"].shape == (n, 1)
  assert out["img/encoded"].shape == out["txt/encoded"].shape
  assert torch.equal(out["img/normalized"], zimg) and torch.equal(out["txt/normalized"], ztxt)
  # views of the two halves of ONE batch: the text half starts where the image half ends
  assert ztxt.data_ptr() == zimg.data_ptr() + zimg.numel() * 4


@pytest.mark.parametrize("pool,n", CASES)
def test_one_pass_over_2n_rows_equals_two_passes(dev, pool, n):
  """apply(image, text) against apply(image, None) and apply(None, text) of the product itself: within the embedding
  bound, not bit for bit (the GEMM tiling depends on M)."""
  c = _case(dev, pool, n)
  p = {"params": c["state"]["params"]}
  zimg, ztxt, _ = c["model"].apply(p, c["image"], c["text"], collect=False)
  zi1, none_t, out_i = c["model"].apply(p, c["image"], None, collect=False)
  none_i, zt1, out_t = c["model"].apply(p, None, c["text"], collect=False)
  assert none_t is None and none_i is None
  assert not any(k.startswith("txt/") for k in out_i) and not any(k.startswith("img/") for k in out_t)
  assert {"t", "t/parameter", "img/norm", "img/normalized"} <= set(out_i)
  ei, et = (zimg - zi1).abs().max().item(), (ztxt - zt1).abs().max().item()
  print(f"[clippo] {pool} n={n}: 2n pass vs two n passes max-abs {ei:.3e} / {et:.3e}")
  assert ei <= TOL_Z and et <= TOL_Z
  assert (zi1.cpu().double() - c["zi"]).abs().max().item() <= TOL_Z
  assert (zt1.cpu().double() - c["zt"]).abs().max().item() <= TOL_Z


@pytest.mark.parametrize("pool,n", CASES)
def test_training_step_matches_the_fp64_composition(dev, pool, n):
  """One step through contrastive.make_update_fn, loss_fn="softmax": loss and every per-tensor gradient (shared weights:
  the sum over both uses) against autograd on the fp64 composition, standing bounds of tests/_parity.py."""
  import _parity
  from big_vision_amd.trainers.proj.image_text import contrastive
  c = _case(dev, pool, n)
  model, config, state = _make_state(dev, pool, n)         # a fresh state: the cached one stays at its initial weights
  update_fn = contrastive.make_update_fn(model, config)
  loss_fwd, meas_fwd = contrastive.loss_fn(model, state["params"], c["image"], c["text"], config)
  state, meas = update_fn(state, None, {"image": c["image"], "labels": c["text"]})
  loss, ref = meas["training_loss"].item(), c["loss"].item()
  print(f"[clippo] {pool} n={n}: loss {loss:.6f} (forward only {loss_fwd.item():.6f}) vs fp64 {ref:.6f}")
  assert abs(loss - ref) <= TOL_LOSS * abs(ref)
  assert abs(loss_fwd.item() - ref) <= TOL_LOSS * abs(ref)
  assert {"t", "t/parameter", "train/nimg", "train/ntxt", "train/i2t_acc", "train/t2i_loss"} <= set(meas)
  store = state["params"].store
  gours = _grads(store)
  assert set(gours) == set(c["gref"]) and "b" not in gours and not any(k.startswith("txt/") for k in gours)
  gnorm, _ = _parity.compare_grads(f"clippo {pool} n={n} softmax", c["gref"], gours)
  assert abs(meas["l2_grads"].item() - gnorm) <= 2e-2 * gnorm, (meas["l2_grads"].item(), gnorm)


@pytest.mark.parametrize("pool,n", CASES)
def test_zero_text_cotangent_equals_the_image_only_backward(dev, pool, n):
  """Weight sharing through the model's backward: the 2n pass with the text half's cotangent forced to zero (None, and
  explicit zeros) accumulates what the n-row pass on the images alone does.  Same arithmetic on the image rows - zero
  rows add exact zeros - under another GEMM tiling: the bound test_microbatched_step_equals_full_batch holds two
  batchings of one step to (2e-3 of the tensor's norm, tensors below 1e-3 of the global norm measured against that)."""
  c = _case(dev, pool, n)
  model, store = c["model"], c["state"]["params"].store
  store.want_grads = True
  shape = tuple(c["image"].shape)
  ex = model.executor(store, "", shape, shape)
  dz = torch.randn((n, EMB), generator=torch.Generator().manual_seed(11)).to(dev)

  def run(image, text, dzimg, dztxt):
    store.zero_grad()
    _, _, _, ctx = ex.fwd(image, text, save=True)
    ex.bwd(ctx, dzimg, dztxt)
    torch.cuda.synchronize()
    return _grads(store)

  alone = run(c["image"], None, dz, None)
  gn = math.sqrt(sum((v ** 2).sum().item() for v in alone.values()))
  assert gn > 0
  for name, g in (("None", run(c["image"], c["text"], dz, None)),
                  ("zeros", run(c["image"], c["text"], dz, torch.zeros_like(dz)))):
    worst = max((v - g[k]).norm().item() / max(v.norm().item(), 1e-3 * gn) for k, v in alone.items())
    print(f"[clippo] {pool} n={n}: dztxt = {name}: worst relative difference to the image-only backward {worst:.3e}")
    for k, v in alone.items():
      assert (v - g[k]).norm().item() <= 2e-3 * max(v.norm().item(), 1e-3 * gn), (name, k)
  # and the other half: both cotangents given = the sum of the two one-sided backwards (linearity of the backward)
  both = run(c["image"], c["text"], dz, -0.5 * dz)
  txt = run(c["image"], c["text"], None, -0.5 * dz)
  for k, v in both.items():
    assert (v - alone[k] - txt[k]).norm().item() <= 4e-3 * max(v.norm().item(), 1e-3 * gn), k
  store.zero_grad()


def test_sigmoid_losses_are_refused(dev):
  from big_vision_amd.trainers.proj.image_text import contrastive
  c = _case(dev, "map", 4)
  for name in ("sigmoid", "chunked_sigmoid"):
    with pytest.raises(ValueError, match="need the model's bias parameter"):
      contrastive.make_update_fn(c["model"], _config(loss_fn=name))


# ------------------------------------------------------------------ evaluators ----
N_EVAL, BS, MARGIN = 10, 4, 1e-4


def _exp_delta(t):
  """What the device-side temperature adds to a logit's error (tests/test_contrastive_eval_gpu.py)."""
  import _eval_bounds as B
  return (B.EXP0 + B.EXPX * abs(math.log(t)) + 1.0) * B.U * abs(t)


def test_contrastive_evaluator_on_rendered_captions(dev):
  """10 pairs at batch size 4 (the last batch: two real rows, two padded and masked) through
  evaluators.proj.image_text.contrastive on the CLIPPO predict function, the "labels" an fp32 [b, H, W, 3] batch;
  against the masked fp64 formula on the product's own embeddings gathered batch by batch."""
  import _contrastive_bounds as CB
  from big_vision_amd.evaluators.proj.image_text import contrastive as ev_mod
  from big_vision_amd.trainers.proj.image_text import contrastive
  c = _case(dev, "map", 4)
  predict_fn = contrastive.make_predict_fn(c["model"], c["config"])
  image, text = _batch(N_EVAL, seed=5)
  batches = []
  for s in range(0, N_EVAL, BS):
    valid = min(BS, N_EVAL - s)
    pad = lambda x: torch.cat([x[s:s + valid], x[s + valid - 1:s + valid].expand(BS - valid, *x.shape[1:])])
    batches.append({"image": pad(image).to(dev), "labels": pad(text).to(dev),
                    "_mask": torch.tensor([1.0] * valid + [0.0] * (BS - valid))})
  assert [int(b["_mask"].sum()) for b in batches] == [4, 4, 2] and batches[0]["labels"].dtype == torch.float32
  got = dict(ev_mod.Evaluator(predict_fn, True, batches=batches).run(c["state"]))

  cs = ls = ns = bound = 0.0
  margin = float("inf")
  for b in batches:
    zimg, ztxt, out = predict_fn(c["state"], {"image": b["image"], "labels": b["labels"]})
    t = float(torch.exp(out["t/parameter"].double().cpu().reshape(-1)[0]))
    zi, zt = zimg.cpu().double().numpy(), ztxt.cpu().double().numpy()
    keep = b["_mask"].numpy() != 0
    logits = t * zi[keep] @ zt[keep].T                          # numpy fp64 on the real rows and columns
    top = np.sort(logits, axis=1)[:, -2:]
    margin = min(margin, float((top[:, 1] - top[:, 0]).min()))
    lse = lambda x: np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1)
    d = np.diagonal(logits)
    ls += float((0.5 * ((lse(logits) - d) + (lse(logits.T) - d))).sum())
    cs += float((logits.argmax(1) == np.arange(keep.sum())).sum())
    ns += float(keep.sum())
    refs = CB.block64(zimg.cpu()[torch.from_numpy(keep)], ztxt.cpu()[torch.from_numpy(keep)], t)
    for ref in refs:
      ref["delta"] = ref["delta"] + _exp_delta(t)
    bound += 0.5 * (CB.direction_bound(refs[0]) + CB.direction_bound(refs[1]))
  print(f"[clippo] contrastive evaluator: loss {got['loss']:.7f} vs numpy fp64 {ls / ns:.7f} (bound of the sum "
        f"{bound:.3e}), ncorrect {got['ncorrect_minibatch'] * ns:.0f} vs {cs:.0f}, smallest top-2 margin {margin:.3e}")
  assert ns == N_EVAL
  assert margin > MARGIN, f"smallest top-2 logit margin {margin:.3e}: pick another seed"
  assert got["ncorrect_minibatch"] == cs / ns
  assert abs(got["loss"] * ns - ls) <= bound


def test_discriminative_classifier_on_rendered_prompts(dev):
  """Zero-shot classification with image-shaped prompts: 3 classes x 2 rendered prompts (two batches of 4, the second
  padded) and 10 images at batch size 4, against numpy fp64 on the product's own embeddings."""
  from big_vision_amd.evaluators.proj.image_text import discriminative_classifier as dc
  from big_vision_amd.trainers.proj.image_text import contrastive
  c = _case(dev, "map", 4)
  predict_fn = contrastive.make_predict_fn(c["model"], c["config"])
  images, prompts = _batch(N_EVAL, seed=9)
  prompts = prompts[:6]
  prompt_labels = np.array([0, 1, 2, 0, 1, 2])
  labels = np.arange(N_EVAL) % 3
  ev = dc.Evaluator(predict_fn, datasets={"toy": dict(images=images, labels=labels, prompts=prompts,
                                                       prompt_labels=prompt_labels)}, batch_size=BS, device=dev)
  got = ev.evaluate(c["state"], "toy", return_embeddings=True)

  def gather(name, data):       # the product's own embeddings, batch by batch, padded like the evaluator pads
    out = []
    for s in range(0, len(data), BS):
      chunk = data[s:s + BS]
      valid = chunk.shape[0]
      if valid < BS:
        chunk = torch.cat([chunk, chunk[-1:].expand(BS - valid, *chunk.shape[1:])])
      zimg, ztxt, _ = predict_fn(c["state"], {name: chunk.to(dev)})
      out.append((zimg if name == "image" else ztxt)[:valid].cpu().double().numpy())
    return np.concatenate(out)

  ztxt, zimg = gather("labels", prompts), gather("image", images)
  assert np.array_equal(got["texts"]["embedding"].astype(np.float64), ztxt)
  assert np.array_equal(got["images"]["embedding"].astype(np.float64), zimg)
  avg = np.stack([ztxt[prompt_labels == k].mean(0) for k in range(3)])
  avg = avg / (1e-8 + np.linalg.norm(avg, axis=1, keepdims=True))
  logits = zimg @ avg.T
  top = np.sort(logits, axis=1)[:, -2:]
  margin = float((top[:, 1] - top[:, 0]).min())
  correct = int((logits.argmax(1) == labels).sum())
  print(f"[clippo] zero-shot: correct {got['correct']} vs numpy fp64 {correct} of {N_EVAL}, smallest top-2 margin "
        f"{margin:.3e}")
  assert margin > MARGIN, f"smallest top-2 logit margin {margin:.3e}: pick another seed"
  assert (got["correct"], got["count"]) == (correct, N_EVAL) and got["accuracy"] == correct / N_EVAL
  assert ev.run(c["state"]) == [("toy_accuracy", correct / N_EVAL)]


# ------------------------------------------------------------------ two ranks ----
def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _step(dev, comm, image, text):
  from big_vision_amd.trainers.proj.image_text import contrastive
  from big_vision_amd import utils as u
  model, config, state = _make_state(dev, "map", image.shape[0], comm=comm)
  fn = contrastive.make_update_fn(model, config, comm=comm)
  state, meas = fn(state, None, {"image": image, "labels": text})
  torch.cuda.synchronize()
  store = state["params"].store
  params = {k: v.detach().cpu().double() for k, v in u.tree_flatten_with_names(store.full_tree())[0]}
  return meas["training_loss"].item(), meas["l2_grads"].item(), _grads(store), params


def _worker(rank, world, port, out):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, "oracle"))
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                    LOCAL_RANK="0")
  from big_vision_amd import dp
  torch.cuda.set_device(0)
  dev = torch.device("cuda:0")
  comm = dp.init_from_env(backend="gloo")
  image, text = _batch(8)
  n = 8 // world
  loss, gn, grads, params = _step(dev, comm, image[rank * n:(rank + 1) * n].to(dev), text[rank * n:(rank + 1) * n].to(dev))
  digest = {k: (v.sum().item(), v.abs().sum().item()) for k, v in params.items()}
  out.put((rank, loss, gn, {k: v.numpy() for k, v in grads.items()} if rank == 0 else None, digest))
  comm.barrier()
  torch.distributed.destroy_process_group()


def test_two_ranks_match_the_single_process_step(dev):
  """Two rank processes share the GPU over gloo (tests/test_dp_two_ranks_gpu.py, "w2", replicated parameters): all-gather
  of both embeddings, reduce-scatter of their gradients, every block's gradient handed to the overlapped all-reduce
  after the ONE 2n backward - against the single-process step on the 8 pairs, the bounds of that file."""
  import torch.multiprocessing as mp
  from big_vision_amd import dp
  image, text = _batch(8)
  loss1, gn1, g1, _ = _step(dev, dp.Comm(), image.to(dev), text.to(dev))
  ctx = mp.get_context("spawn")
  out = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
  for p in procs:
    p.start()
  res = {}
  for _ in range(2):
    r = out.get(timeout=300)
    res[r[0]] = r[1:]
  for p in procs:
    p.join(60)
    assert p.exitcode == 0, f"rank process failed (exit {p.exitcode})"
  loss2, gn2, g2, digest = res[0]
  assert abs(res[0][0] - res[1][0]) <= 1e-6 * abs(loss1), "ranks disagree on the global loss"
  assert digest == res[1][3], "replicated parameters diverged between the ranks after the update"
  assert abs(loss2 - loss1) <= 1e-4 * abs(loss1), (loss1, loss2)
  assert abs(gn2 - gn1) <= 2e-2 * gn1, (gn1, gn2)
  gnorm = math.sqrt(sum((v ** 2).sum().item() for v in g1.values()))
  for k, v in g1.items():
    assert (v - torch.from_numpy(g2[k])).norm().item() <= 2e-2 * max(v.norm().item(), 1e-2 * gnorm), k
