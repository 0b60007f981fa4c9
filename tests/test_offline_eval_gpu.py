"""Offline evaluation on the GPU: the mean and save evaluators and tools/eval_only.py end to end.

Shapes, the smallest at which this can go wrong: a ViT of width 128, depth 2, 2 heads, mlp_dim 256, patch 16 on 32 x 32
images, 10 classes, gap pooling; 3 batches of 8, the last with `_mask = [1, 1, 1, 0, 0, 0, 0, 0]` (19 real examples:
the padding matters); metric values from 1e-3 to 1e3 (the accumulation matters).

The bound of the mean.  tests/test_kernel_buckets_gpu.py::test_dot holds `bv_dot_f32` to |out - ref| <= 1e-6 |ref| +
1e-6 sqrt(count) against the fp64 sum of the same fp32 operands (DOT_LEGACY below restates its two constants; the
check itself is `_bounds.check` with that tolerance and no other model).  A metric's accumulator receives 3 launches
of 8 elements; the bound is applied ONCE, with count = 24, to their total S - less than the three per-launch
allowances add up to.  The count of real examples M = 19 is a sum of products 1 * 1, exact in fp32 and fp64, so the
yielded mean S / M errs by the error of S over M plus one fp64 rounding of the division (1.1e-16 relative, ten orders
below the bound and not granted separately): |mean - ref| <= 1e-6 |ref| + 1e-6 sqrt(24) / 19.  The reference is numpy,
fp64, on the host arrays after the same cast to fp32 - never the code under test.
"""
import json
import math

import numpy as np
import pytest
import torch

import _bounds as B

pytestmark = pytest.mark.gpu

N, RES, CLASSES, NBATCH = 8, 32, 10, 3
MODEL = dict(width=128, depth=2, num_heads=2, mlp_dim=256, patch_size=(16, 16), pool_type="gap")
LAST_MASK = [1, 1, 1, 0, 0, 0, 0, 0]
NSEEN = 2 * N + 3
DOT_LEGACY = (1e-6, 1e-6)     # test_kernel_buckets_gpu.py::test_dot: rtol, and atol per sqrt(count)


def _masks():
  return [torch.ones(N), torch.ones(N), torch.tensor(LAST_MASK, dtype=torch.float32)]


# ------------------------------------------------------------------- mean ----
def _metric_arrays():
  """Host arrays [3, 8] per metric, 1e-3 .. 1e3, every padding row finite and non-zero; the int metric 1 .. 1000."""
  rs = np.random.RandomState(11)
  a = np.logspace(-3, 3, NBATCH * N)[rs.permutation(NBATCH * N)].astype(np.float32).reshape(NBATCH, N)
  b = torch.from_numpy(np.logspace(-3, 3, NBATCH * N)[rs.permutation(NBATCH * N)].astype(np.float32)
                       .reshape(NBATCH, N)).to(torch.bfloat16)
  c = np.round(np.logspace(0, 3, NBATCH * N))[rs.permutation(NBATCH * N)].astype(np.int32).reshape(NBATCH, N)
  return {"a": torch.from_numpy(a), "b": b, "c": torch.from_numpy(c)}


@pytest.fixture(scope="module")
def metric_batches(dev):
  arrays = _metric_arrays()
  batches = [{**{k: v[i].to(dev) for k, v in arrays.items()}, "_mask": m.to(dev)} for i, m in enumerate(_masks())]
  mask = torch.stack(_masks()).double().numpy()
  # fp64 numpy on the host arrays after the evaluator's cast to fp32
  ref = {k: float((mask * v.to(torch.float32).numpy().astype(np.float64)).sum() / mask.sum()) for k, v in arrays.items()}
  assert mask.sum() == NSEEN
  return batches, ref


def _metrics_fn(train_state, batch):
  return {"a": batch["a"], "b": batch["b"], "c": batch["c"]}


def test_mean_against_numpy(dev, metric_batches):
  from big_vision_amd.evaluators import mean
  batches, ref = metric_batches
  assert batches[0]["a"].dtype == torch.float32 and batches[0]["b"].dtype == torch.bfloat16 \
      and batches[0]["c"].dtype == torch.int32
  got = list(mean.Evaluator(_metrics_fn, batches=batches).run(None))
  assert [k for k, _ in got] == ["a", "b", "c"]
  legacy = (DOT_LEGACY[0], DOT_LEGACY[1] * math.sqrt(NBATCH * N) / NSEEN)
  worst = 0.0
  for key, value in got:
    rel = abs(value - ref[key]) / abs(ref[key])
    worst = max(worst, rel)
    print(f"[offline eval] mean {key}: {value!r} vs fp64 {ref[key]!r}, rel err {rel:.3e}")
    B.check(torch.tensor([value], dtype=torch.float64), torch.tensor([ref[key]], dtype=torch.float64), None, legacy,
            name=f"mean {key}")
  print(f"[offline eval] mean: worst rel err {worst:.3e}")


def test_mean_launches_and_rank_split(dev, metric_batches, monkeypatch):
  from big_vision_amd import _lib, dp
  from big_vision_amd.evaluators import mean
  batches, _ = metric_batches

  class Names:
    def __init__(self):
      self.names = []

    def begin(self, name, args):
      self.names.append(name)

  fetched = []
  for method in ("cpu", "item", "tolist"):
    def counted(self, *a, _orig=getattr(torch.Tensor, method), _m=method, **kw):
      if self.is_cuda:
        fetched.append((_m, tuple(self.shape)))
      return _orig(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, method, counted)
  obs = Names()
  monkeypatch.setattr(_lib, "observer", obs)
  whole = list(mean.Evaluator(_metrics_fn, batches=batches).run(None))
  assert obs.names == ["bv_dot_f32"] * (4 * NBATCH)                  # 3 metrics + the mask count per batch, nothing else
  assert fetched == [("cpu", (4,))]                                  # one copy to the host per evaluation

  class TwoRanks(dp.Comm):
    """A one-rank Comm whose scalar all-reduce adds what the other "rank" accumulated."""
    def __init__(self, other=None):
      super().__init__()
      self.other, self.mine = other, None

    def all_reduce_scalars_(self, t):
      self.mine = t.clone()
      if self.other is not None:
        t.add_(self.other)
  rank1 = TwoRanks()
  list(mean.Evaluator(_metrics_fn, batches=batches[2:], comm=rank1).run(None))
  split = list(mean.Evaluator(_metrics_fn, batches=batches[:2], comm=TwoRanks(rank1.mine)).run(None))
  # (d1 + d2) + d3 either way: the same additions in the same order
  assert split == whole


# ------------------------------------------------------------ model, save ----
@pytest.fixture(scope="module")
def world(dev):
  """The tiny model with its zero-initialised head perturbed (every logit would be 0), the three image batches and
  the logits of calling the model directly."""
  from big_vision_amd.models import vit
  model = vit.Model(num_classes=CLASSES, **MODEL)
  store = model.make_store((N, RES, RES, 3))
  store.init_random(1)
  g = torch.Generator().manual_seed(3)
  for name in store.leaf_names():
    if name.startswith("head/"):
      leaf = store.leaf(name)
      leaf.add_((0.5 * torch.randn(leaf.shape, generator=g)).to(dev))
  store.mark_dirty(); store.refresh_shadow()
  params = store.tree()
  batches = []
  for mask in _masks():
    labels = torch.nn.functional.one_hot(torch.randint(0, CLASSES, (N,), generator=g), CLASSES).float()
    batches.append({"image": (torch.rand((N, RES, RES, 3), generator=g) * 2 - 1).to(dev), "labels": labels.to(dev),
                    "_mask": mask.to(dev)})
  predict_fn = lambda p, b: model.apply({"params": p}, b["image"], collect=False)
  logits = [predict_fn(params, b)[0].clone() for b in batches]
  assert len(set(torch.cat(logits).argmax(-1).tolist())) > 1            # the logits are not degenerate
  return dict(model=model, store=store, params=params, batches=batches, predict_fn=predict_fn, logits=logits)


def _real(tensors, batches):
  return torch.cat([t[b["_mask"] == 1] for t, b in zip(tensors, batches)]).cpu()


def test_save_round_trip(dev, world, tmp_path):
  from big_vision_amd import utils as u
  from big_vision_amd.evaluators import save
  batches = world["batches"]
  ev = save.Evaluator(world["predict_fn"], "{workdir}/pred-{step:09d}.npz", batches=batches, workdir=str(tmp_path))
  assert list(ev.run(world["params"])) == []
  res = u.load_checkpoint_np(str(tmp_path / "pred-000000000.npz"))
  flat = dict(u.tree_flatten_with_names(res)[0])
  assert {"inputs/image", "inputs/labels", "outputs/0", "outputs/1/logits", "outputs/1/head_input"} <= set(flat)
  assert "inputs/_mask" not in flat
  assert all(v.shape[0] == NSEEN for v in flat.values()), {k: v.shape for k, v in flat.items()}
  want = _real(world["logits"], batches)
  assert want.dtype == torch.float32 and np.array_equal(flat["outputs/0"], want.numpy())
  assert np.array_equal(flat["outputs/1/logits"], want.numpy())
  assert np.array_equal(flat["inputs/image"], _real([b["image"] for b in batches], batches).numpy())
  assert np.array_equal(flat["inputs/labels"], _real([b["labels"] for b in batches], batches).numpy())


# -------------------------------------------------------------- eval_only ----
def _config(model_init):
  from big_vision_amd.compat.ml_collections import ConfigDict
  c = ConfigDict()
  c.model_name, c.model, c.num_classes = "vit", dict(MODEL), CLASSES
  c.init_shapes = [(1, RES, RES, 3)]
  c.model_init = model_init
  c.eval_repeats = 2
  c.evals = {}
  c.evals.val = dict(type="classification", loss_name="softmax_xent", log_steps=1000)
  c.evals.avg = dict(type="mean", pred="scores", pred_kw=dict(temperature=2.0), log_steps=1000)
  c.evals.dump = dict(type="save", outfile="{workdir}/pred-{step:09d}.npz", pred_kw=dict(collect=False), log_steps=1000)
  return c


@pytest.fixture(scope="module")
def offline(dev, world, tmp_path_factory):
  """eval_only.run on the saved parameters and, in a second work directory, without `model_init`."""
  from big_vision_amd import utils as u
  from big_vision_amd.tools import eval_only
  root = tmp_path_factory.mktemp("offline")
  ckpt = str(root / "tiny.npz")
  u.save_params_npz(ckpt, dict(world["params"]))
  model, batches = world["model"], world["batches"]

  def scores(params, batch, temperature):
    logits = model.apply({"params": params}, batch["image"], collect=False)[0]
    return {"top": (logits / temperature).max(-1).values, "arg": logits.argmax(-1)}
  out = {"ckpt": ckpt}
  for tag, init in (("loaded", ckpt), ("fresh", "")):
    workdir = root / tag
    out[tag] = eval_only.run(_config(init), workdir=str(workdir), batches={k: batches for k in ("val", "avg", "dump")},
                             predict_fns={"scores": scores})
    out[tag + "_dir"] = workdir
  return out


def test_eval_only_end_to_end(dev, world, offline):
  from big_vision_amd import train
  from big_vision_amd import utils as u
  from big_vision_amd.evaluators import classification
  from big_vision_amd.models import vit
  res, workdir = offline["loaded"], offline["loaded_dir"]
  assert sorted(res) == [0, 1]
  assert set(res[0]) == {"num_params", "val/prec@1", "val/loss", "avg/top", "avg/arg"}
  assert res[0]["num_params"] == sum(v.numel() for _, v in u.tree_flatten_with_names(world["params"])[0])
  # the classification evaluator built by hand on the same loaded parameters: same kernels in the same order
  model = vit.Model(num_classes=CLASSES, **MODEL)
  store = model.make_store((1, RES, RES, 3))
  store.init_random(5)
  train.load_init(model, store, offline["ckpt"], dict(MODEL), {}, key="model_init")
  store.refresh_shadow()
  ev = classification.Evaluator(lambda p, b: model.apply({"params": p}, b["image"]), "softmax_xent",
                                batches=world["batches"])
  by_hand = dict(ev.run(store.tree()))
  print(f"[offline eval] eval_only {res[0]['val/prec@1']!r} {res[0]['val/loss']!r} by hand {by_hand}")
  assert res[0]["val/prec@1"] == by_hand["prec@1"] and res[0]["val/loss"] == by_hand["loss"]
  # the loaded parameters are the saved ones: the mean evaluator sees the logits of the model that was saved
  logits = _real(world["logits"], world["batches"]).double()
  assert res[0]["avg/arg"] == pytest.approx(float(logits.argmax(-1).double().mean()), rel=1e-6)
  assert res[0]["avg/top"] == pytest.approx(float((logits.float() / 2.0).max(-1).values.double().mean()), rel=1e-6)
  # eval_repeats lines with identical values
  lines = [json.loads(l) for l in (workdir / "big_vision_metrics.txt").read_text().splitlines()]
  assert [l.pop("step") for l in lines] == [0, 1] and lines[0].pop("num_params") == res[0]["num_params"]
  assert lines[0] == lines[1] == res[1]
  # the save evaluator wrote its file into the work directory, step 0 (no optimizer in the state)
  saved = u.load_checkpoint_np(str(workdir / "pred-000000000.npz"))
  assert np.array_equal(saved["outputs"]["0"], logits.float().numpy())


def test_model_init_is_honoured(dev, offline):
  loaded, fresh = offline["loaded"][0], offline["fresh"][0]
  assert loaded["num_params"] == fresh["num_params"]
  # zero-initialised head: every logit is 0 and the loss is log(10), to the rounding of the kernel's fp32 logf
  ulp = 2.0 ** -22                                                     # fp32 spacing at log(10) = 2.30
  print(f"[offline eval] fresh loss {fresh['val/loss']!r} vs log(10) {math.log(10.0)!r}, loaded {loaded['val/loss']!r}")
  assert abs(fresh["val/loss"] - math.log(CLASSES)) <= B.DEV_ULPS * ulp
  assert abs(loaded["val/loss"] - fresh["val/loss"]) > 1e-3
  assert (offline["fresh_dir"] / "pred-000000000.npz").exists()
