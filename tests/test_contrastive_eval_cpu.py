"""Host logic of the contrastive evaluator without a GPU: `ops.contrastive_eval`, the ONE helper that launches, is
replaced by an fp64 stand-in built on tests/_contrastive_bounds.py.  Checked here: the import path and `from_config`,
the `run` contract, that removing the padded examples equals the reference's masked formula (fp64, 1e-12), and the
collective choreography of `use_global_batch` over real `gloo` ranks (the pattern of tests/test_dp_gloo.py)."""
import importlib
import math
import os
import socket
import sys

import pytest
import torch

import _contrastive_bounds as CB
from big_vision_amd import ops
from big_vision_amd.compat.ml_collections import ConfigDict
from big_vision_amd.evaluators import common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, T = 16, 10.0


def standin(calls):
  def contrastive_eval(zimg, ztxt, t, acc_it, acc_ti, row_offset=0, cols=None, log_t=None, per_row=False):
    assert zimg.dtype == ztxt.dtype == torch.float32 and zimg.shape == ztxt.shape and not per_row
    assert acc_it.dtype == acc_ti.dtype == torch.float64 and acc_it.shape == acc_ti.shape == (3,)
    calls.append((zimg.shape[0], row_offset, None if cols is None else cols[0].shape[0], log_t is not None))
    if zimg.shape[0] == 0:
      return None
    t = float(torch.exp(log_t.double())) if log_t is not None else float(t)
    for acc, ref in zip((acc_it, acc_ti), CB.block64(zimg, ztxt, t, row_offset, cols)):
      acc += torch.tensor([ref["ncorrect"], ref["loss_sum"], ref["nseen"]], dtype=torch.float64)
    return None
  return contrastive_eval


@pytest.fixture()
def kernel(monkeypatch):
  calls = []
  monkeypatch.setattr(ops, "contrastive_eval", standin(calls))
  return calls


def _predict_fn(seen=None, log_t=False):
  """The "towers" are the identity: the batch carries the embeddings themselves."""
  def predict_fn(train_state, batch):
    assert set(batch) == {"image", "labels"}, set(batch)
    if seen is not None:
      seen.append(train_state)
    out = {"t": torch.tensor([T])}
    if log_t:
      out["t/parameter"] = torch.tensor([math.log(T)])
    return batch["image"], batch["labels"], out
  return predict_fn


def _batches(masks, seed=0, label_key="labels", wrong_every=3):
  out = []
  for i, mask in enumerate(masks):
    zi, zt = CB.planted(len(mask), E, seed + i, eps=0.5, wrong_every=wrong_every)
    out.append({"image": zi, label_key: zt, "_mask": torch.tensor(mask, dtype=torch.float32)})
  return out


def _reference(batches, t=T, label_key="labels"):
  """contrastive.py:84-99 over the literal masked formula, fp64."""
  c = l = n = 0.0
  for b in batches:
    cb, lb, nb = CB.eval_sums64(b["image"], b[label_key], t, b["_mask"])
    c, l, n = c + cb, l + lb, n + nb
  return c / n, l / n


MASKS = ([1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0], [1, 0, 1, 1, 0, 1], [0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0])


# ------------------------------------------------------------- import path ----
def test_import_path_and_from_config(kernel):
  """Fails without the feature: `big_vision.evaluators.proj.image_text.contrastive` does not resolve."""
  mod = importlib.import_module("big_vision.evaluators.proj.image_text.contrastive")
  from big_vision_amd.evaluators.proj.image_text import contrastive
  assert mod is contrastive
  c = ConfigDict()
  c.evals = {}
  c.evals.val = dict(type="proj.image_text.contrastive", use_global_batch=True, log_steps=7,
                     data=dict(name="coco_captions", split="val"), pp_fn="decode|resize(224)")
  predict_fn = _predict_fn()
  (name, ev, logsteps, prefix), = common.from_config(c, {"predict": predict_fn})
  assert (name, logsteps, prefix) == ("val", 7, "val/") and isinstance(ev, contrastive.Evaluator)
  assert ev.predict_fn is predict_fn and ev.use_global_batch is True and ev.label_key == "labels"
  assert ev.pipeline_kw == dict(data=dict(name="coco_captions", split="val"), pp_fn="decode|resize(224)",
                                batch_size=None)
  ev.batches = _batches(MASKS)
  got = dict(ev.run(None))
  want = _reference(ev.batches)
  assert got["ncorrect_minibatch"] == pytest.approx(want[0], abs=1e-12)
  assert got["loss"] == pytest.approx(want[1], abs=1e-12)


def test_trainers_expose_the_two_input_predict_fn():
  import inspect
  from big_vision_amd.trainers.proj.image_text import contrastive as tc, siglip
  assert tc.make_predict_fn is siglip.make_predict_fn
  assert list(inspect.signature(siglip.make_predict_fn).parameters) == ["model", "config"]
  from big_vision_amd import utils as u
  assert list(inspect.signature(u.bidirectional_contrastive_loss).parameters) == ["zimg", "ztxt", "t", "mask", "reduction"]


# ------------------------------------------------------------ run contract ----
class FakeComm:
  size, rank = 1, 0

  def __init__(self):
    self.calls = []

  def all_reduce_scalars_(self, t):
    assert t.dtype == torch.float64 and t.numel() == 6           # both accumulators, together
    self.calls.append(t)
    t *= 2          # as if a second host had seen the same examples: the ratios must not move


@pytest.mark.parametrize("use_global_batch", [True, False])
def test_run_contract(kernel, use_global_batch):
  from big_vision_amd.evaluators.proj.image_text import contrastive
  seen, comm = [], FakeComm()
  batches = _batches(MASKS, label_key="txt")
  ev = contrastive.Evaluator(_predict_fn(seen, log_t=True), use_global_batch, label_key="txt", batches=batches,
                             comm=comm, data={"name": "x"}, pp_fn="pp", batch_size=6, cache_final=True, cache_raw=False,
                             prefetch=1)
  assert ev.pipeline_kw == dict(data={"name": "x"}, pp_fn="pp", batch_size=6, cache_final=True, cache_raw=False,
                                prefetch=1)
  state = {"params": object()}
  got = list(ev.run(state))
  assert [k for k, _ in got] == ["ncorrect_minibatch", "loss"]
  want = _reference(batches, t=float(torch.exp(torch.tensor([math.log(T)]).double())), label_key="txt")
  assert got[0][1] == pytest.approx(want[0], abs=1e-12) and got[1][1] == pytest.approx(want[1], abs=1e-12)
  assert 0.0 < got[0][1] < 1.0                                   # the planted mistakes are in: not a constant
  # one call per batch that holds a real example, on the real rows only, the temperature as a device-side log;
  # the all-masked batch reached neither the towers nor the helper
  assert kernel == [(6, 0, None, True), (3, 0, None, True), (4, 0, None, True), (1, 0, None, True)]
  assert seen == [state] * 4
  assert len(comm.calls) == 1                                    # one reduction per evaluation, at the end
  assert all(set(b) == {"image", "txt", "_mask"} for b in batches)
  assert list(ev.run(state)) == got and len(kernel) == 8          # `batches` is re-iterated, not consumed


def test_one_copy_to_the_host_per_evaluation(kernel, monkeypatch):
  from big_vision_amd.evaluators.proj.image_text import contrastive
  reads = []
  real_zeros = torch.zeros

  class Spy(torch.Tensor):
    def cpu(self, *a, **kw):
      reads.append(self.numel() * self.element_size())
      return torch.Tensor.cpu(self.as_subclass(torch.Tensor), *a, **kw)

    def tolist(self):
      reads.append("tolist")
      return self.as_subclass(torch.Tensor).tolist()

    def item(self):
      reads.append("item")
      return self.as_subclass(torch.Tensor).item()

  def zeros(*a, **kw):
    z = real_zeros(*a, **kw)
    return z.as_subclass(Spy) if kw.get("dtype") == torch.float64 else z
  monkeypatch.setattr(contrastive.torch, "zeros", zeros)
  ev = contrastive.Evaluator(_predict_fn(), False, batches=_batches(MASKS))
  got = dict(ev.run(None))
  monkeypatch.setattr(contrastive.torch, "zeros", real_zeros)
  assert reads == [48], reads
  assert got["loss"] == pytest.approx(_reference(ev.batches)[1], abs=1e-12)


def test_empty_batches_raise_and_all_padding_is_nan(kernel):
  from big_vision_amd.evaluators.proj.image_text import contrastive
  with pytest.raises(ValueError, match="`batches` is empty"):
    list(contrastive.Evaluator(_predict_fn(), True).run(None))
  with pytest.raises(ValueError, match="`batches` is empty"):
    list(contrastive.Evaluator(_predict_fn(), False, batches=[], comm=FakeComm()).run(None))
  seen = []
  got = dict(contrastive.Evaluator(_predict_fn(seen), False, batches=_batches([[0, 0, 0]])).run(None))
  assert kernel == [] and seen == []                             # launched nothing
  assert math.isnan(got["loss"]) and math.isnan(got["ncorrect_minibatch"])     # 0 / 0, as in the reference


# ---------------------------------------- removed rows == the masked formula ----
@pytest.mark.parametrize("mask", [[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0], [1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 0, 1, 1, 1],
                                  [0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]],
                         ids=["none", "prefix", "interior", "first", "single", "single-first", "v=0"])
@pytest.mark.parametrize("t", [1.0, 10.0, 100.0])
def test_removed_rows_equal_the_masked_formula(mask, t):
  zi, zt = CB.planted(len(mask), E, seed=11, eps=0.7, wrong_every=2)
  want = CB.eval_sums64(zi, zt, t, mask)            # the literal formula: -inf in padded rows and columns
  got = CB.removed64(zi, zt, t, mask)               # the padded examples removed, no mask
  assert got[2] == want[2] == sum(mask)
  assert got[0] == want[0]
  assert abs(got[1] - want[1]) <= 1e-12
  # the per-example values too: the real ones agree, the padded ones are exactly zero
  l, nc, _ = CB.masked64(zi, zt, t, mask)
  keep = torch.tensor(mask) != 0
  assert bool((l[~keep] == 0).all())
  if keep.any():
    lr, ncr, _ = CB.masked64(zi[keep], zt[keep], t)
    assert (l[keep] - lr).abs().max() <= 1e-12 and torch.equal(nc[keep], ncr)


def test_the_standin_restates_the_same_thing():
  """block64 (what the stand-in, and on the GPU the kernels, compute) against masked64 on an unmasked batch."""
  zi, zt = CB.planted(9, E, seed=3, eps=0.7, wrong_every=2)
  it, ti = CB.block64(zi, zt, T)
  l, nc, _ = CB.masked64(zi, zt, T)
  assert it["ncorrect"] == float(nc.sum()) and 0 < it["ncorrect"] < 9
  assert (0.5 * (it["loss"] + ti["loss"]) - l).abs().max() <= 1e-12


# --------------------------------------------------------------- multi-rank ----
B_RANK, NB = 5, 3


def _global_data(world):
  """NB global batches of world * B_RANK examples; padding in the middle of the gathered batch, one rank all padding
  in the last batch, one batch without padding."""
  out = []
  for j in range(NB):
    zi, zt = CB.planted(world * B_RANK, E, seed=100 + j, eps=0.6, wrong_every=3)
    mask = torch.ones(world * B_RANK)
    if j == 1:
      mask[B_RANK - 2:B_RANK] = 0                   # the tail of rank 0: the offsets of every later rank move
      mask[-1] = 0
    if j == 2:
      mask[B_RANK:2 * B_RANK] = 0                   # rank 1 holds nothing real
      mask[0] = 0
    out.append((zi, zt, mask))
  return out


def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _worker(rank, world, port, out):
  sys.path.insert(0, ROOT)
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                    LOCAL_RANK=str(rank))
  from big_vision_amd import dp
  from big_vision_amd.evaluators.proj.image_text import contrastive
  comm = dp.init_from_env(backend="gloo")
  assert comm.size == world and comm.rank == rank
  calls = []
  ops.contrastive_eval = standin(calls)
  rows = slice(rank * B_RANK, (rank + 1) * B_RANK)
  batches = [{"image": zi[rows], "labels": zt[rows], "_mask": m[rows]} for zi, zt, m in _global_data(world)]
  res = {}
  for use_global in (True, False):
    del calls[:]
    res[use_global] = (dict(contrastive.Evaluator(_predict_fn(), use_global, batches=batches, comm=comm).run(None)),
                       list(calls))
  comm.barrier()
  out.put((rank, res))
  import torch.distributed as dist
  dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_row_blocks_add_up_to_the_global_batch(world):
  import torch.multiprocessing as mp
  ctx = mp.get_context("spawn")
  out = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
  for p in procs:
    p.start()
  res = dict(out.get(timeout=240) for _ in range(world))
  for p in procs:
    p.join(60)
    assert p.exitcode == 0, f"rank process failed (exit {p.exitcode})"
  data = _global_data(world)
  # use_global_batch=True: the single-process result on the concatenated batch (contrastive.py:54-63)
  c = l = n = 0.0
  for zi, zt, m in data:
    cb, lb, nb = CB.eval_sums64(zi, zt, T, m)
    c, l, n = c + cb, l + lb, n + nb
  assert 0 < c < n
  # use_global_batch=False: every rank's batch is its own universe; the sums are added up
  cl = ll = nl = 0.0
  for zi, zt, m in data:
    for r in range(world):
      rows = slice(r * B_RANK, (r + 1) * B_RANK)
      cb, lb, nb = CB.eval_sums64(zi[rows], zt[rows], T, m[rows])
      cl, ll, nl = cl + cb, ll + lb, nl + nb
  assert nl == n and abs(ll / nl - l / n) > 1e-3                 # the two settings are different questions
  for r in range(world):
    got, calls = res[r][True]
    assert got["ncorrect_minibatch"] == pytest.approx(c / n, abs=1e-12), r
    assert got["loss"] == pytest.approx(l / n, abs=1e-12), r
    # this rank's rows against the gathered real columns, its identity block at its offset among the real examples
    want_calls = []
    for _, _, m in data:
      v, off = int(m[r * B_RANK:(r + 1) * B_RANK].sum()), int(m[:r * B_RANK].sum())
      want_calls.append((v, off, int(m.sum()), False))
    assert calls == want_calls, (r, calls, want_calls)
    got, calls = res[r][False]
    assert got["ncorrect_minibatch"] == pytest.approx(cl / nl, abs=1e-12), r
    assert got["loss"] == pytest.approx(ll / nl, abs=1e-12), r
    assert all(cols is None and off == 0 for _, off, cols, _ in calls)


def test_one_rank_makes_the_two_settings_identical(kernel):
  from big_vision_amd import dp
  from big_vision_amd.evaluators.proj.image_text import contrastive
  batches = _batches(MASKS)
  runs = [list(contrastive.Evaluator(_predict_fn(), g, batches=batches, comm=c).run(None))
          for g in (True, False) for c in (None, dp.Comm())]
  assert all(r == runs[0] for r in runs)
