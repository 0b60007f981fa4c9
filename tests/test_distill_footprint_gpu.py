"""Memory footprint of every entry point of libbvdistill (include/bvdistill.h), with the harness of tests/_footprint.py
that holds libbvhip to its header: the operands of ONE call are carved out of a guarded 0xFF arena; no byte may change
outside the declared write extents, no output may depend on a byte outside an input extent, every output element is
written, and the values meet the bounds of tests/_distill_bounds.py.

One row per entry point, optional-pointer pattern and C in {5, 257, 1003} (scalar accesses; nothing about these rows is
a multiple of 4 or of the 256 lanes), plus C = 1000 (16-byte accesses) and C = 4100 (re-reading loops) with every
pointer given.  tests/test_distill_abi_cpu.py holds this table to `_lib.PROTOTYPES_DISTILL` without a GPU."""
import pytest
import torch

import _distill_bounds as D
import _footprint as F
from _footprint import Op

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
N = 3
ROWS = []   # (entry point, case id, fn(dev))
KIND_IDS = {"l2": 0, "euclidean": 1, "kl": 2, "hard": 3, "logsoftmax_euclidean": 4, "agree": 5}
KW = {"l2": {}, "euclidean": {}, "kl": dict(t=2.0), "hard": dict(ls=0.1), "logsoftmax_euclidean": {}, "agree": dict(k=5)}


def stream():
  return torch.cuda.current_stream().cuda_stream


def call(name, *args):
  from big_vision_amd import _lib
  return _lib.call(name, *args)


def _dist_row(kind, C, mask, accumulate=False):
  """mask: bit 0 per_row, bit 1 loss_sum, bit 2 dstudent."""
  s, T = (D.tied_logits(N, C, C) if kind in ("hard", "agree") else (D.logits(N, C, C), D.logits(N, C, C + 1)))
  kw = KW[kind]
  base = 0.01 * D.logits(N, C, C + 2, scale=1.0)

  def make():
    ops = [Op("student", F32, (N, C), fill=s), Op("teacher", F32, (N, C), fill=T)]
    if mask & 1:
      ops.append(Op("per_row", F32, (N,), "out"))
    if mask & 2:
      ops.append(Op("loss_sum", F64, (1,), "inout"))
    if mask & 4:
      ops.append(Op("dstudent", F32, (N, C), "inout", fill=base) if accumulate else Op("dstudent", F32, (N, C), "out"))
    return ops

  def launch(ar):
    ptr = lambda name, bit: ar.ptr(name) if mask & bit else None
    call("bv_distill_dist", KIND_IDS[kind], ar.ptr("student"), ar.ptr("teacher"), ptr("per_row", 1), ptr("loss_sum", 2),
         ptr("dstudent", 4), int(accumulate), N, C, 4 * N, kw.get("t", 1.0), kw.get("ls", 0.0), 1e-12, kw.get("k", 1),
         stream())

  def fn(dev):
    r = F.run("bv_distill_dist", f"{kind}-C{C}-mask{mask}", make, launch, dev)
    ref_v = D.dist64(kind, s, T, **kw)
    if kind == "agree":
      bv = torch.zeros(N, dtype=F64)
    else:
      bv, bg = D.bounds(kind, s, T, n_global=4 * N, **kw)
    if mask & 1:
      D.check(r["per_row"], ref_v, bv, D.LEGACY_VALUE, "per_row")
    if mask & 2:
      D.check(r["loss_sum"], (0.5 + ref_v.sum() / (4 * N)).reshape(1), (bv.sum() / (4 * N)).reshape(1), D.LEGACY_VALUE, "loss_sum")
    if mask & 4:
      _, ref_g = D.value_and_grad64(kind, s, T, n_global=4 * N, **kw)
      if accumulate:
        ref_g, bg = ref_g + base.double(), bg + D.U * base.abs().double()
      D.check(r["dstudent"], ref_g, bg, D.LEGACY_GRAD, "dstudent")
  ROWS.append(("bv_distill_dist", f"{kind}-C{C}-mask{mask}{'-acc' if accumulate else ''}", fn))


for _kind in KIND_IDS:
  for _C in (5, 257, 1003):
    for _mask in ((1, 2, 3) if _kind == "agree" else (7, 6, 5, 4, 3, 2, 1)):
      _dist_row(_kind, _C, _mask)
  for _C in (1000, 4100):
    _dist_row(_kind, _C, 3 if _kind == "agree" else 7)
  if _kind != "agree":
    for _C in (5, 1000, 4100):
      _dist_row(_kind, _C, 4, accumulate=True)


def _entropy_row(C, mask):
  x = D.logits(N, C, C + 7)

  def make():
    return ([Op("logits", F32, (N, C), fill=x)] + ([Op("per_row", F32, (N,), "out")] if mask & 1 else [])
            + ([Op("sum", F64, (1,), "inout")] if mask & 2 else []))

  def launch(ar):
    call("bv_distill_entropy", ar.ptr("logits"), ar.ptr("per_row") if mask & 1 else None,
         ar.ptr("sum") if mask & 2 else None, N, C, 4 * N, stream())

  def fn(dev):
    r = F.run("bv_distill_entropy", f"C{C}-mask{mask}", make, launch, dev)
    ref, b = D.entropy64(x), D.entropy_bound(x)
    if mask & 1:
      D.check(r["per_row"], ref, b, D.LEGACY_VALUE, "entropy")
    if mask & 2:
      D.check(r["sum"], (0.5 + ref.sum() / (4 * N)).reshape(1), (b.sum() / (4 * N)).reshape(1), D.LEGACY_VALUE, "entropy sum")
  ROWS.append(("bv_distill_entropy", f"C{C}-mask{mask}", fn))


def _softmax_row(C, accumulate):
  x = D.logits(N, C, C + 9)
  base = torch.softmax(D.logits(N, C, C + 10), -1) * 0.5

  def make():
    return [Op("logits", F32, (N, C), fill=x),
            Op("probs", F32, (N, C), "inout", fill=base) if accumulate else Op("probs", F32, (N, C), "out")]

  def launch(ar):
    call("bv_distill_softmax_acc", ar.ptr("logits"), ar.ptr("probs"), 0.5, int(accumulate), N, C, stream())

  def fn(dev):
    r = F.run("bv_distill_softmax_acc", f"C{C}-acc{int(accumulate)}", make, launch, dev)
    ref = 0.5 * torch.softmax(x.double(), -1) + (base.double() if accumulate else 0.0)
    D.check(r["probs"], ref, D.softmax_bound(x, 0.5) + D.U, D.LEGACY_GRAD, "probs")
  ROWS.append(("bv_distill_softmax_acc", f"C{C}-acc{int(accumulate)}", fn))


for _C in (5, 257, 1003, 1000, 4100):
  for _mask in (3, 2, 1):
    _entropy_row(_C, _mask)
  for _acc in (False, True):
    _softmax_row(_C, _acc)


@pytest.mark.parametrize("fn", [pytest.param(fn, id=f"{e}-{c}") for e, c, fn in ROWS])
def test_footprint(dev, fn):
  fn(dev)
