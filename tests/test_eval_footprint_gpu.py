"""Memory footprint of the entry point of libbveval (include/bveval.h), with the harness of tests/_footprint.py that
holds the other two libraries to their headers: the operands of ONE call are carved out of a guarded 0xFF arena; no
byte may change outside the declared write extents (logits, labels and mask stay bit-identical; `acc` is exactly 24
bytes), no output may depend on a byte outside an input extent, every output element is written, and the values meet
the bounds of tests/_eval_bounds.py.

One row per loss, optional-pointer pattern (mask, acc, row_loss, row_top1; at least one output) and C in {5, 257, 1003}
at n = 3 (4-byte loads, a wave per row), plus C = 1000 (16-byte loads), C = 1025 (a workgroup per row) and C = 4100
(both) with every pointer given.  tests/test_eval_abi_cpu.py holds this table to `_lib.PROTOTYPES_EVAL` without a GPU."""
import pytest
import torch

import _eval_bounds as B
import _footprint as F
from _footprint import Op

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32
N = 3
ROWS = []   # (entry point, case id, fn(dev))
LOSS_IDS = {"softmax_xent": 0, "sigmoid_xent": 1}
ACC_BASE = 0.5    # what _footprint.Arena fills an `inout` operand with


def stream():
  return torch.cuda.current_stream().cuda_stream


def call(name, *args):
  from big_vision_amd import _lib
  return _lib.call(name, *args)


def _row(loss, C, bits):
  """bits: 1 acc, 2 row_loss, 4 row_top1, 8 mask."""
  x = B.dyadic_logits(N, C, C)
  y = B.multihot_labels(x, C + 1) if loss == "sigmoid_xent" else B.onehot_labels(x, C + 1)
  m = torch.tensor([1.0, 0.0, 1.0])

  def make():
    ops = [Op("logits", F32, (N, C), fill=x), Op("labels", F32, (N, C), fill=y)]
    if bits & 8:
      ops.append(Op("mask", F32, (N,), fill=m))
    if bits & 1:
      ops.append(Op("acc", F64, (3,), "inout"))
    if bits & 2:
      ops.append(Op("row_loss", F32, (N,), "out"))
    if bits & 4:
      ops.append(Op("row_top1", I32, (N,), "out"))
    return ops

  def launch(ar):
    ptr = lambda name, bit: ar.ptr(name) if bits & bit else None
    call("bv_eval_classify", LOSS_IDS[loss], ar.ptr("logits"), ar.ptr("labels"), ptr("mask", 8), ptr("acc", 1),
         ptr("row_loss", 2), ptr("row_top1", 4), N, C, stream())

  def fn(dev):
    r = F.run("bv_eval_classify", f"{loss}-C{C}-mask{bits}", make, launch, dev)
    ref = B.classify64(loss, x, y, m if bits & 8 else None)
    bound = B.loss_bound(loss, x, y)
    if bits & 1:
      acc = r["acc"]
      assert acc.shape == (3,) and acc.element_size() * acc.numel() == 24
      assert acc[0].item() == ACC_BASE + ref["ncorrect"] and acc[2].item() == ACC_BASE + ref["nseen"]
      B.check_loss_sum(acc[1].item() - ACC_BASE, ref, bound, "acc[1]")
    if bits & 2:
      B.check(r["row_loss"], ref["loss"], bound, B.LEGACY_VALUE, "row_loss")
    if bits & 4:
      assert torch.equal(r["row_top1"].long(), ref["top1"])
  ROWS.append(("bv_eval_classify", f"{loss}-C{C}-mask{bits}", fn))


for _loss in LOSS_IDS:
  for _C in (5, 257, 1003):
    for _bits in range(1, 16):
      if _bits & 7:                     # at least one output
        _row(_loss, _C, _bits)
  for _C in (1000, 1025, 4100):
    _row(_loss, _C, 15)


@pytest.mark.parametrize("fn", [pytest.param(fn, id=f"{e}-{c}") for e, c, fn in ROWS])
def test_footprint(dev, fn):
  fn(dev)
