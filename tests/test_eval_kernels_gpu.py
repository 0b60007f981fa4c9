"""libbveval.so through its C ABI (include/bveval.h) vs the fp64 restatement of tests/_eval_bounds.py.  Loss values
are held to max(legacy tolerance of test_kernels_gpu.py::test_softmax_xent, per-element rounding model); the counts
(ncorrect, nseen) and the argmax columns must be EXACTLY equal.

Shapes: n in {1, 7, 64}; C in {1, 2, 5, 257, 1000, 1003, 1024, 1025, 4099, 4100, 21843}: fewer classes than lanes,
lane tails, both sides of the wave-per-row / workgroup-per-row switch at C = 1024, C % 4 == 0 (16-byte loads: 1000
and 1024 on the wave side, 4100 on the workgroup side) and not (4-byte loads), and a row far beyond 4096 columns.

KERNELS names, for every kernel instantiation in the library, the test below that launches it;
tests/test_eval_abi_cpu.py compares the list with the library's symbols.
"""
import pytest
import torch

import _eval_bounds as B

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NS = (1, 7, 64)
CS = (1, 2, 5, 257, 1000, 1003, 1024, 1025, 4099, 4100, 21843)
LOSS_IDS = {"softmax_xent": 0, "sigmoid_xent": 1}

# eval_classify_kernel<KIND, VEC, WG>: loss, 16-byte loads, workgroup per row
KERNELS = {f"_ZN12_GLOBAL__N_120eval_classify_kernelILi{k}ELi{v}ELi{w}EEEvNS_8EvalArgsE": f"test_classify_matches_fp64[{name}]"
           for name, k in LOSS_IDS.items() for v in (0, 1) for w in (0, 1)}

WORST = {}


def _note(name, ratios):
  w = WORST.setdefault(name, [0.0, 0.0])
  w[0], w[1] = max(w[0], ratios[0]), max(w[1], ratios[1])


def _labels(loss, logits, seed):
  return B.multihot_labels(logits, seed) if loss == "sigmoid_xent" else B.onehot_labels(logits, seed)


def _run(loss, logits, labels, mask, dev):
  from big_vision_amd import ops
  acc, rows, top1 = ops.eval_classify(loss, logits.to(dev), labels.to(dev), None if mask is None else mask.to(dev),
                                      per_row=True)
  return acc.cpu(), rows.cpu(), top1.cpu()


def _check(loss, logits, labels, mask, dev, tag, finite_rows=None):
  """One call against classify64: losses within the model, counts and argmax exact.  finite_rows: the rows whose loss
  is finite in the reference (default: all); the others must be NaN in both."""
  acc, rows, top1 = _run(loss, logits, labels, mask, dev)
  ref = B.classify64(loss, logits, labels, mask)
  bound = B.loss_bound(loss, logits, labels)
  name = f"{loss} {tag}"
  assert torch.equal(top1.long(), ref["top1"]), (name, top1.tolist()[:8], ref["top1"].tolist()[:8])
  assert acc[0].item() == ref["ncorrect"] and acc[2].item() == ref["nseen"], (name, acc.tolist(), ref["ncorrect"], ref["nseen"])
  if finite_rows is None:
    _note(f"{loss} row", B.check(rows, ref["loss"], bound, B.LEGACY_VALUE, name + " row_loss"))
    _note(f"{loss} sum", B.check_loss_sum(acc[1].item(), ref, bound, name + " acc[1]"))
  else:
    keep = torch.zeros(rows.shape[0], dtype=torch.bool)
    keep[finite_rows] = True
    B.check(rows[keep], ref["loss"][keep], bound[keep], B.LEGACY_VALUE, name + " row_loss")
    assert torch.isnan(rows[~keep]).all() and torch.isnan(ref["loss"][~keep]).all(), name
    assert torch.isnan(acc[1]), name                  # classification.py:45: the NaN loss reaches the sum
  return acc, rows, top1, ref


@pytest.mark.parametrize("loss", list(LOSS_IDS))
def test_classify_matches_fp64(dev, loss):
  """Both losses at every (n, C), with a 0/1 mask, on dyadic logits (multiples of 1/8: long rows are full of exact
  ties) and, at n = 7, on Gaussian logits of deviation 3."""
  for C in CS:
    for n in NS:
      x = B.dyadic_logits(n, C, 10 * n + C)
      _check(loss, x, _labels(loss, x, n + C), B.mask01(n, n + 2 * C), dev, f"n={n} C={C}")
    g = torch.Generator().manual_seed(C)
    x = (torch.randn((7, C), generator=g) * 3).float()
    _check(loss, x, _labels(loss, x, C + 1), None, dev, f"gauss C={C}")
  print({k: [f"{v:.3g}" for v in w] for k, w in WORST.items() if k.startswith(loss)})


@pytest.mark.parametrize("C", [5, 257, 1000, 1025, 4100])
def test_planted_ties_and_nans(dev, C):
  """The row maximum at two or three columns with the label at only the first (even rows: correct) or only the last
  (odd rows: wrong): row_top1 is the first column and ncorrect follows it.  Then a row with one NaN and a row with two:
  the first NaN wins, whatever the finite maximum is."""
  n = 8
  g = torch.Generator().manual_seed(C)
  x = B.dyadic_logits(n, C, C, lo=-32, hi=24)
  y = torch.zeros((n, C))
  first = []
  for r in range(n):
    cols = torch.randperm(C, generator=g)[: 2 + r % 2].sort().values
    x[r, cols] = 3.5
    first.append(int(cols[0]))
    y[r, cols[0] if r % 2 == 0 else cols[-1]] = 1.0
  for loss in LOSS_IDS:
    acc, _, top1, _ = _check(loss, x, y, None, dev, f"ties C={C}")
    assert top1.tolist() == first and acc[0].item() == n // 2 and acc[2].item() == n
  # NaNs: row 1 has one (not at the finite maximum), row 2 has two; the labels sit at the expected columns
  nan_cols = {1: [C // 2], 2: [C // 3, C - 1]}
  for r, cols in nan_cols.items():
    x[r, cols] = float("nan")
    y[r] = 0.0
    y[r, cols[0]] = 1.0
  for loss in LOSS_IDS:
    acc, _, top1, _ = _check(loss, x, y, None, dev, f"nans C={C}", finite_rows=[0, 3, 4, 5, 6, 7])
    assert top1[1].item() == C // 2 and top1[2].item() == C // 3
    assert acc[0].item() == n // 2 + 1            # rows 0, 2 (now through its NaN), 4, 6 and row 1


def test_mask_semantics(dev):
  """mask = 0 rows, all-zero label rows under mask = 1 (dropped through max y), mask = NULL, multi-hot rows."""
  for C in (257, 1025):
    n = 8
    x = B.dyadic_logits(n, C, 3 * C)
    for loss in LOSS_IDS:
      y = _labels(loss, x, C)
      y[2] = 0.0
      y[5] = 0.0
      mask = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
      acc, _, _, ref = _check(loss, x, y, mask, dev, f"mask C={C}")
      assert acc[2].item() == 4.0 == ref["nseen"]          # rows 0, 3, 6, 7
      acc, _, _, _ = _check(loss, x, y, None, dev, f"mask NULL C={C}")
      assert acc[2].item() == 6.0                          # NULL = ones; the two all-zero rows still drop out
      if loss == "sigmoid_xent":
        assert y.sum(-1).max() > 1                         # multi-hot rows took part


def test_extreme_logits(dev):
  """|logits| up to 1e3: rows where all but one exponential underflow, a constant row at +1e3, a spread row.  The
  online log-sum-exp must stay finite and inside the model."""
  for C in (1000, 4099):
    g = torch.Generator().manual_seed(C)
    x = (torch.randn((4, C), generator=g) * 300).clamp(-1e3, 1e3).float()
    x[1] = -1e3
    x[1, C // 2] = 1e3
    x[2] = 1e3
    x[3] = torch.randn((C,), generator=g)
    x[3, 7] = 1e3
    for loss in LOSS_IDS:
      _, rows, _, _ = _check(loss, x, _labels(loss, x, C), None, dev, f"extreme C={C}")
      assert torch.isfinite(rows).all()


def test_acc_accumulates_over_calls(dev):
  from big_vision_amd import ops
  n, C = 64, 1003
  x = B.dyadic_logits(n, C, 1)
  for loss in LOSS_IDS:
    y, m = _labels(loss, x, 2).to(dev), B.mask01(n, 3).to(dev)
    xd = x.to(dev)
    whole = ops.eval_classify(loss, xd, y, m)
    acc = ops.eval_classify(loss, xd[: n // 2].contiguous(), y[: n // 2].contiguous(), m[: n // 2].contiguous())
    out = ops.eval_classify(loss, xd[n // 2:].contiguous(), y[n // 2:].contiguous(), m[n // 2:].contiguous(), acc=acc)
    assert out is acc
    whole, acc = whole.cpu(), acc.cpu()
    assert acc[0].item() == whole[0].item() and acc[2].item() == whole[2].item() and whole[2].item() > 0
    assert abs(acc[1].item() - whole[1].item()) <= 1e-12 * abs(whole[1].item())


def test_every_optional_pointer_null_in_turn(dev):
  """mask / acc / row_loss / row_top1: any may be NULL and the others do not change; all three outputs NULL is an
  invalid call."""
  from big_vision_amd import _lib
  n, C = 7, 257
  x = B.dyadic_logits(n, C, 1)
  y = B.onehot_labels(x, 2)
  m = B.mask01(n, 3)
  xd, yd, md = x.to(dev), y.to(dev), m.to(dev)
  p = lambda t: None if t is None else t.data_ptr()
  stream = torch.cuda.current_stream().cuda_stream
  for loss, kind in LOSS_IDS.items():
    for use_mask in (True, False):
      ref = B.classify64(loss, x, y, m if use_mask else None)
      bound = B.loss_bound(loss, x, y)
      full = None
      for bits in (7, 6, 5, 3, 4, 2, 1):
        acc = torch.zeros(3, device=dev, dtype=F64) if bits & 1 else None
        rows = torch.full((n,), float("nan"), device=dev) if bits & 2 else None
        top1 = torch.full((n,), -1, device=dev, dtype=torch.int32) if bits & 4 else None
        _lib.call("bv_eval_classify", kind, p(xd), p(yd), p(md) if use_mask else None, p(acc), p(rows), p(top1), n, C, stream)
        torch.cuda.synchronize()
        if full is None:
          full = (acc, rows, top1)
          B.check(rows, ref["loss"], bound, B.LEGACY_VALUE, "row_loss")
          B.check_loss_sum(acc[1].item(), ref, bound, "acc[1]")
          assert torch.equal(top1.cpu().long(), ref["top1"])
          assert acc[0].item() == ref["ncorrect"] and acc[2].item() == ref["nseen"]
          continue
        assert rows is None or torch.equal(rows, full[1]), bits
        assert top1 is None or torch.equal(top1, full[2]), bits
        if acc is not None:
          assert acc[0].item() == full[0][0].item() and acc[2].item() == full[0][2].item()
          assert abs(acc[1].item() - full[0][1].item()) <= 1e-12 * abs(full[0][1].item())
  lib = _lib.handle("eval")
  assert lib.bv_eval_classify(0, p(xd), p(yd), p(md), None, None, None, n, C, None) == -1     # BVE_ERR_INVALID_ARG
  assert b"bv_eval_classify" in lib.bv_eval_last_error() and b"all NULL" in lib.bv_eval_last_error()


@pytest.mark.parametrize("C", [1000, 1003, 4100])
def test_views_off_the_16_byte_grid_take_the_4_byte_path(dev, C):
  """Both matrices one float past a 16-byte boundary: C % 4 == 0 no longer selects the 16-byte loads.  The lane-to-column
  assignment differs between the two paths, so the values are held to the model, not to each other; an odd C as well.
  Nothing around the views changes."""
  from big_vision_amd import ops
  n = 7
  x = B.dyadic_logits(n, C, C)
  for loss in LOSS_IDS:
    y = _labels(loss, x, C + 1)
    buf = torch.zeros(2 * n * C + 16, device=dev)
    at = -(-(1 + n * C) // 4) * 4 + 1                    # the next offset past the logits that is 1 mod 4
    xo, yo = buf[1:1 + n * C].view(n, C), buf[at:at + n * C].view(n, C)
    xo.copy_(x); yo.copy_(y)
    assert xo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == 4 and xo.is_contiguous()
    before = buf.clone()
    acc, rows, top1 = ops.eval_classify(loss, xo, yo, per_row=True)
    ref = B.classify64(loss, x, y)
    bound = B.loss_bound(loss, x, y)
    B.check(rows, ref["loss"], bound, B.LEGACY_VALUE, f"{loss} off-grid row_loss C={C}")
    B.check_loss_sum(acc[1].item(), ref, bound, f"{loss} off-grid acc[1] C={C}")
    assert torch.equal(top1.cpu().long(), ref["top1"])
    assert acc[0].item() == ref["ncorrect"] and acc[2].item() == ref["nseen"]
    assert torch.equal(buf, before)
    _check(loss, x, y, None, dev, f"aligned C={C}")


def test_invalid_arguments(dev):
  """Every BVE_ERR_INVALID_ARG of include/bveval.h, with the entry point's name in the message."""
  from big_vision_amd import _lib, ops
  lib = _lib.handle("eval")
  x = B.dyadic_logits(2, 8, 1).to(dev)
  y = B.onehot_labels(x.cpu(), 2).to(dev)
  acc = torch.zeros(3, device=dev, dtype=F64)
  X, Y, A = x.data_ptr(), y.data_ptr(), acc.data_ptr()
  bad = {"n <= 0": (0, X, Y, None, A, None, None, 0, 8, None), "n < 0": (0, X, Y, None, A, None, None, -1, 8, None),
         "C <= 0": (0, X, Y, None, A, None, None, 2, 0, None), "unknown kind": (2, X, Y, None, A, None, None, 2, 8, None),
         "negative kind": (-1, X, Y, None, A, None, None, 2, 8, None),
         "NULL logits": (0, None, Y, None, A, None, None, 2, 8, None), "NULL labels": (1, X, None, None, A, None, None, 2, 8, None),
         "all outputs NULL": (1, X, Y, None, None, None, None, 2, 8, None)}
  for what, args in bad.items():
    assert lib.bv_eval_classify(*args) == -1, what
    assert lib.bv_eval_last_error().decode().startswith("bv_eval_classify: "), what
    with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: "):
      _lib.call("bv_eval_classify", *args)
  torch.cuda.synchronize()
  assert acc.cpu().tolist() == [0.0, 0.0, 0.0]
  with pytest.raises(RuntimeError, match="GPU"):
    ops.eval_classify("softmax_xent", torch.zeros(2, 8), torch.zeros(2, 8))
  with pytest.raises(AttributeError, match="nope"):
    ops.eval_classify("nope", x, y)
