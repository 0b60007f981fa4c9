"""libbvdistill.so through its C ABI (include/bvdistill.h) vs the fp64 restatement of tests/_distill_bounds.py, held
to max(legacy tolerance of test_kernels_gpu.py::test_softmax_xent, per-element rounding model) - see that module.
tests/test_distill_bounds_cpu.py proves on the CPU that these bounds reject the plausible slips.

Shapes: n in {1, 3, 7}; C in {1, 5, 255, 256, 257, 1000, 1003, 4100}: fewer classes than lanes, around one pass of the
256 lanes, C % 4 == 0 (16-byte path: 256, 1000) and not (scalar path), and one row longer than the 4096-column
register cache (re-reading path); n_global in {n, 4 n}; t in {0.5, 1, 2}; ls in {0, 0.1}; k in {1, 5}.

KERNELS names, for every kernel instantiation in the library, the test below that launches it;
tests/test_distill_abi_cpu.py compares the list with the library's symbols.
"""
import pytest
import torch

import _distill_bounds as D

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NS = (1, 3, 7)
CS = (1, 5, 255, 256, 257, 1000, 1003, 4100)
MODES = {0: "16-byte accesses, row in registers (C in {256, 1000})", 1: "scalar accesses, row in registers",
         2: "re-reading loops (C = 4100)"}
KIND_IDS = {"l2": 0, "euclidean": 1, "kl": 2, "hard": 3, "logsoftmax_euclidean": 4, "agree": 5}

KERNELS = {}
for _kind, _i in KIND_IDS.items():
  for _m in MODES:
    KERNELS[f"_ZN12_GLOBAL__N_119distill_dist_kernelILi{_i}ELi{_m}EEEvNS_8DistArgsE"] = (
        "test_agree_matches_the_rank_count" if _kind == "agree" else f"test_dist_matches_fp64[{_kind}]")
for _m in MODES:
  KERNELS[f"_ZN12_GLOBAL__N_122distill_entropy_kernelILi{_m}EEEvPKfPfPdii"] = "test_entropy_matches_fp64"
  KERNELS[f"_ZN12_GLOBAL__N_126distill_softmax_acc_kernelILi{_m}EEEvPKfPffii"] = "test_softmax_acc_matches_fp64"

WORST = {}


def _note(name, ratios):
  w = WORST.setdefault(name, [0.0, 0.0])
  w[0], w[1] = max(w[0], ratios[0]), max(w[1], ratios[1])


def _inputs(kind, n, C, seed):
  if kind in ("hard", "agree"):
    return D.tied_logits(n, C, seed)
  return D.logits(n, C, seed), D.logits(n, C, seed + 100)


def _run(kind, s, T, dev, n_global=None, **kw):
  from big_vision_amd import ops
  acc = torch.zeros(1, device=dev, dtype=F64)
  rows, g = ops.distill_dist(kind, s.to(dev), T.to(dev), loss_sum=acc, per_row=True, want_grad=True, n_global=n_global,
                             **kw)
  return rows, g, acc


def _check(kind, s, T, dev, tag, n_global=None, **kw):
  n = s.shape[0]
  rows, g, acc = _run(kind, s, T, dev, n_global=n_global, **kw)
  ref_v, ref_g = D.value_and_grad64(kind, s, T, n_global=n_global, **kw)
  bv, bg = D.bounds(kind, s, T, n_global=n_global, **kw)
  name = f"{kind} {tag}"
  _note(f"{kind} value", D.check(rows, ref_v, bv, D.LEGACY_VALUE, name + " per_row"))
  _note(f"{kind} derivative", D.check(g, ref_g, bg, D.LEGACY_GRAD, name + " dstudent"))
  ng = n_global or n
  _note(f"{kind} loss", D.check(acc, (ref_v.sum() / ng).reshape(1), (bv.sum() / ng).reshape(1), D.LEGACY_VALUE, name + " loss_sum"))


PARAMS = {"l2": [{}], "euclidean": [{}], "kl": [dict(t=0.5), dict(t=1.0), dict(t=2.0)],
          "hard": [dict(ls=0.0), dict(ls=0.1)], "logsoftmax_euclidean": [{}]}


@pytest.mark.parametrize("kind", list(PARAMS))
def test_dist_matches_fp64(dev, kind):
  """Every kind at every (n, C, n_global) and parameter value: per-row values, the loss share and the derivative.
  Worst measured error / tolerance (error / rounding model alone) over all shapes, MI355X, printed with -s:
    kind                   value            loss share       derivative
    l2                     0.012  (0.14)    0.0098 (0.12)    0.0015 (0.83)
    euclidean              0.0088 (0.16)    0.0084 (0.16)    0.0022 (0.30)
    kl                     0.036  (0.10)    0.036  (0.067)   0.049  (0.56)
    hard                   0.039  (0.16)    0.026  (0.11)    0.0047 (0.43)
    logsoftmax_euclidean   0.011  (0.085)   0.011  (0.075)   0.118  (0.30)
  i.e. no element uses more than 12 % of its tolerance, and the rounding model alone would hold everywhere."""
  for C in CS:
    for n in NS:
      for kw in PARAMS[kind]:
        if C == 1 and kw.get("ls"):
          continue                          # ls / (C - 1): rejected, see test_invalid_arguments
        s, T = _inputs(kind, n, C, 10 * n + C)
        for ng in (None, 4 * n):
          _check(kind, s, T, dev, f"n={n} C={C} n_global={ng} {kw}", n_global=ng, **kw)
  print({k: [f"{x:.3g}" for x in v] for k, v in WORST.items() if k.startswith(kind)})


def test_near_zero_distances_need_the_model(dev):
  """The square roots near eps and KL between nearly equal rows: student = teacher (value sqrt(eps), derivative 0)
  and student = teacher + 1e-3 noise, where the legacy tolerance alone would be the wrong yardstick."""
  for C in (257, 1000):
    T = D.logits(3, C, 5)
    for noise in (0.0, 1e-3):
      s = T + noise * D.logits(3, C, 6, scale=1.0)
      for kind, kw in (("euclidean", {}), ("logsoftmax_euclidean", {}), ("kl", dict(t=2.0)), ("l2", {})):
        _check(kind, s, T, dev, f"near-zero noise={noise} C={C}", **kw)


def test_extreme_logits(dev):
  """|logits| up to 1e3: most teacher probabilities underflow below the 1e-8 clip; row 1's value is the clip's own
  contribution (~1.3e-5).  kl at t = 1 and 2, hard, and the entropy of such rows."""
  from big_vision_amd import ops
  s, T = D.extreme_logits()
  for kind, kw in (("kl", dict(t=1.0)), ("kl", dict(t=2.0)), ("hard", dict(ls=0.1)), ("logsoftmax_euclidean", {})):
    _check(kind, s, T, dev, "extreme", **kw)
  h = ops.distill_entropy(T.to(dev), per_row=True)
  D.check(h, D.entropy64(T), D.entropy_bound(T), D.LEGACY_VALUE, "entropy extreme")


@pytest.mark.parametrize("k", [1, 5])
def test_agree_matches_the_rank_count(dev, k):
  """Planted exact ties (multiples of 1/8): fp32 and fp64 agree on every argmax and rank, no row is excluded, and the
  result must be exactly 0 or 1."""
  from big_vision_amd import ops
  seen = set()
  for C in CS:
    for n in NS:
      s, T = D.tied_logits(n, C, 3 * n + C)
      rows, _ = ops.distill_dist("agree", s.to(dev), T.to(dev), per_row=True, k=k)
      ref = D.dist64("agree", s, T, k=k)
      assert torch.equal(rows.cpu().double(), ref), (C, n, k)
      acc = torch.zeros(1, device=dev, dtype=F64)
      ops.distill_dist("agree", s.to(dev), T.to(dev), loss_sum=acc, k=k, n_global=4 * n)
      assert abs(acc.item() - ref.sum().item() / (4 * n)) <= 1e-12
      seen |= set(ref.tolist())
  assert seen == {0.0, 1.0}


def test_accumulate_over_two_teachers_equals_the_sum_of_two_calls(dev):
  from big_vision_amd import ops
  for C in (257, 1000, 4100):
    s, T1, T2 = (D.logits(3, C, i).to(dev) for i in (1, 2, 3))
    for kind, kw in (("kl", dict(t=2.0)), ("euclidean", {}), ("hard", dict(ls=0.1))):
      _, g1 = ops.distill_dist(kind, s, T1, want_grad=True, **kw)
      _, g2 = ops.distill_dist(kind, s, T2, want_grad=True, **kw)
      acc = torch.zeros(1, device=dev, dtype=F64)
      _, g = ops.distill_dist(kind, s, T1, want_grad=True, loss_sum=acc, **kw)
      _, g = ops.distill_dist(kind, s, T2, dstudent=g, loss_sum=acc, **kw)
      # one fp32 add (or one fused multiply-add) per element on top of the first call's bits
      assert ((g - (g1 + g2)).abs() <= 2 * D.U * (g1.abs() + g2.abs())).all(), (kind, C)
      ref = sum(D.dist64(kind, s.cpu(), T.cpu(), **kw).mean() for T in (T1, T2))
      assert abs(acc.item() - ref.item()) <= 1e-5 * abs(ref.item()) + 1e-6


def test_every_optional_pointer_null_in_turn(dev):
  """per_row / loss_sum / dstudent: any subset may be NULL and the others do not change (bit-identical)."""
  from big_vision_amd import _lib, ops
  n, C = 3, 257
  s, T = D.logits(n, C, 1).to(dev), D.logits(n, C, 2).to(dev)
  p = lambda t: None if t is None else t.data_ptr()
  stream = torch.cuda.current_stream().cuda_stream
  full = None
  for mask in (7, 6, 5, 3, 4, 2, 1, 0):
    rows = torch.full((n,), float("nan"), device=dev) if mask & 1 else None
    acc = torch.zeros(1, device=dev, dtype=F64) if mask & 2 else None
    g = torch.full((n, C), float("nan"), device=dev) if mask & 4 else None
    _lib.call("bv_distill_dist", KIND_IDS["kl"], p(s), p(T), p(rows), p(acc), p(g), 0, n, C, n, 2.0, 0.0, 1e-12, 1, stream)
    torch.cuda.synchronize()
    if full is None:
      full = (rows, acc, g)
      continue
    for got, want in zip((rows, g), (full[0], full[2])):
      assert got is None or torch.equal(got, want), mask
    assert acc is None or abs(acc.item() - full[1].item()) <= 1e-12 * abs(full[1].item())
  for mask in (3, 2, 1):
    rows = torch.full((n,), float("nan"), device=dev) if mask & 1 else None
    acc = torch.zeros(1, device=dev, dtype=F64) if mask & 2 else None
    _lib.call("bv_distill_entropy", p(s), p(rows), p(acc), n, C, n, stream)
    ref = D.entropy64(s.cpu())
    if rows is not None:
      D.check(rows, ref, D.entropy_bound(s.cpu()), D.LEGACY_VALUE, "entropy rows")
    if acc is not None:
      assert abs(acc.item() - ref.mean().item()) <= 1e-5 * ref.mean().item()


def test_unaligned_rows_take_the_scalar_path(dev):
  """C % 4 == 0 but a base address that is 4 bytes off a 16-byte boundary: the same values as the aligned call."""
  from big_vision_amd import ops
  n, C = 3, 256
  s, T = D.logits(n, C, 1), D.logits(n, C, 2)
  buf = torch.zeros(2 * n * C + 2, device=dev)
  so, To = buf[1:1 + n * C].view(n, C), buf[n * C + 1:2 * n * C + 1].view(n, C)
  so.copy_(s); To.copy_(T)
  assert so.data_ptr() % 16 == 4
  rows, g = ops.distill_dist("kl", so, To, per_row=True, want_grad=True, t=2.0)
  ref_v, ref_g = D.value_and_grad64("kl", s, T, t=2.0)
  bv, bg = D.bounds("kl", s, T, t=2.0)
  D.check(rows, ref_v, bv, D.LEGACY_VALUE, "unaligned value")
  D.check(g, ref_g, bg, D.LEGACY_GRAD, "unaligned derivative")
  assert float(buf[0]) == 0.0 and float(buf[-1]) == 0.0


def test_entropy_matches_fp64(dev):
  from big_vision_amd import ops
  for C in CS:
    for n in NS:
      x = D.logits(n, C, n + C)
      ref = D.entropy64(x)
      for ng in (n, 4 * n):
        acc = torch.zeros(1, device=dev, dtype=F64)
        rows = ops.distill_entropy(x.to(dev), sum=acc, per_row=True, n_global=ng)
        b = D.entropy_bound(x)
        _note("entropy", D.check(rows, ref, b, D.LEGACY_VALUE, f"entropy n={n} C={C}"))
        D.check(acc, (ref.sum() / ng).reshape(1), (b.sum() / ng).reshape(1), D.LEGACY_VALUE, f"entropy sum n={n} C={C}")
  print(WORST.get("entropy"))


def test_softmax_acc_matches_fp64(dev):
  """probs = w softmax(a), then probs += w softmax(b): the teacher ensemble; rows sum to 1."""
  from big_vision_amd import ops
  for C in CS:
    for n in NS:
      a, b = D.logits(n, C, n + C), D.logits(n, C, n + C + 50)
      pa, pb = torch.softmax(a.double(), -1), torch.softmax(b.double(), -1)
      probs = ops.distill_softmax_acc(a.to(dev), 0.5)
      _note("softmax", D.check(probs, 0.5 * pa, D.softmax_bound(a, 0.5), D.LEGACY_GRAD, f"softmax n={n} C={C}"))
      first = probs.clone()
      out = ops.distill_softmax_acc(b.to(dev), 0.5, probs)
      assert out is probs
      D.check(probs, 0.5 * (pa + pb), D.softmax_bound(a, 0.5) + D.softmax_bound(b, 0.5) + D.U, D.LEGACY_GRAD,
              f"ensemble n={n} C={C}")
      assert (probs.double().sum(-1) - 1).abs().max() <= 1e-5
      assert not torch.equal(first, probs) or C == 1
  print(WORST.get("softmax"))


def test_invalid_arguments(dev):
  from big_vision_amd import _lib, ops
  s, T = D.logits(2, 1, 1).to(dev), D.logits(2, 1, 2).to(dev)
  with pytest.raises(RuntimeError, match="label smoothing needs C > 1"):
    ops.distill_dist("hard", s, T, per_row=True, ls=0.1)
  ops.distill_dist("hard", s, T, per_row=True, ls=0.0)
  s, T = D.logits(2, 8, 1).to(dev), D.logits(2, 8, 2).to(dev)
  with pytest.raises(RuntimeError, match="agree"):
    ops.distill_dist("agree", s, T, want_grad=True)
  with pytest.raises(RuntimeError, match="t > 0"):
    ops.distill_dist("kl", s, T, per_row=True, t=0.0)
  with pytest.raises(RuntimeError, match="bad shape"):
    ops.distill_dist("kl", s, T, per_row=True, n_global=1)
  with pytest.raises(AssertionError, match="Unknown kind of distance"):
    ops.distill_dist("cosine", s, T)
  lib = _lib.handle("distill")
  assert lib.bv_distill_dist(9, s.data_ptr(), T.data_ptr(), None, None, None, 0, 2, 8, 2, 1.0, 0.0, 0.0, 1, None) == -1
  assert b"unknown kind" in lib.bv_distill_last_error()
  with pytest.raises(RuntimeError, match="GPU"):
    ops.distill_entropy(torch.zeros(2, 8))
