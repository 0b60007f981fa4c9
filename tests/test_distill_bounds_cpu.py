"""The bounds of tests/_distill_bounds.py bite (in the style of test_tolerance_power_cpu.py): the fp64 restatement
rounded once to fp32 passes every check, and each of seven plausible slips of a distillation-loss kernel - written
here as fp64 mutants of the restatement - is rejected on at least one element of the value or of the derivative."""
import pytest
import torch

import _distill_bounds as D

F64 = torch.float64


def _check_all(kind, out_v, out_g, s, T, n_global=None, **kw):
  ref_v, ref_g = D.value_and_grad64(kind, s, T, n_global=n_global, **kw)
  bv, bg = D.bounds(kind, s, T, n_global=n_global, **kw)
  D.check(out_v, ref_v, bv, D.LEGACY_VALUE, f"{kind} value")
  D.check(out_g, ref_g, bg, D.LEGACY_GRAD, f"{kind} derivative")


CASES = [("l2", {}), ("euclidean", {}), ("kl", dict(t=0.5)), ("kl", dict(t=2.0)), ("hard", dict(ls=0.0)),
         ("hard", dict(ls=0.1)), ("logsoftmax_euclidean", {})]


@pytest.mark.parametrize("kind,kw", CASES, ids=[f"{k}-{v}" for k, v in CASES])
@pytest.mark.parametrize("C", [5, 257, 1000])
def test_the_restatement_rounded_to_fp32_passes(kind, kw, C):
  s, T = (D.tied_logits(3, C, 1) if kind == "hard" else (D.logits(3, C, 1), D.logits(3, C, 2)))
  v, g = D.value_and_grad64(kind, s, T, n_global=12, **kw)
  _check_all(kind, v.float(), g.float(), s, T, n_global=12, **kw)


def test_the_restatement_passes_on_the_extreme_inputs():
  s, T = D.extreme_logits()
  for t in (1.0, 2.0):
    v, g = D.value_and_grad64("kl", s, T, t=t)
    _check_all("kl", v.float(), g.float(), s, T, t=t)
  y = torch.softmax(T.double(), -1)
  assert (y < D.CLIP).float().mean() > 0.9 and (y[0] == 0).any()      # the case is what its docstring says


def _mutant(fn, s, T, n_global):
  s64 = s.to(F64).clone().requires_grad_(True)
  v = fn(s64, T.to(F64))
  (v.sum() / n_global).backward()
  return v.detach(), s64.grad


def _kl(s, T, t, power=2, entropy=True, clip=True):
  y = torch.softmax(T / t, -1)
  v = -(y * D.log_softmax64(s / t)).sum(-1)
  if entropy:
    v = v + ((y * y.clamp_min(D.CLIP).log()) if clip else torch.xlogy(y, y)).sum(-1)
  return t ** power * v


def _hard(s, T, ls, denom_c=False, last=False):
  C = T.shape[-1]
  a = (C - 1 - D.first_argmax(T.flip(-1))) if last else D.first_argmax(T)
  pl = torch.nn.functional.one_hot(a, C).to(F64)
  if ls:
    pl = (1.0 - ls) * pl + (ls / (C if denom_c else C - 1)) * (1.0 - pl)
  return D.xent_kl64(s, pl)


def test_mutants_are_rejected():
  s, T = D.logits(3, 257, 1), D.logits(3, 257, 2)
  ts, tT = D.tied_logits(3, 257, 1)
  xs, xT = D.extreme_logits()
  n = 3
  mutants = {
      "t instead of t^2": ("kl", dict(t=2.0), s, T, n, lambda a, b: _kl(a, b, 2.0, power=1)),
      "no -H(y) term": ("kl", dict(t=2.0), s, T, n, lambda a, b: _kl(a, b, 2.0, entropy=False)),
      "clip dropped": ("kl", dict(t=1.0), xs, xT, 4, lambda a, b: _kl(a, b, 1.0, clip=False)),
      "ls / C instead of ls / (C - 1)": ("hard", dict(ls=0.1), ts, tT, n, lambda a, b: _hard(a, b, 0.1, denom_c=True)),
      "last instead of first argmax": ("hard", dict(ls=0.1), ts, tT, n, lambda a, b: _hard(a, b, 0.1, last=True)),
  }
  for name, (kind, kw, a, b, ng, fn) in mutants.items():
    v, g = _mutant(fn, a, b, ng)
    with pytest.raises(AssertionError):
      _check_all(kind, v.float(), g.float(), a, b, n_global=ng, **kw)
    ok_v, ok_g = D.value_and_grad64(kind, a, b, n_global=ng, **kw)     # ... and the unmutated function passes there
    _check_all(kind, ok_v.float(), ok_g.float(), a, b, n_global=ng, **kw)


def test_the_clip_mutant_is_caught_by_the_value_of_the_row_at_the_clip():
  """Row 1 of the extreme inputs: student = teacher, 3999 classes at p ~ 5.6e-9.  Its value is 3999 y (log 1e-8 - log y)
  ~ 1.3e-5; without the clip it is 0."""
  xs, xT = D.extreme_logits()
  ref = D.dist64("kl", xs, xT)
  mut = _kl(xs.double(), xT.double(), 1.0, clip=False)
  bv, _ = D.bounds("kl", xs, xT)
  tol = D.tolerance(ref, bv, D.LEGACY_VALUE)
  assert 1e-5 < ref[1] < 2e-5 and (mut[1] - ref[1]).abs() > 2 * tol[1]


def test_gradient_mutants_are_rejected():
  s, T = D.logits(3, 257, 1), D.logits(3, 257, 2)
  ref_v, ref_g = D.value_and_grad64("logsoftmax_euclidean", s, T, n_global=3)
  _, bg = D.bounds("logsoftmax_euclidean", s, T, n_global=3)
  e = D.log_softmax64(s.double()) - D.log_softmax64(T.double())
  no_p_term = e / ref_v[:, None] / 3                                    # without - p sum_c e_c
  with pytest.raises(AssertionError):
    D.check(no_p_term.float(), ref_g, bg, D.LEGACY_GRAD, "lse derivative without the p sum e term")
  # mean over n instead of n_global: every kind's derivative and loss share are 4x too large on a 4-rank batch
  for kind, kw in CASES:
    a, b = (D.tied_logits(3, 257, 1) if kind == "hard" else (s, T))
    _, g_n = D.value_and_grad64(kind, a, b, n_global=3, **kw)
    ref_v, ref_g = D.value_and_grad64(kind, a, b, n_global=12, **kw)
    _, bg = D.bounds(kind, a, b, n_global=12, **kw)
    with pytest.raises(AssertionError):
      D.check(g_n.float(), ref_g, bg, D.LEGACY_GRAD, f"{kind} derivative over n")
    loss_bound = D.bounds(kind, a, b, n_global=12, **kw)[0].sum() / 12
    with pytest.raises(AssertionError):
      D.check((ref_v.sum() / 3).float().reshape(1), (ref_v.sum() / 12).reshape(1), loss_bound.reshape(1), D.LEGACY_VALUE,
              f"{kind} loss over n")


def test_entropy_and_softmax_bounds_accept_fp32_and_reject_slips():
  x = D.logits(3, 1003, 4)
  h = D.entropy64(x)
  D.check(h.float(), h, D.entropy_bound(x), D.LEGACY_VALUE, "entropy")
  with pytest.raises(AssertionError):      # entropy in bits
    D.check((h / 0.6931471805599453).float(), h, D.entropy_bound(x), D.LEGACY_VALUE, "entropy / ln 2")
  p = torch.softmax(x.double(), -1)
  D.check((0.5 * p).float(), 0.5 * p, D.softmax_bound(x, 0.5), D.LEGACY_GRAD, "softmax")
  with pytest.raises(AssertionError):      # unnormalised weight
    D.check(p.float(), 0.5 * p, D.softmax_bound(x, 0.5), D.LEGACY_GRAD, "softmax, weight dropped")


def test_agree_restatement_breaks_ties_to_the_lower_index():
  s = torch.tensor([[1.0, 2.0, 2.0, 0.0], [2.0, 2.0, 1.0, 2.0]])
  T = torch.tensor([[0.0, 5.0, 5.0, 1.0], [0.0, 1.0, 1.0, 1.0]])    # argmax 1 (first of two), 1 (first of three)
  assert D.dist64("agree", s, T, k=1).tolist() == [1.0, 0.0]        # row 1: column 0 ties and comes first
  assert D.dist64("agree", s, T, k=2).tolist() == [1.0, 1.0]
  got = torch.topk(s, 2, dim=-1).indices                             # (torch.topk's tie order is unspecified: the counts are)
  assert got.shape == (2, 2)
