"""fp64 restatement of one batch of the classification evaluator (include/bveval.h), its inputs, and a per-element
rounding-error model of the fp32 kernel of big_vision_amd/csrc/eval.hip, in the manner of tests/_distill_bounds.py.

The reference point of every check is `classify64` below, written from evaluators/classification.py:37-53 and
utils.py:236-243 / :276-281 of the reference, never from a kernel output.

Tolerance of a loss value = max(legacy, model):
  legacy  what test_kernels_gpu.py::test_softmax_xent grants a loss value: rtol 1e-5 / atol 1e-6;
  model   a forward rounding-error bound of the operation chain the kernel runs, evaluated in fp64 on the test's own
          inputs.  It exceeds the legacy tolerance where the arithmetic makes it: `(sum y) lse - sum y l` cancels at
          large logits, and a long row passes through many rescales.
Counts (ncorrect, nseen) and argmax columns carry NO tolerance: with 0/1 labels, 0/1 masks and dyadic logits fp32 and
fp64 agree exactly.

Model (u = 2^-24; the `__expf` / `logf` constants are those of tests/_distill_bounds.py; every constant is a
deterministic worst case, nothing is fitted to GPU output):
  * one fp32 operation: relative error u.  __expf(x): relative EXP0 u + EXPX |x| u.  logf / log1pf: LOG_ULPS ulp of the
    result (the documented bound of the ROCm device library for both).
  * a row is shared by LANES(C) lanes (64 for C <= 1024, a wave per row; 256 above, a workgroup per row), each holding
    DEPTH(C) = ceil(C / LANES) columns.  A sum over the row is DEPTH deep in a lane, then 6 shuffle levels and (for a
    workgroup) 2 more merges: |err| <= ACC(C) u sum |terms|, ACC = DEPTH + 9.
  * online log-sum-exp: a lane rescales its running sum once per group of four columns (and once per column of a tail
    of at most three), and every merge level rescales again: an exponential reaches the row's final sum through at
    most RESCALES(C) = ceil(DEPTH / 4) + 3 + 8 further factors exp(m_old - m_new) after its own.  All exponents along
    that chain are <= 0 and add up to x_c - max(x), so the |x|-proportional parts of the __expf errors (and of the
    subtractions that form the arguments) add up to (EXPX + 1) |x_c - max x| u, and each of the RESCALES + 1 factors adds
    (EXP0 + 2) u (its __expf, the multiplication, the addition).  A result below the normal range may be flushed: an
    absolute 2^-126 per column.
"""
import math

import torch

from _distill_bounds import EXP0, EXPX, LEGACY_VALUE, LOG_ULPS, U, check, tolerance  # noqa: F401  (re-exported)

F64 = torch.float64
WAVE_ROW_MAX_C = 1024          # BVE_WAVE_ROW_MAX_C of include/bveval.h
TINY = 2.0 ** -126
LOSSES = ("softmax_xent", "sigmoid_xent")


def lanes(C):
  return 64 if C <= WAVE_ROW_MAX_C else 256


def depth(C):
  return math.ceil(C / lanes(C))


def acc(C):
  return depth(C) + 9.0


def rescales(C):
  return math.ceil(depth(C) / 4) + 3 + 8.0


# ----------------------------------------------------------------- inputs ----
def dyadic_logits(n, C, seed, lo=-32, hi=32):
  """Multiples of 1/8 in [lo / 8, hi / 8]: exact in fp32 and fp64 alike, so both agree on every comparison.  Long rows
  hold every value many times over: the argmax is decided by the tie rule there."""
  g = torch.Generator().manual_seed(seed)
  return torch.randint(lo, hi + 1, (n, C), generator=g).float() / 8


def first_argmax(x):
  """jnp.argmax: a NaN is the maximum, the first NaN / the first maximum wins."""
  x = torch.as_tensor(x)
  key = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)
  if torch.isnan(x).any():   # +inf logits would tie with the NaN stand-in: not used by any builder here
    assert not torch.isinf(x).any()
  mx = key.max(-1, keepdim=True).values
  idx = torch.arange(x.shape[-1]).expand_as(x)
  return torch.where(key == mx, idx, torch.full_like(idx, x.shape[-1])).min(-1).values


def onehot_labels(logits, seed):
  """One-hot rows: even rows carry the label at the argmax column (a correct prediction), odd rows at a random one."""
  n, C = logits.shape
  g = torch.Generator().manual_seed(seed)
  cols = torch.randint(0, C, (n,), generator=g)
  a = first_argmax(logits)
  cols = torch.where(torch.arange(n) % 2 == 0, a, cols)
  return torch.nn.functional.one_hot(cols, C).float()


def multihot_labels(logits, seed, k=3):
  """Up to k ones per row (sigmoid_xent's multi-label rows), the argmax column among them in even rows."""
  n, C = logits.shape
  g = torch.Generator().manual_seed(seed)
  y = onehot_labels(logits, seed)
  for r in range(n):
    y[r, torch.randint(0, C, (k - 1,), generator=g)] = 1.0
  return y


def mask01(n, seed):
  g = torch.Generator().manual_seed(seed)
  m = (torch.rand((n,), generator=g) < 0.7).float()
  m[0] = 1.0
  return m


# ------------------------------------------------------- fp64 restatement ----
def log_sigmoid64(x):
  return torch.clamp(x, max=0.0) - torch.log1p(torch.exp(-x.abs()))


def loss64(loss_name, logits, labels):
  """utils.py:236-243 / :276-281 at reduction=False, fp64."""
  l, y = logits.to(F64), labels.to(F64)
  if loss_name == "softmax_xent":
    s = l - l.max(-1, keepdim=True).values
    return -(y * (s - s.exp().sum(-1, keepdim=True).log())).sum(-1)
  if loss_name == "sigmoid_xent":
    return -(y * log_sigmoid64(l) + (1.0 - y) * log_sigmoid64(-l)).sum(-1)
  raise AttributeError(loss_name)


def classify64(loss_name, logits, labels, mask=None):
  """classification.py:37-53 in fp64.  Returns a dict: `loss` [n] (unmasked, per example), `top1` [n] (int64), `m` [n]
  (mask * max label) and the three sums `ncorrect`, `loss_sum`, `nseen` (floats)."""
  l, y = torch.as_tensor(logits).to(F64), torch.as_tensor(labels).to(F64)
  m = torch.ones(l.shape[0], dtype=F64) if mask is None else torch.as_tensor(mask).to(F64)
  m = m * y.max(-1).values                                    # :41
  loss = loss64(loss_name, l, y)                              # :43-44
  top1 = first_argmax(l)                                      # :47
  correct = y.gather(-1, top1[:, None])[:, 0]                 # :49-50
  return {"loss": loss, "top1": top1, "m": m, "ncorrect": float((correct * m).sum()),
          "loss_sum": float((loss * m).sum()), "nseen": float(m.sum())}


# ----------------------------------------------------------------- bounds ----
def loss_bound(loss_name, logits, labels):
  """Bound [n] of the fp32 kernel's per-example loss against loss64 on these inputs."""
  x, y = logits.to(F64), labels.to(F64)
  C = x.shape[-1]
  A = acc(C)
  if loss_name == "softmax_xent":
    M = x.max(-1, keepdim=True).values
    d = x - M
    e = d.exp()
    z = e.sum(-1, keepdim=True)
    p = e / z
    rel_e = U * ((rescales(C) + 1.0) * (EXP0 + 2.0) + (EXPX + 1.0) * d.abs() + 2.0)   # + the two adds of a group of four
    rel_z = (p * rel_e).sum(-1) + C * TINY
    lz = z.log()[:, 0]
    lse = M[:, 0] + lz
    d_lse = rel_z + LOG_ULPS * 2 * U * lz.abs().clamp_min(1.0) + U * lse.abs()
    sy, syl = y.sum(-1), (y * x).sum(-1)
    e_sy = A * U * y.abs().sum(-1)
    e_syl = (A + 1.0) * U * (y * x).abs().sum(-1)
    loss = sy * lse - syl
    return sy.abs() * d_lse + e_sy * lse.abs() + U * (sy * lse).abs() + e_syl + U * loss.abs()
  if loss_name == "sigmoid_xent":
    a = x.abs()
    e = (-a).exp()
    t = torch.log1p(e)
    e_t = e * U * (EXP0 + EXPX * a) + LOG_ULPS * 2 * U * t + TINY
    lp, ln = log_sigmoid64(x), log_sigmoid64(-x)
    e_lp, e_ln = e_t + U * lp.abs(), e_t + U * ln.abs()
    term = y * lp + (1.0 - y) * ln
    e_term = y.abs() * e_lp + (1.0 - y).abs() * e_ln + U * ((y * lp).abs() + 2 * ((1.0 - y) * ln).abs() + term.abs())
    return e_term.sum(-1) + A * U * term.abs().sum(-1)
  raise AttributeError(loss_name)


def sum_bound(ref, row_bound):
  """Bound of acc[1] = sum_i loss_i m_i: the rows' bounds under the same weights; the fp64 products and the fp64 sum
  over rows (in any order) add 2^-52 per operation, n + 1 operations deep at most."""
  n = ref["m"].numel()
  return float((ref["m"].abs() * row_bound).sum() + (n + 1) * 2.0 ** -52 * (ref["loss"] * ref["m"]).abs().sum())


def check_loss_sum(got, ref, row_bound, name):
  """acc[1] against the reference's loss sum under max(legacy, summed model)."""
  return check(torch.as_tensor([got], dtype=F64), torch.as_tensor([ref["loss_sum"]], dtype=F64),
               torch.as_tensor([sum_bound(ref, row_bound)], dtype=F64), LEGACY_VALUE, name)
