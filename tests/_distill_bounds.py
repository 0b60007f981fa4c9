"""fp64 restatement of the distillation distances (include/bvdistill.h), their inputs, and per-element rounding-error
bounds for the fp32 kernels of big_vision_amd/csrc/distill.hip, in the manner of tests/_bounds.py.

The reference point of every check is the fp64 restatement `dist64` below (written from the table of bvdistill.h /
distance.py:35-67, utils.py:276-281; torch autograd gives the derivative), never a kernel output.

Tolerance = max(legacy, model), elementwise:
  legacy  what test_kernels_gpu.py::test_softmax_xent holds bv_softmax_xent to: rtol 1e-5 / atol 1e-6 on a loss value,
          rtol 1e-4 / atol 1e-7 on a derivative element;
  model   a forward rounding-error bound of the operation chain the kernel is prescribed to run, evaluated in fp64 on
          the test's own inputs.  It exceeds the legacy tolerance only where the arithmetic makes it: the square roots
          near eps (the value's error is divided by the value), t^2 at large logits, derivative elements that are the
          difference of two nearly equal probabilities.

Model (u = 2^-24, the fp32 unit roundoff; every constant is a deterministic worst case, nothing is fitted):
  * one fp32 operation: relative error u.
  * __expf(x) = v_exp_f32(x * log2(e)): the hardware exp2 is accurate to 1 ulp and the rounded product moves the
    exponent by |x| log2(e) u, i.e. the result by a relative |x| u; with the scaling of x before it,
    rel(__expf(x)) <= EXP0 u + EXPX |x| u, EXP0 = 4, EXPX = 2.
  * logf(z): 2 ulp of the result (the documented bound of the ROCm device library) plus the relative error of z.
  * a sum of C terms held 256 lanes x ceil(C / 256) deep, then 6 shuffle levels and 3 adds:
    |err| <= ACC(C) u sum |terms|, ACC(C) = ceil(C / 256) + 9.
"""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
EXP0, EXPX = 4.0, 2.0
LOG_ULPS = 2.0
LEGACY_VALUE = (1e-5, 1e-6)
LEGACY_GRAD = (1e-4, 1e-7)
KINDS = ("l2", "euclidean", "kl", "hard", "logsoftmax_euclidean")
CLIP = 1e-8


def acc(C):
  return math.ceil(C / 256) + 9.0


# ----------------------------------------------------------------- inputs ----
def logits(n, C, seed, scale=3.0):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn((n, C), generator=g) * scale).float()


def tied_logits(n, C, seed):
  """(student, teacher) whose values are multiples of 1/8 in [-4, 4] with planted exact ties: in every row the
  teacher's maximum appears at two or three columns (the FIRST one is the argmax), and the student's value at that
  column is shared by other columns on both sides of it.  Exact in fp32 and fp64 alike, so the two agree on every
  argmax and every rank."""
  g = torch.Generator().manual_seed(seed)
  s = torch.randint(-32, 33, (n, C), generator=g).float() / 8
  t = torch.randint(-32, 25, (n, C), generator=g).float() / 8
  for r in range(n):
    cols = torch.randperm(C, generator=g)[:3].sort().values
    t[r, cols[: min(3, C)]] = 3.5 + r / 8            # the row's maximum, two or three times
    a = int(cols[0])
    same = torch.randperm(C, generator=g)[: max(1, C // 4)]
    s[r, same] = s[r, a].clone()                      # ties with the student's value at the argmax column
  return s, t


def extreme_logits(seed=7, n=4, C=4000):
  """Logits of magnitude up to 1e3: after the max subtraction most teacher probabilities underflow far below the 1e-8
  clip (some to exactly 0 in fp32).  Row 1: the student equals the teacher and C - 1 teacher classes sit at p ~ 5.6e-9,
  just under the clip - the value IS the clip's contribution.  Row 2: student = teacher + small noise at scale 1e3."""
  g = torch.Generator().manual_seed(seed)
  s = (torch.randn((n, C), generator=g) * 300).clamp(-1e3, 1e3)
  t = (torch.randn((n, C), generator=g) * 300).clamp(-1e3, 1e3)
  s[0, 3], t[0, 5] = 1e3, 1e3
  t[1] = -19.0
  t[1, 17] = 0.0
  s[1] = t[1]
  s[2] = t[2] + torch.randn((C,), generator=g) * 0.25
  return s.float(), t.float()


# ------------------------------------------------------- fp64 restatement ----
def log_softmax64(x):
  x = x - x.max(-1, keepdim=True).values
  return x - x.exp().sum(-1, keepdim=True).log()


def first_argmax(x):
  mx = x.max(-1, keepdim=True).values
  idx = torch.arange(x.shape[-1]).expand_as(x)
  return torch.where(x == mx, idx, torch.full_like(idx, x.shape[-1])).min(-1).values


def hard_labels(teacher, ls):
  C = teacher.shape[-1]
  pl = torch.nn.functional.one_hot(first_argmax(teacher), C).to(F64)
  if ls:
    pl = (1.0 - ls) * pl + (ls / (C - 1)) * (1.0 - pl)
  return pl


def xent_kl64(lg, y):
  """utils.py:276-281 with reduction=False, kl=True."""
  return -(y * log_softmax64(lg)).sum(-1) + (y * y.clamp_min(CLIP).log()).sum(-1)


def dist64(kind, student, teacher, t=1.0, ls=0.0, eps=1e-12, k=1):
  """Per-row distances, fp64 (student may require grad)."""
  s, T = student.to(F64), teacher.to(F64)
  d = s - T
  if kind == "l2":
    return (d * d).sum(-1)
  if kind == "euclidean":
    return ((d * d).sum(-1) + eps).sqrt()
  if kind == "kl":
    return t ** 2 * xent_kl64(s / t, torch.softmax(T / t, -1))
  if kind == "hard":
    return xent_kl64(s, hard_labels(T, ls))
  if kind == "logsoftmax_euclidean":
    e = log_softmax64(s) - log_softmax64(T)
    return ((e * e).sum(-1) + eps).sqrt()
  if kind == "agree":
    a = first_argmax(T)
    sa = s.gather(-1, a[:, None])
    idx = torch.arange(s.shape[-1]).expand_as(s)
    ahead = (s > sa).sum(-1) + ((s == sa) & (idx < a[:, None])).sum(-1)
    return (ahead < k).to(F64)
  raise AssertionError(kind)


def value_and_grad64(kind, student, teacher, n_global=None, **kw):
  """(per-row values [n], d(sum values / n_global)/d student [n, C]) in fp64."""
  s = student.to(F64).clone().requires_grad_(True)
  v = dist64(kind, s, teacher, **kw)
  (v.sum() / (n_global or student.shape[0])).backward()
  return v.detach(), s.grad


def entropy64(lg):
  lp = log_softmax64(lg.to(F64))
  return -(lp.exp() * lp).sum(-1)


# ----------------------------------------------------------------- bounds ----
def _softmax_parts(x, inv_t):
  """max-shifted exponent u_c = (x_c - max) / t, probabilities and the error terms of the kernel's evaluation:
  rel_p[c] relative error of p_c = __expf(u_c) / z, d_lz absolute error of log z."""
  x = x.to(F64)
  u = (x - x.max(-1, keepdim=True).values) * inv_t
  e = u.exp()
  z = e.sum(-1, keepdim=True)
  p = e / z
  C = x.shape[-1]
  rel_e = U * (EXP0 + EXPX * u.abs() + 2.0)                       # subtraction, scaling, __expf
  rel_z = (p * rel_e).sum(-1, keepdim=True) + acc(C) * U          # the terms' errors, weighted, + the accumulation
  lz = z.log()
  d_lz = rel_z + LOG_ULPS * 2 * U * lz.abs().clamp_min(1.0)
  rel_p = rel_e + rel_z + 2 * U                                   # reciprocal of z, product
  return u, p, lz, rel_p, d_lz


def bounds(kind, student, teacher, n_global=None, t=1.0, ls=0.0, eps=1e-12):
  """(value bound [n], derivative bound [n, C]) of the fp32 kernel against dist64 on these inputs."""
  s, T = student.to(F64), teacher.to(F64)
  n, C = s.shape
  inv_n = 1.0 / (n_global or n)
  A = acc(C)
  if kind in ("l2", "euclidean"):
    d = s - T
    ss = (d * d).sum(-1)
    e_ss = (A + 3.0) * U * ss                                     # (d (1 + u))^2 fused into the sum
    if kind == "l2":
      return e_ss + U * ss, inv_n * 6 * U * d.abs()               # 2 d / n_global: the difference, fl(1 / n_global), the product
    v = (ss + eps).sqrt()
    e_v = e_ss / (2 * v) + 2 * U * v + U * eps / v
    g = d / v[:, None] * inv_n
    return e_v, g.abs() * (e_v / v + 4 * U)[:, None]
  if kind in ("kl", "hard"):
    tt = t if kind == "kl" else 1.0
    us, ps, lzs, rel_ps, d_lzs = _softmax_parts(s, 1.0 / tt)
    lp = us - lzs
    e_lp = 2 * U * us.abs() + d_lzs + U * lp.abs()
    if kind == "kl":
      ut, y, lzt, rel_y, d_lzt = _softmax_parts(T, 1.0 / tt)
      ly_raw = ut - lzt
      ly = ly_raw.clamp_min(math.log(CLIP))
      # max(., log 1e-8) is 1-Lipschitz: the clipped value errs by at most what the raw one does, and not at all
      # where the raw one is further below the clip than any such error
      e_ly = torch.where(ly_raw > math.log(CLIP) - 1e-3, 2 * U * ut.abs() + d_lzt + U * ly_raw.abs(), torch.zeros_like(ly))
    else:
      y = hard_labels(T, ls)
      ly = y.clamp_min(CLIP).log()
      rel_y = torch.full_like(y, 3 * U) * (y != 1.0)               # 1 - ls, ls / (C - 1) in fp32
      e_ly = (LOG_ULPS * 2 * U * ly.abs() + rel_y) * (y > 0)
    diff = ly - lp
    term = y * diff
    e_term = y * (e_ly + e_lp + U * diff.abs()) + y * rel_y * diff.abs() + U * term.abs()
    e_sum = e_term.sum(-1) + A * U * term.abs().sum(-1)
    value = tt * tt * term.sum(-1)
    e_v = tt * tt * e_sum + 3 * U * value.abs()
    g_scale = tt * inv_n
    e_g = g_scale * (ps * rel_ps + y * rel_y + 2 * U * (ps - y).abs() + 2 * U * (ps + y))
    return e_v, e_g
  if kind == "logsoftmax_euclidean":
    us, ps, lzs, rel_ps, d_lzs = _softmax_parts(s, 1.0)
    ut, _, lzt, _, d_lzt = _softmax_parts(T, 1.0)
    e = (us - lzs) - (ut - lzt)
    e_e = U * (us.abs() + (us - lzs).abs() + ut.abs() + (ut - lzt).abs() + e.abs()) + d_lzs + d_lzt
    ss = (e * e).sum(-1)
    e_ss = (2 * e.abs() * e_e + e_e * e_e).sum(-1) + (A + 2.0) * U * ss
    se = e.sum(-1)
    e_se = e_e.sum(-1) + A * U * e.abs().sum(-1)
    v = (ss + eps).sqrt()
    e_v = e_ss / (2 * v) + 2 * U * v + U * eps / v
    num = e - ps * se[:, None]
    e_num = e_e + ps * se.abs()[:, None] * (rel_ps + U) + ps * e_se[:, None] + U * num.abs()
    g = num / v[:, None] * inv_n
    e_g = inv_n * e_num / v[:, None] + g.abs() * (e_v / v + 4 * U)[:, None]
    return e_v, e_g
  raise AssertionError(kind)


def entropy_bound(lg):
  u, p, lz, rel_p, d_lz = _softmax_parts(lg, 1.0)
  term = p * (lz - u)
  e_term = term.abs() * (rel_p + 2 * U) + p * (d_lz + U * u.abs())
  return e_term.sum(-1) + acc(lg.shape[-1]) * U * term.abs().sum(-1)


def softmax_bound(lg, weight=1.0):
  _, p, _, rel_p, _ = _softmax_parts(lg, 1.0)
  return abs(weight) * p * (rel_p + 3 * U)


def tolerance(ref, model, legacy):
  rtol, atol = legacy
  return torch.maximum(atol + rtol * ref.abs(), model)


def check(out, ref, model, legacy, name):
  """|out - ref| <= max(legacy, model) elementwise; NaN / Inf fail.  Returns (worst error / tolerance, worst error /
  model bound)."""
  o, r = out.detach().cpu().to(F64), ref.detach().cpu().to(F64)
  assert o.shape == r.shape, (name, tuple(o.shape), tuple(r.shape))
  assert torch.isfinite(o).all(), f"{name}: non-finite output"
  err = (o - r).abs()
  tol = tolerance(r, model.to(F64), legacy)
  ratio = (err / tol).max().item()
  ratio_model = (err / model.clamp_min(1e-300)).max().item()
  bad = err > tol
  assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the bound, worst err/tol {ratio:.3g} "
                         f"(max abs err {err.max().item():.3e}, ref max {r.abs().max().item():.3e})")
  return ratio, ratio_model
