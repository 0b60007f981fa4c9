"""GSAM gradient (Surrogate Gap Guided Sharpness-Aware Minimization, arXiv 2203.08065) on the flat parameter store,
mirroring `big_vision/trainers/proj/gsam/gsam.py`.

Reference: `gsam_gradient` (:29-122): the clean loss and gradient (:69), its norm (`dual_vector`, :19-27, :70), the
perturbation radius `sam_rho` from the learning rate (:72-75), the per-worker perturbation `params + sam_rho g_clean /
(|g_clean| + eps)` (:82-83), the gradient at the perturbed weights (:86) and the decomposition of one gradient along
the other (:92-119).  `rho_max == rho_min`, `alpha == 0` is SAM (:67).

Kept: the name `gsam_gradient`, its hyper-parameters with their defaults, the clean loss as the returned loss, a
gradient that is NOT averaged over the workers (the trainer does that, train.py:211).
New: parameters and gradients are the flat fp32 buffers of a ParamStore, so every tree-wide operation of the reference
is one vector operation.  Both decompositions collapse to `g_gsam = a g_robust + b g_clean` (`combine_coefficients`):

  minimize_fp (:92-105)      a = 1 + alpha <g_r, g_c> / |g_r|^2      b = -alpha
  otherwise   (:106-119)     a = alpha                               b = 1 - alpha <g_r, g_c> / |g_c|^2

The three reductions are `bv_sqnorm` / `bv_dot_f32`; the perturbation and the combination are `y <- a_y y + a_x x`
on `bv_sgemm_strided` against a 64 x 64 identity (`axpby_`).  The scalars (sam_rho, the perturbation scale, a, b) are
fp64 host arithmetic on the reductions' results: 8 bytes cross to the host after the clean pass and 16 after the robust pass
(none there when alpha == 0: the coefficients do not depend on the reductions).  The unperturbed fp32 master and its
bf16 shadow are kept as copies over the robust pass and copied back, so they are restored bit for bit.

Out of scope: `adaptive_perturbation=True` (:78-80) needs the element-wise product |p| g, which no entry point of
libbvhip computes; it raises NotImplementedError.  Frozen leaves have no gradient here, so they are not perturbed and
do not count in |g_clean| (the reference differentiates them too and freezes only their update).
"""
from __future__ import annotations

import math

import torch

from big_vision_amd import ops

F32 = torch.float32
F64 = torch.float64

# y <- a_y y + a_x x runs on bv_sgemm_strided over the buffers seen as [rows, 64] matrices (see axpby_).  Its grids put
# ceil(rows / 64) (VALU kernel) or ceil(rows / 128) (matrix-pipe kernels) workgroups along gridDim.y, which ends at
# 65535: at most 65535 * 64 rows per launch; 4095 * 1024 rows (268 M elements) keeps the ranges whole 1024-element chunks
AXPBY_COLS = 64
AXPBY_ROWS = 4095 * 1024


def hparams(rho_max, rho_min, alpha, lr_max, lr_min, eps=1e-12, adaptive_perturbation=False, minimize_fp=True):
  """`config.gsam` as the keyword arguments of the reference's gsam_gradient (:29-31): a missing or an unknown key is
  the TypeError that calling it would give."""
  if adaptive_perturbation:
    raise NotImplementedError(
        "config.gsam.adaptive_perturbation=True (gsam.py:78-80) perturbs by |p| * sam_rho * g / (|g| + eps): an "
        "element-wise product of the parameters and the gradient, which no existing libbvhip entry point computes "
        "(DESIGN.md 4.5, 4.51)")
  return dict(rho_max=float(rho_max), rho_min=float(rho_min), alpha=float(alpha), lr_max=float(lr_max),
              lr_min=float(lr_min), eps=float(eps), minimize_fp=bool(minimize_fp))


def sam_rho(lr, rho_max, rho_min, lr_max, lr_min):
  """Perturbation radius at learning rate `lr` (:72-75)."""
  if lr_max == lr_min:
    return rho_max
  return rho_min + (rho_max - rho_min) * (lr - lr_min) / (lr_max - lr_min)


def perturbation_scale(rho, g_clean_sqnorm, eps=1e-12):
  """c of `params + c g_clean` (:82-83): sam_rho / (|g_clean| + eps)."""
  return rho / (math.sqrt(g_clean_sqnorm) + eps)


def combine_coefficients(alpha, minimize_fp, dot=None, g_robust_sqnorm=None, g_clean_sqnorm=None):
  """(a, b) of g_gsam = a g_robust + b g_clean (:92-119); dot = <g_robust, g_clean>.  alpha == 0 needs no reduction."""
  if minimize_fp:
    # g_r - alpha (g_c - <g_r / |g_r|, g_c> g_r / |g_r|)
    return (1.0 + alpha * dot / g_robust_sqnorm if alpha else 1.0), -alpha
  # g_c + alpha (g_r - <g_c / |g_c|, g_r> g_c / |g_c|)
  return alpha, (1.0 - alpha * dot / g_clean_sqnorm if alpha else 1.0)


def axpby_(y, a_y, x, a_x, eye, rows=AXPBY_ROWS):
  """y <- a_y y + a_x x over flat fp32 buffers of a multiple of 64 elements, in place: bv_sgemm_strided as
  C[R, 64] = a_x A[R, 64] I[64, 64] + a_y C with `eye` the device identity, in ranges of `rows` rows.  The kernels are
  k-ordered fmaf chains, so A I is x bit for bit (x_k * 0 adds an exact zero) and the result is
  fl(fl(a_x x) + fl(a_y y)); a_y == 0 never reads y.  (N = 1, K = 1 gives the same values on 1/64 of each workgroup:
  measured 5.3 ms against 0.65 ms per sweep of 88 M elements)  A non-finite x spreads over its row of
  64 (inf * 0): such a step is lost either way, check_finite stops it."""
  n, w = y.numel(), AXPBY_COLS
  assert x.numel() == n and n % w == 0 and y.is_contiguous() and x.is_contiguous()
  for lo in range(0, n // w, rows):
    m = min(rows, n // w - lo)
    ops.sgemm(x[lo * w:(lo + m) * w], w, 1, eye, w, 1, y[lo * w:(lo + m) * w].view(m, w), m, w, w, alpha=a_x, beta=a_y)
  return y


class Buffers:
  """What the GSAM step keeps beside a ParamStore, allocated once: `g_clean` (the clean gradient, kept over the
  robust pass), copies of the fp32 master and the bf16 shadow of the trainable prefix, the reductions' accumulators."""

  def __init__(self, store):
    if store.master_sharded:
      raise NotImplementedError("the GSAM step perturbs the whole fp32 master: sharded parameters are not supported")
    n, dev = store.trainable_count, store.device
    self.store = store
    self.g_clean = torch.zeros(n, device=dev, dtype=F32)
    self.master = torch.empty(n, device=dev, dtype=F32)
    self.shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    self.eye = torch.eye(AXPBY_COLS, device=dev, dtype=F32)      # the B operand of axpby_
    self.red = torch.zeros(3, device=dev, dtype=F64)     # |g_clean|^2, <g_robust, g_clean>, |g_robust|^2


def gsam_gradient(grad_fn, store, buf, *, rho_max, rho_min, alpha, lr, lr_max, lr_min, eps=1e-12,
                  minimize_fp=True, scale=1.0, stages=None):
  """The GSAM gradient (:69-122), times `scale`, into `store.grad`; returns the clean loss accumulator.

  grad_fn(): one forward / backward at the store's current weights; zeroes and fills `store.grad` and returns the
  loss as an f64[1] device tensor.  buf: this store's Buffers.  stages: a dict that receives, for tests, the host
  scalars (`sam_rho`, `c`, `a`, `b`, the reductions) and copies of `g_robust`, the perturbed master and shadow."""
  n = store.trainable_count
  master, shadow = store.master[:n], store.shadow[:n]
  # clean pass (:69-70)
  loss = grad_fn()
  buf.g_clean.copy_(store.grad)
  buf.red.zero_()
  ops.sqnorm_(buf.g_clean, buf.red[0:1])
  rho = sam_rho(lr, rho_max, rho_min, lr_max, lr_min)
  sq_clean = buf.red[0].item()                       # 8 bytes to the host; waits for the clean pass
  c = perturbation_scale(rho, sq_clean, eps)
  # per-worker perturbation (:82-83) of the weights every kernel reads: the fp32 master and its bf16 shadow
  buf.master.copy_(master)
  buf.shadow.copy_(shadow)
  axpby_(master, 1.0, buf.g_clean, c, buf.eye)
  ops.cast_bf16(master, shadow)
  store.shadow_version += 1
  if stages is not None:
    stages.update(master_perturbed=master.clone(), shadow_perturbed=shadow.clone())
  # robust pass (:86), then the weights come back bit for bit
  try:
    grad_fn()
  finally:
    master.copy_(buf.master)
    shadow.copy_(buf.shadow)
    store.shadow_version += 1
  # decomposition (:92-119)
  dot = sq_robust = None
  if alpha:
    ops.dot_(store.grad, buf.g_clean, buf.red[1:2])
    ops.sqnorm_(store.grad, buf.red[2:3])
    dot, sq_robust = buf.red[1:3].tolist()           # 16 bytes to the host; waits for the robust pass
  a, b = combine_coefficients(alpha, minimize_fp, dot, sq_robust, sq_clean)
  if stages is not None:
    stages.update(sam_rho=rho, c=c, a=a, b=b, sq_clean=sq_clean, dot=dot, sq_robust=sq_robust,
                  g_robust=store.grad.clone())
  axpby_(store.grad, a * scale, buf.g_clean, b * scale, buf.eye)
  return loss
