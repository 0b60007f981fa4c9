"""Elementwise error bounds derived from the arithmetic each kernel is prescribed to do, and the checkers that hold
the GPU parity tests to them.

A flat `rtol = atol = 1e-2` lets a bf16 output be more than two ulps off at unit scale: truncation instead of
round-to-nearest-even, a double rounding in an epilogue or an erf GELU all pass it.  The bounds here instead follow
the operation sequence the kernels promise (fp32 accumulation of exact products of bf16 operands, one
round-to-nearest-even to the output dtype, the fp32 epilogue arithmetic of bv_common.h, Flax's fast LayerNorm
variance) and are as tight as that arithmetic allows.  tests/test_tolerance_power_cpu.py proves, on the CPU, that
every bound accepts an emulation of the prescribed arithmetic and rejects a catalogue of plausible slips.

Model (u = 2^-24, the fp32 unit roundoff):
  * fp32 accumulation of K products: |err| <= gamma(K) u (|A| @ |B|^T), gamma(K) = min(LAM sqrt(K), K).  K u is the
    deterministic worst case; LAM sqrt(K) u is the probabilistic bound of Higham & Mary (SIAM J. Sci. Comput. 2019),
    which holds with probability >= 1 - 2 exp(-LAM^2 / 2) per element when the rounding errors are independent and
    zero-mean.  LAM = 6 puts that below 3e-8, so a 51 M-element output (66 816 x 768) expects < 2 false failures
    from the model's tail even if every element sat at its worst case - and random-sign data sits ~sqrt(K) below it.
  * bf16 output of an fp32 value with error e: 0.5 ulp_bf16(|ref| + e) + e (the ulp is taken at |ref| + e so that a
    value just below a power of two whose fp32 estimate crosses it does not fail falsely).
  * fp32 output: e + F32_ULPS ulp_fp32(|ref|).

Every checker takes the assertion's previous `(rtol, atol)` as `legacy=`: the bound used is min(model, atol + rtol
|ref|) elementwise, so no assertion that moved to a checker became weaker; the report line of each check says on
what share of the elements the legacy cap (not the model) applies.  NaN / Inf in an output fail (the old
`err > tol` test let a NaN through: every comparison with NaN is false).
"""
import collections
import math

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

U = 2.0 ** -24          # fp32 unit roundoff
U_BF16 = 2.0 ** -8      # bf16 unit roundoff: 8 significant bits, ulp(1) = 2^-7, one round-to-nearest-even <= 2^-8
LAM = 6.0               # probabilistic accumulation constant, see the module docstring
F32_ULPS = 4            # fp32 outputs: the final roundings (bias / residual add, store) and the fp32 epilogue ops
LN_EPS = 1e-6           # flax nn.LayerNorm default (layernorm.hip: eps = 1e-6)


# ----------------------------------------------------------------- inputs ----
def rnd(shape, dev, seed, scale=1.0, dtype=F32):
  """The GPU tests' input generator: seeded on the CPU, so the CPU proofs build the very same tensors."""
  g = torch.Generator(device="cpu").manual_seed(seed)
  return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dev).to(dtype)


LN_EDGE_IDX = (0, 1, 2, 3, 4, 7, 10)   # kinds 1e-2, 1e-3, mean, 1e-2, 1e-3, mean, 1e-2; rows 1, 4, 7, 10 (a
                                       # stride-3 selection from row 1) hold all three kinds


def ln_edge_rows(x, idx=LN_EDGE_IDX, seed=90, first_kind=0):
  """Overwrite rows `idx` of x (in place, dtype kept) with the LayerNorm edge rows, cycling through
    mean ~0, std 1e-2   and   mean ~0, std 1e-3  (var + eps depends on eps: these pin eps = 1e-6),
    mean 2, std 0.5     (|mean| / std = 4: E[x^2] - E[x]^2 cancels 17 : 1, the fast variance's weak spot; at
                         |mean| / std >= 8 the Flax formula itself leaves the fp32 output's 1e-5 tolerance).
  Returns the list of (row, kind) written."""
  rows, D = x.shape
  out = []
  for j, r in enumerate(i for i in idx if i < rows):
    kind = (j + first_kind) % 3
    z = rnd((D,), "cpu", seed + j)
    v = (1e-2 * z) if kind == 0 else ((1e-3 * z) if kind == 1 else (2.0 + 0.5 * z))
    x[r] = v.to(x.device).to(x.dtype)
    out.append((r, ("std1e-2", "std1e-3", "mean/std4")[kind]))
  return out


def siglip_extreme_inputs(dev, n=7, B=21, off=14, E=32):
  """SigLIP at t = 100 (t' = log 100, not clipped) and b = -10: logits t z_i.z_j + b reach about -110 .. +90."""
  zi = torch.nn.functional.normalize(rnd((n, E), dev, 81), dim=1)
  zt = torch.nn.functional.normalize(rnd((B, E), dev, 82), dim=1)
  zt[off:off + n] = 0.9 * zt[off:off + n] + 0.1 * zi
  zt = torch.nn.functional.normalize(zt, dim=1)
  zt[0] = zi[0]    # a negative identical to image 0: logit +90, where exp(-m s) = exp(90) overflows fp32
  zt[1] = -zi[1]   # an anti-aligned negative: logit -110
  return zi, zt


def softmax_xent_extreme_inputs(dev, n=6, C=1000):
  """Logits up to +-1e3 (rows: one-hot on the maximum, soft labels over a spread of 2e3, a row at -1e3 but one)."""
  logits = rnd((n, C), dev, 83, 300.0).clamp(-1e3, 1e3)
  logits[0, 5] = 1e3
  logits[1] = -1e3; logits[1, 7] = 1e3
  logits[2] = 1e3 * torch.tanh(rnd((C,), dev, 84))
  labels = torch.softmax(rnd((n, C), dev, 85, 2.0), -1)
  labels[0] = 0; labels[0, 5] = 1.0
  labels[3] = 0; labels[3, 11] = 1.0
  return logits, labels


def sigmoid_xent_extreme_inputs(dev, n=4, C=300):
  """Logits beyond +-90 (exp(|l|) overflows fp32 above 88.7), up to +-1e3, with soft labels."""
  logits = rnd((n, C), dev, 86, 60.0)
  logits[0, :6] = torch.tensor([95.0, -95.0, 200.0, -200.0, 1e3, -1e3])
  logits[1] = 120.0 * torch.sign(rnd((C,), dev, 87))
  labels = torch.rand((n, C), generator=torch.Generator().manual_seed(88)).to(dev)
  return logits, labels


def opt_inputs(n, dev, seed, zero_grad=False):
  """(p, g) of the optimizer tests, fp32: parameters cycling through p = 0, |p| ~ 1e-4 (the update is resolved to
  ulps there, not to ulp(p)), |p| ~ 1 and a few |p| ~ 30; gradients of scale 1e-3 with a few exact zeros and a few
  1e-12 elements."""
  p = rnd((n,), "cpu", seed)
  k = torch.arange(n) % 8
  p = torch.where(k == 0, torch.zeros_like(p), torch.where(k < 3, p * 1e-4, p))
  p[5::61] = 30.0 * torch.sign(rnd((n,), "cpu", seed + 7))[5::61]
  g = rnd((n,), "cpu", seed + 1, 1e-3)
  g[3::37] = 0.0
  g[11::41] = 1e-12
  if zero_grad:
    g.zero_()
  return p.to(dev), g.to(dev)


# Adafactor leaves of the optimizer tests: (name, buffer shape, index into it giving the leaf, gradient edit).  The
# leaf is the indexed view of a contiguous buffer, so its strides / offset are those of a slice of a fused or padded
# tensor; factored_dims + af_view (big_vision_amd/optax.py) turn it into the kernel's [B1][B2][R][C] view.
_S = slice
AF_SPECS = [
    ("32x33", (32, 33), (), None), ("33x32", (33, 32), (), None), ("32x257", (32, 257), (), None),
    ("300x64", (300, 64), (), None), ("64x64", (64, 64), (), None),
    ("qkv-query", (128, 3, 2, 64), (_S(None), 0), None), ("qkv-key", (128, 3, 2, 64), (_S(None), 1), None),
    ("2x3x32x40-padded", (2, 5, 34, 48), (_S(None), _S(1, 4), _S(1, 33), _S(3, 43)), None),
    ("one", (1,), (), None), ("100", (100,), (), None), ("257", (257,), (), None), ("31x500", (31, 500), (), None),
    ("2x3x5x7", (2, 3, 5, 7), (), None),
    ("40x48-zero-row-col", (40, 48), (), "rowcol"), ("32x36-zero-grad", (32, 36), (), "zero"),
]


def af_leaf_inputs(spec, dev, seed):
  """Buffers (flat fp32 p, g of the whole buffer) and the leaf's (shape, strides, offset) for one AF_SPECS entry."""
  name, bshape, index, edit = spec
  n = math.prod(bshape)
  p, g = opt_inputs(n, "cpu", seed)
  t = torch.empty(bshape, device="meta")[index]
  shape, strides, off = tuple(t.shape), tuple(t.stride()), t.storage_offset()
  gv = g.as_strided(shape, strides, off)
  if edit == "zero":
    gv.zero_()
  elif edit == "rowcol":
    gv[3, :] = 0.0
    gv[:, 5] = 0.0
  return p.to(dev), g.to(dev), shape, strides, off


# ------------------------------------------------------------------ units ----
def _exp2_floor_log2(x):
  return torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126))))


def ulp_bf16(x):
  """Spacing of bf16 numbers at magnitude |x| (8 significant bits); normal range."""
  return _exp2_floor_log2(x) * 2.0 ** -7


def ulp_f32(x):
  return _exp2_floor_log2(x) * 2.0 ** -23


def gamma(K):
  """Accumulation constant of a K-term fp32 sum (see the module docstring)."""
  return min(LAM * math.sqrt(K), float(K))


def acc_term(absprod, K):
  """Error of an fp32-accumulated K-term contraction whose |A| @ |B|^T is absprod."""
  return gamma(K) * U * absprod.double()


def bf16_bound(ref, e):
  """bf16 output (one round-to-nearest-even) of an fp32 value within e of ref."""
  a = ref.double().abs() + e
  return 0.5 * ulp_bf16(a) + e


def f32_bound(ref, e, ulps=F32_ULPS):
  return e + ulps * ulp_f32(ref)


# --------------------------------------------------------------- checker ----
def check(out, ref, bound, legacy, name="", lo_hi=None, report=True):
  """|out - ref| <= bound elementwise, the model bound capped elementwise at the legacy atol + rtol |ref|.
  lo_hi: optional (lo, hi) tensors; then the error is the distance of out from the interval [lo, hi] (the prescribed
  value is known only to lie in it, e.g. a bf16 operand that the kernel rounds from an fp32 value sitting within its
  evaluation error of a rounding midpoint) and the legacy assertion |out - ref| <= legacy is made separately.
  Returns max(err / bound)."""
  rtol, atol = legacy
  o = out.double()
  r = ref.double().to(o.device)
  leg = atol + rtol * r.abs()
  if bound is None:
    b, capped = leg, None
  else:
    model = bound.double().to(o.device).expand_as(r)
    capped = ~(model <= leg)   # where the model is looser than the legacy tolerance, the legacy tolerance applies
    b = torch.where(capped, leg, model)
  if lo_hi is None:
    err = (o - r).abs()
  else:
    lo, hi = (t.double().to(o.device) for t in lo_hi)
    err = torch.maximum(torch.maximum(lo - o, o - hi), torch.zeros_like(o))
    lerr = (o - r).abs()
    lbad = ~(lerr <= leg)
    assert not bool(lbad.any()), f"{name}: {int(lbad.sum())}/{lbad.numel()} outside the legacy tolerance"
  bad = ~(err <= b)          # NaN fails
  ratio = (err / b.clamp_min(1e-300)).nan_to_num(float("inf"))
  worst = ratio.max().item() if ratio.numel() else 0.0
  if report:
    cap = "legacy tolerance only" if capped is None else \
        f"legacy cap applies on {100 * capped.double().mean().item():.1f}%"
    print(f"[bounds] {name}: max err/bound {worst:.3f}, {cap}")
  assert not bool(bad.any()), (f"{name}: {int(bad.sum())}/{bad.numel()} outside the bound, max err/bound {worst:.3f}, "
                               f"max abs err {(o - r).abs().nan_to_num(float('inf')).max().item():.3e} "
                               f"(ref max {r.abs().max().item():.3e})")
  return worst


def count_rejected(out, ref, bound, legacy=None, lo_hi=None):
  """Number of elements the checker would reject (for the CPU proofs)."""
  o = out.double(); r = ref.double()
  b = bound.double().expand_as(r)
  if legacy is not None:
    b = torch.minimum(b, legacy[1] + legacy[0] * r.abs())
  if lo_hi is None:
    err = (o - r).abs()
  else:
    lo, hi = (t.double() for t in lo_hi)
    err = torch.maximum(torch.maximum(lo - o, o - hi), torch.zeros_like(o))
  return int((~(err <= b)).sum())


# ------------------------------------------------------------------ GEMM ----
def gemm_f32(ref, absprod, K, n_adds=1):
  """fp32 output: accumulation + the fp32 adds of the epilogue (bias, residual / position row)."""
  e = acc_term(absprod, K)
  return f32_bound(ref, e, F32_ULPS + n_adds)


def gemm_bf16(ref, absprod, K, n_adds=1):
  """bf16 output of an fp32-accumulated GEMM (+ n_adds fp32 epilogue adds, each one rounding of |ref| + e)."""
  e = acc_term(absprod, K)
  e = e + n_adds * U * (ref.double().abs() + e) * 2
  return bf16_bound(ref, e)


def absprod(a, b_t):
  """|A| @ |B|^T of the bf16 operands as the kernel sees them (A [M][K], B^T [K][N]), fp64."""
  return a.double().abs() @ b_t.double().abs()


# ------------------------------------------------------------------ GELU ----
_K0 = -2.0 * 1.4426950408889634 * 0.7978845608028654   # bv_common.h: z = x (k0 + k1 x^2), g = x / (1 + 2^z)
_K1 = _K0 * 0.044715


def _gelu_sig64(x):
  """s = sigmoid(2u) = (1 + tanh(u)) / 2 without the cancellation of 1 + tanh(u) for x << 0 (torch's fp64 tanh-form
  GELU loses every digit below x ~ -6)."""
  return torch.sigmoid(2 * 0.7978845608028654 * (x + 0.044715 * x ** 3))


def gelu_tanh64(h):
  x = h.double()
  return x * _gelu_sig64(x)


def dgelu_tanh64(h):
  x = h.double()
  s = _gelu_sig64(x)
  return s + x * s * (1 - s) * 2 * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)


def _gelu_eval_err(h):
  """Error of the fp32 evaluation of g = x s, s = 1 / (1 + 2^z) (one exp2, one rcp, 4 fp32 roundings), and of
  g' = s + g (1 - s) u', as (e_g, e_dg).  z is computed with a relative error of a few u; 2^z amplifies it by
  ln 2 |z|; the hardware exp2 / rcp are within 1-2 ulp.  Safety factor 2."""
  x = h.double()
  z = x * (_K0 + _K1 * x * x)
  s = torch.sigmoid(-z * math.log(2.0))
  g = x * s
  up = 2 * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)
  rel = U * (16 + 4 * z.abs())
  return rel * g.abs(), rel * (s.abs() + (g * (1 - s) * up).abs())


def gelu_g(h):
  """g = bf16(gelu_tanh(h)) of the bf16 pre-activation h the kernel stored: (ref, bound)."""
  ref = gelu_tanh64(h)
  e, _ = _gelu_eval_err(h)
  return ref, bf16_bound(ref, e)


def gelu_dg(h):
  """d = bf16(gelu_tanh'(h)): (ref, bound)."""
  ref = dgelu_tanh64(h)
  _, e = _gelu_eval_err(h)
  return ref, bf16_bound(ref, e)


def rne_bf16(x):
  return x.double().to(F32).to(BF16).double()


def dgelu_bf16_interval(h):
  """The bf16 derivative the GELU' epilogues multiply by lies in [lo, hi]: the roundings of gelu'(h) -+ its fp32
  evaluation error (round-to-nearest-even is monotone).  Almost everywhere lo == hi."""
  d = dgelu_tanh64(h)
  _, e = _gelu_eval_err(h)
  return rne_bf16(d - e), rne_bf16(d + e)


def gelu_bwd(prod, absp, K, h):
  """dX = bf16(P o bf16(gelu'(h))) (bv_common.h mlp_act_from_h: gelu' is rounded to bf16 before the product, as
  GELU_GD stores it), P = the fp32-accumulated product: ((lo, hi) interval of the prescribed value, bound around it)."""
  dlo, dhi = dgelu_bf16_interval(h)
  p = prod.double()
  lo, hi = torch.minimum(p * dlo, p * dhi), torch.maximum(p * dlo, p * dhi)
  e = acc_term(absp, K) * torch.maximum(dlo.abs(), dhi.abs())
  e = e + U * (p.abs() * dhi.abs()) * 2
  mid = torch.maximum(lo.abs(), hi.abs())
  return (lo, hi), bf16_bound(mid, e)


def mul_bwd(prod, absp, K, d):
  """dX = bf16(P o d), d the stored bf16 operand: bound around prod * d."""
  ref = prod.double() * d.double()
  e = acc_term(absp, K) * d.double().abs() + U * ref.abs() * 2
  return ref, bf16_bound(ref, e)


# ------------------------------------------------------------- LayerNorm ----
def _ln_stats(x, eps=LN_EPS):
  x = x.double()
  D = x.shape[-1]
  mean = x.mean(-1, keepdim=True)
  var = x.var(-1, unbiased=False, keepdim=True)
  ex2 = (x * x).mean(-1, keepdim=True)
  # one wave per row: each lane accumulates D / 64 values, then a 6-level butterfly (layernorm.hip wave_sum); a
  # pairwise or two-pass summation is at least as accurate
  gam = gamma(-(-D // 64) + 6) + 2
  dmean = gam * U * x.abs().mean(-1, keepdim=True) + U * mean.abs()
  # fast variance E[x^2] - E[x]^2 in fp32: the sum of squares and the square of the mean each carry their own
  # rounding; the cancellation term (E[x^2] + mean^2) / (var + eps) is what grows for |mean| >> std
  dvar = gam * U * (ex2 + mean * mean) + 2 * mean.abs() * dmean
  rstd = (var + eps).rsqrt()
  r_rel = 0.5 * dvar / (var + eps) + 4 * U     # relative error of rstd (rsqrt within ~2 ulp, + eps add)
  return mean, rstd, dmean, r_rel


def ln_fwd(x, scale, bias, eps=LN_EPS):
  """y = (x - mean) rstd scale + bias with fp32 statistics: (ref, e) where e bounds the fp32 value's error."""
  x = x.double(); s = scale.double(); b = bias.double()
  mean, rstd, dmean, r_rel = _ln_stats(x, eps)
  xh = (x - mean) * rstd
  ref = xh * s + b
  e = xh.abs() * s.abs() * (r_rel + 4 * U) + rstd * s.abs() * dmean + 2 * U * (ref.abs() + b.abs())
  return ref, e


def ln_fwd_bounds(x, scale, bias, eps=LN_EPS):
  """(ref, bound of the fp32 output, bound of the bf16 output)."""
  ref, e = ln_fwd(x, scale, bias, eps)
  return ref, f32_bound(ref, e), bf16_bound(ref, e)


def ln_bwd(x, scale, dy, dres=None, eps=LN_EPS):
  """dx = rstd (g - mean(g) - xh mean(g xh)) (+ dres), g = dy scale, with the forward's fp32 mean / rstd:
  (ref, e)."""
  x = x.double(); s = scale.double(); dy = dy.double()
  D = x.shape[-1]
  mean, rstd, dmean, r_rel = _ln_stats(x, eps)
  xh = (x - mean) * rstd
  g = dy * s
  s1 = g.mean(-1, keepdim=True)
  s2 = (g * xh).mean(-1, keepdim=True)
  dx = rstd * (g - s1 - xh * s2)
  gam = gamma(-(-D // 64) + 6) + 2
  dxh = xh.abs() * (r_rel + 2 * U) + rstd * dmean
  ds1 = gam * U * g.abs().mean(-1, keepdim=True)
  ds2 = gam * U * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * dxh).mean(-1, keepdim=True)
  t = g.abs() + s1.abs() + xh.abs() * s2.abs()
  e = rstd * (t * (r_rel + 4 * U) + s2.abs() * dxh + ds1 + xh.abs() * ds2)
  if dres is not None:
    dx = dx + dres.double()
  e = e + 2 * U * dx.abs()
  return dx, e


def ln_bwd_bounds(x, scale, dy, dres=None, eps=LN_EPS):
  ref, e = ln_bwd(x, scale, dy, dres, eps)
  return ref, f32_bound(ref, e), bf16_bound(ref, e)


# ------------------------------------------------------------- attention ----
def attn_fwd_bounds(qkv, n, L, H, Dh, lens=None):
  """Self-attention forward on the bf16 qkv [n L, 3 H Dh]: (o_ref, o bound, lse_ref, lse bound), fp64.
  Prescribed: S = (q k^T) fp32-accumulated, P = exp(S / sqrt(Dh) - max) in fp32 with an fp32 row sum l, o =
  bf16(sum_k bf16(P) v / l) - the P V product takes bf16 P and V operands, which adds 2^-8 sum_k P |v| (one rounding
  of each P) to the contraction rule; lse = max + log(l)."""
  q, k, v = qkv.double().view(n, L, 3, H, Dh).unbind(2)
  sc = 1.0 / math.sqrt(Dh)
  s = torch.einsum("nqhd,nkhd->nhqk", q, k) * sc
  es = torch.einsum("nqhd,nkhd->nhqk", q.abs(), k.abs()) * sc * gamma(Dh) * U   # error of S
  if lens is not None:
    mask = torch.arange(L, device=s.device)[None, :] < torch.as_tensor(lens, device=s.device)[:, None]
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    es = es.masked_fill(~mask[:, None, None, :], 0.0)
  lse = torch.logsumexp(s, -1)
  p = torch.exp(s - lse[..., None])
  # relative error of each P (S error, the fp32 exponent argument and the hardware exp2) and of the row sum
  smax = s.amax(-1)
  t = es.amax(-1) + 8 * U * (s.abs().nan_to_num(0.0, posinf=0.0, neginf=0.0).amax(-1) + smax.abs() + 1)
  sum_rel = 2 * t + gamma(L) * U
  o = torch.einsum("nhqk,nkhd->nqhd", p, v)
  pv = torch.einsum("nhqk,nkhd->nqhd", p, v.abs())
  tq = t.permute(0, 2, 1)[..., None]
  sq = sum_rel.permute(0, 2, 1)[..., None]
  # P term: each P is rounded to bf16 once (round-to-nearest-even, relative error <= U_BF16 = 2^-8), so the P V
  # numerator is off by at most U_BF16 sum_k P |v|
  e_o = pv * (U_BF16 + 2 * tq + gamma(L) * U) + o.abs() * (sq + 2 * U)
  o_ref = o.reshape(n * L, H * Dh)
  o_b = bf16_bound(o_ref, e_o.reshape(n * L, H * Dh))
  e_lse = t + sum_rel + 4 * U * (lse.abs() + smax.abs() + 1)
  return o_ref, o_b, lse, f32_bound(lse, e_lse)


# --------------------------------------------------- attention backward ----
# What the kernels document (headers and comments of attention3.hip, attention5.hip, attention_dh.hip), per path.
# Which shape takes which path is decided by big_vision_amd/csrc/attn_route.h; attn_bwd_path below restates it for the
# error models and is held to that header for every shape by tests/test_attn_route_cpu.py.
#   every path   S and dP fp32-accumulated over Dh; P = exp2(S c - lse log2 e) from the STORED fp32 lse (so P carries
#                the forward's lse error); dS = P o (dP - delta) in fp32; dV takes bf16(P), dQ / dK take bf16(dS) as
#                MFMA operands, accumulated over L in fp32; 1 / sqrt(Dh) (0.125 exactly at Dh = 64, the fp32
#                1 / sqrtf(Dh) otherwise) multiplies the fp32 accumulator; one round-to-nearest-even to bf16.  Masked
#                (key-padded) launches take the same arithmetic: P of a padded key is exactly 0, so are its dK / dV.
#   attn3 dq     (masked Dh = 64; every adh launch) two sweeps: delta = fp32 rowsum(P o dP), stored.
#   attn3 dq1    (unmasked Dh = 64 outside the one-launch shapes) one sweep: delta~ = rowsum(dO o bf16 O),
#                dS~ = P o (dP - delta~), eps = rowsum(dS~), dQ = sum bf16(dS~) K - eps sum bf16(P) K, delta = delta~
#                + eps is stored for the dK / dV launch.  In exact arithmetic that is P o (dP - delta) with delta =
#                rowsum(P o dP) + delta~ (1 - rowsum P): the terms below marked "dq1".
#   attn5        (the route's ATTN_5 family) one launch: delta as attn3 dq but kept in LDS (never
#                stored: the delta buffer is NOT filled on this path); phase 1b forms dS from the bf16 P of the LDS
#                image, so dS carries one more 2^-8 rounding: the terms marked "attn5".
#   bias rows    every path sums the fp32 accumulators (after the scale, BEFORE the bf16 rounding) over a (sample,
#                head)'s rows - DPP row sums + per-wave LDS rows (attention3 / attention5 BM = 1, 3), fp32 atomics
#                (attention_dh) - and ops.attn_bwd sums the per-sample rows (bv_colsum).  attention5 uses identities
#                where it can: v-bias = column sums of dO, k-bias = exactly 0, and for L % 16 != 0 (BM = 2) q-bias =
#                scale sum_key bf16(cs_key) K[key], cs_key = fp32 sum_q bf16(dS[q][key]).
#
# Headroom (worst max err / bound).  fp32 emulation of the documented arithmetic on the CPU
# (tests/test_tolerance_power_cpu.py, n = 2, H = 2, qkv seed 1 x 1.5, dO seed 2):
#   family (L, Dh)              dq    dk    dv    delta  dbias q / k / v    model / legacy tolerance, median (max)
#   attn3 dq+dkv (64, 64)       0.74  0.75  0.81  <0.01  0.18 0.17 0.19     0.024 (0.12)
#   attn5        (64, 64)       0.71  0.62  0.81  <0.01  0.15 0.13 0.19     0.035 (0.22)
#   attn3 dq+dkv (197, 64)      0.75  0.75  0.80  <0.01  0.10 0.11 0.20     0.023 (0.14)
#   attn5        (197, 64)      0.73  0.63  0.80  <0.01  0.07 0.15 0.20     0.037 (0.24)
#   attn3 dq+dkv (441, 64)      0.70  0.72  0.74  <0.01  0.09 0.09 0.15     0.021 (0.15)
#   dq1 + dkv32  (441, 64)      0.70  0.71  0.74  <0.01  0.06 0.08 0.15     0.021 (0.15)
#   adh          (100, 72)      0.79  0.77  0.84  <0.01  0.16 0.14 0.17     0.023 (0.14)
# The MI355X figures per kernel family are printed by every check ("[bounds] <case> [<family>] <part>: max err/bound")
# when the GPU files run with -s; they were not measured when this section was written (no GPU was available) and a
# value above 1 there is a failure to explain from the kernel source, not a number to absorb.
AttnBwd = collections.namedtuple("AttnBwd", "g g_bound delta delta_bound db db_bound path")
NO_LEGACY = (0.0, float("inf"))   # for outputs that no earlier assertion covered (delta)


def attn_bwd_path(L, Dh, masked, one_launch=True):
  """The kernel family ops.attn_bwd dispatches to: the mirror of csrc/attn_route.h (see the comment block above)."""
  if Dh != 64 or L > 576:
    return "adh"
  if masked:
    return "attn3 dq+dkv"
  if one_launch and (L <= 64 or 192 < L <= 208):
    return "attn5"
  return "attn3 dq1+dkv" if L <= 272 else "attn3 dq1+attn4 dkv32"


def _attn_bwd_chunk(qkv, d_o, m, L, H, Dh, lens, path):
  q, k, v = qkv.double().view(m, L, 3, H, Dh).unbind(2)
  do = d_o.double().view(m, L, H, Dh)
  sc = 1.0 / math.sqrt(Dh)
  o_ref, o_b, lse, lse_b = attn_fwd_bounds(qkv, m, L, H, Dh, lens)
  s = torch.einsum("nqhd,nkhd->nhqk", q, k) * sc
  es = torch.einsum("nqhd,nkhd->nhqk", q.abs(), k.abs()) * sc * gamma(Dh) * U   # fp32 accumulation of S over Dh
  if lens is not None:
    mask = torch.arange(L, device=s.device)[None, :] < torch.as_tensor(lens, device=s.device)[:, None]
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
  p = torch.exp(s - lse[..., None])
  sabs = s.abs().nan_to_num(0.0, posinf=0.0, neginf=0.0)
  # relative error of P: the S accumulation, the stored lse (within the forward's lse bound), the fp32 exponent
  # argument fma(S, c, -lse log2 e) and the hardware exp2
  rel_p = es + lse_b[..., None] + 8 * U * (sabs + lse.abs()[..., None] + 1)
  dp = torch.einsum("nqhd,nkhd->nhqk", do, v)
  e_dp = gamma(Dh) * U * torch.einsum("nqhd,nkhd->nhqk", do.abs(), v.abs())          # fp32 accumulation of dP over Dh
  delta = (p * dp).sum(-1)
  e_delta = (p * (e_dp + rel_p * dp.abs())).sum(-1)                                  # P and dP errors carried into the row sum
  e_delta = e_delta + (gamma(L) + 2) * U * (p * dp.abs()).sum(-1)                    # fp32 row sum over L (+ the product)
  epsb = 0.0
  if "dq1" in path:
    # dq1: |delta - delta~| <= sum_d |dO| |O_kernel - O| (the forward's o bound) + the fp32 dot product over Dh
    o_err = o_b.view(m, L, H, Dh) + gamma(Dh) * U * o_ref.abs().view(m, L, H, Dh)
    epsb = (do.abs() * o_err).sum(-1).permute(0, 2, 1)
    # dq1: the stored delta is rowsum(P o dP) + delta~ (1 - rowsum P); rowsum P is 1 only to the relative error of P
    e_delta = e_delta + (delta.abs() + epsb) * ((p * rel_p).sum(-1) + (gamma(L) + 4) * U)
    epsb = epsb[..., None]
  ds = p * (dp - delta[..., None])
  e_ds = p * (e_dp + e_delta[..., None]) + (rel_p + 2 * U) * ds.abs()                # dP, delta, P errors + the 2 fp32 ops
  # Operand roundings, exactly: one round-to-nearest-even of x to bf16 is off by at most half a bf16 ulp AT x (between
  # 2^-9 |x| and 2^-8 |x|, by x's mantissa), the ulp taken at |x| + its own error as in bf16_bound.  A flat 2^-8 |x|
  # is up to twice that and lets a second rounding of dP or delta hide inside the bound.
  h_p = 0.5 * ulp_bf16(p * (1 + rel_p))                      # bf16(P)
  # dq1: bf16 rounding of dS~ = dS + (delta - delta~) P, and of the bf16 P of the eps correction term
  dsq = ds.abs() + epsb * p
  if path == "attn5":
    # attn5: dS = bf16(P) (dP - delta), then bf16(dS): the P rounding carried through the product + the dS rounding
    via_p = h_p * (dp - delta[..., None]).abs()
    a_k = via_p + 0.5 * ulp_bf16(ds.abs() + via_p + e_ds)
    a_q = a_k
  else:
    a_k = 0.5 * ulp_bf16(ds.abs() + e_ds)
    a_q = 0.5 * ulp_bf16(dsq + e_ds) + epsb * h_p            # (dq1: + eps times the rounding of the correction's bf16 P)
  a_v = h_p
  s_q = e_ds + gamma(L) * U * dsq                            # dS error + fp32 accumulation over L
  s_k = e_ds + gamma(L) * U * ds.abs()
  s_v = p * (rel_p + gamma(L) * U)                           # P error + fp32 accumulation over L
  dq = torch.einsum("nhqk,nkhd->nqhd", ds, k) * sc
  dk = torch.einsum("nhqk,nqhd->nkhd", ds, q) * sc
  dv = torch.einsum("nhqk,nqhd->nkhd", p, do)
  # + the scale multiply (and the rounding of 1 / sqrtf(Dh) itself for Dh != 64) on the fp32 accumulator
  e_sys = torch.stack([torch.einsum("nhqk,nkhd->nqhd", s_q, k.abs()) * sc + 2 * U * dq.abs(),
                       torch.einsum("nhqk,nqhd->nkhd", s_k, q.abs()) * sc + 2 * U * dk.abs(),
                       torch.einsum("nhqk,nqhd->nkhd", s_v, do.abs())], 2).reshape(m * L, 3 * H * Dh)
  e_rnd = torch.stack([torch.einsum("nhqk,nkhd->nqhd", a_q, k.abs()) * sc,
                       torch.einsum("nhqk,nqhd->nkhd", a_k, q.abs()) * sc,
                       torch.einsum("nhqk,nqhd->nkhd", a_v, do.abs())], 2).reshape(m * L, 3 * H * Dh)
  g = torch.stack([dq, dk, dv], 2).reshape(m * L, 3 * H * Dh)
  # Bias rows sum the fp32 accumulators of all rows.  Their systematic errors add up; the operand roundings are one
  # independent round-to-nearest-even per (query, key) element, so over the rows x L terms of a column they add in
  # quadrature (the module's probabilistic rule, LAM sqrt(sum of squares)) - the worst-case sum would exceed the
  # column sum of |g| itself.
  sys_db = e_sys.sum(0)
  var_db = torch.stack([torch.einsum("nhqk,nkhd->hd", a_q ** 2, k ** 2) * sc ** 2,
                        torch.einsum("nhqk,nqhd->hd", a_k ** 2, q ** 2) * sc ** 2,
                        torch.einsum("nhqk,nqhd->hd", a_v ** 2, do ** 2)]).reshape(-1)
  if path == "attn5" and L % 16:
    # attn5 BM = 2: cs_key is rounded to bf16 before the K contraction that yields the q-bias gradient
    cs = ds.sum(2)                                           # [m, H, L(key)]
    sys_db[:H * Dh] += (U_BF16 * sc * torch.einsum("nhk,nkhd->nhd", cs.abs(), k.abs())).sum(0).reshape(-1)
  return g, e_sys + e_rnd, delta, e_delta, sys_db, var_db


def attn_bwd_bounds(qkv, d_o, n, L, H, Dh, lens=None, path=None, chunk_elems=1 << 22):
  """Self-attention backward on the bf16 qkv [n L, 3 H Dh] and dO [n L, H Dh], fp64: AttnBwd(g, g_bound [n L, 3 H Dh]
  (dq | dk | dv, bf16 outputs), delta, delta_bound [n, H, L] (fp32), db, db_bound [3 H Dh] (fp32 column sums of g,
  bound without the caller's initial value), path).  path (attn_bwd_path) selects the documented variant terms; the
  model runs over blocks of samples so that no [n, H, L, L] tensor exceeds chunk_elems."""
  if path is None:
    path = attn_bwd_path(L, Dh, lens is not None)
  step = max(1, chunk_elems // (H * L * L))
  gs, es, ds_, eds, edb, vdb = [], [], [], [], 0.0, 0.0
  for i0 in range(0, n, step):
    i1 = min(n, i0 + step)
    g, e, d, ed, eb, vb = _attn_bwd_chunk(qkv[i0 * L:i1 * L], d_o[i0 * L:i1 * L], i1 - i0, L, H, Dh,
                                      None if lens is None else list(lens[i0:i1]), path)
    gs.append(g); es.append(bf16_bound(g, e)); ds_.append(d); eds.append(f32_bound(d, ed)); edb = edb + eb; vdb = vdb + vb
  g = torch.cat(gs)
  db = g.sum(0)
  # + the fp32 summation over the n L rows (row sums, per-wave rows, per-sample rows, bv_colsum)
  edb = edb + LAM * torch.sqrt(vdb) + gamma(n * L) * U * g.abs().sum(0)
  return AttnBwd(g, torch.cat(es), torch.cat(ds_), torch.cat(eds), db, edb, path)


def capped_share(ref, bound, legacy):
  """Share of the elements on which the legacy tolerance, not the model, is the bound."""
  return (~(bound.double() <= legacy[1] + legacy[0] * ref.double().abs())).double().mean().item()


# --------------------------------------------------------- MAP attention ----
# attention.hip map_attn_* (Dh = 64) and attention_dh.hip adh_map_*: one wave per (sample, head), everything fp32 on
# the VALU (no bf16 operand): s = (q . k) scale accumulated over Dh, p = exp(s - max) / sum (stored fp32; keys >=
# kv_len get p = 0 exactly), o = bf16(sum_l p v) accumulated over L; backward from the STORED p: dp = dO . v over
# Dh, dsum = sum_l p dp (wave sum), ds = p (dp - dsum), dv = bf16(p dO), dk = bf16(ds (q scale)), dq = bf16(scale
# sum_l ds k).
MapAttn = collections.namedtuple("MapAttn", "p p_bound o o_bound dq dq_bound dkv dkv_bound")


def _map_core(q, kv, n, L, H, Dh, lens):
  qd = q.double().view(n, H, Dh)
  k, v = kv.double().view(n, L, 2, H, Dh).unbind(2)
  sc = 1.0 / math.sqrt(Dh)
  s = torch.einsum("nhd,nkhd->nhk", qd, k) * sc
  es = torch.einsum("nhd,nkhd->nhk", qd.abs(), k.abs()) * sc * gamma(Dh) * U          # fp32 accumulation of s over Dh
  if lens is not None:
    ln = torch.as_tensor(lens, device=s.device).long().clamp(1, L)
    s = s.masked_fill(~(torch.arange(L, device=s.device)[None, :] < ln[:, None])[:, None, :], float("-inf"))
  p = torch.softmax(s, -1)
  sabs = s.abs().nan_to_num(0.0, posinf=0.0, neginf=0.0)
  t = es + 8 * U * (sabs + s.amax(-1, keepdim=True).abs() + 1)    # s error, the fp32 exponent argument, the exp
  t = torch.where(p > 0, t, torch.zeros_like(t))
  # p = e / sum e: the element's own error, the sum's (at most the row maximum, + the wave sum over L), the divide
  rel_p = t + t.amax(-1, keepdim=True) + (gamma(L) + 4) * U
  return qd, k, v, sc, p, rel_p


def map_attn_fwd_bounds(q, kv, n, L, H, Dh, lens=None):
  """(p_ref [n, H, L], p bound (fp32 output), o_ref [n, H Dh], o bound (bf16 output)), fp64."""
  qd, k, v, sc, p, rel_p = _map_core(q, kv, n, L, H, Dh, lens)
  o = torch.einsum("nhk,nkhd->nhd", p, v)
  e_o = torch.einsum("nhk,nkhd->nhd", p * (rel_p + gamma(L) * U), v.abs())            # p error + fp32 accumulation over L
  return p, f32_bound(p, rel_p * p), o.reshape(n, H * Dh), bf16_bound(o, e_o).reshape(n, H * Dh)


def map_attn_bwd_bounds(q, kv, d_o, n, L, H, Dh, lens=None):
  """(dq_ref [n, H Dh], dq bound, dkv_ref [n L, 2 H Dh], dkv bound), bf16 outputs, fp64; the kernel's p is the
  forward's stored one, within map_attn_fwd_bounds' p bound of the exact softmax the reference uses."""
  qd, k, v, sc, p, rel_p = _map_core(q, kv, n, L, H, Dh, lens)
  do = d_o.double().view(n, H, Dh)
  rel_p = rel_p + F32_ULPS * U                                                        # the stored fp32 p
  dp = torch.einsum("nhd,nkhd->nhk", do, v)
  e_dp = gamma(Dh) * U * torch.einsum("nhd,nkhd->nhk", do.abs(), v.abs())             # fp32 accumulation of dp over Dh
  dsum = (p * dp).sum(-1, keepdim=True)
  e_dsum = (p * (e_dp + rel_p * dp.abs())).sum(-1, keepdim=True)                      # p and dp errors in the row sum
  e_dsum = e_dsum + (gamma(L) + 2) * U * (p * dp.abs()).sum(-1, keepdim=True)         # fp32 (wave) sum over L
  ds = p * (dp - dsum)
  e_ds = p * (e_dp + e_dsum) + (rel_p + 2 * U) * ds.abs()                             # dp, dsum, p errors + the 2 fp32 ops
  dq = torch.einsum("nhk,nkhd->nhd", ds, k) * sc
  # ds error + fp32 accumulation over L + the scale multiply
  e_dq = torch.einsum("nhk,nkhd->nhd", e_ds + gamma(L) * U * ds.abs(), k.abs()) * sc + 2 * U * dq.abs()
  dk = ds.permute(0, 2, 1)[..., None] * qd[:, None] * sc
  e_dk = e_ds.permute(0, 2, 1)[..., None] * qd.abs()[:, None] * sc + 4 * U * dk.abs() # ds error + (q scale), product
  dv = p.permute(0, 2, 1)[..., None] * do[:, None]
  e_dv = (rel_p.permute(0, 2, 1)[..., None] + 2 * U) * dv.abs()                       # p error + the product
  dkv = torch.stack([dk, dv], 2).reshape(n * L, 2 * H * Dh)
  e_dkv = torch.stack([e_dk, e_dv], 2).reshape(n * L, 2 * H * Dh)
  return dq.reshape(n, H * Dh), bf16_bound(dq, e_dq).reshape(n, H * Dh), dkv, bf16_bound(dkv, e_dkv)



# -------------------------------------------------------------- optimizer ----
# loss_optim.hip opt_chain (bv_adam_step, bv_trace_step) and adafactor.hip (bv_adafactor_leaf, bv_adafactor_step), per
# element, every operation fp32 (the compiler may contract a multiply-add into one fma: one rounding fewer, never more):
#   clip    gn = (float) sqrt(gsq) (fp64 sqrt, one rounding to fp32); clip = gn > clip_norm ? clip_norm / gn : 1, so
#           gn == clip_norm is the NO-clip side; g' = g clip                          (loss_optim.hip:416-420, 445)
#   adam    m' = b1 m + (1 - b1) g'; v' = b2 v + ((1 - b2) g') g'; u = (m' / bc1) / (sqrtf(v' / bc2) + eps): eps
#           OUTSIDE the root, after the bc2 division; u from the UNROUNDED m'          (loss_optim.hip:451-453)
#   trace   t' = g' + beta t; u = nesterov ? g' + beta t' (the unrounded t') : t'     (loss_optim.hip:456-457)
#   tail    d = (lr_eff u + wd_eff p) sched; p' = p - d; m' / t' stored fp32 or as ONE round-to-nearest-even to bf16;
#           shadow = rne(p'); stats += sum p'^2, sum d^2: fp32 over a thread's 4 elements, then fp64
#                                                                                     (loss_optim.hip:461-496)
#   adafactor  x = g clip; v_row' = d v_row + (1 - d) (sum_C (x^2 + eps) / C); v_col' likewise over R; rcm = sum_R
#           v_row' / R; u = (x rsqrtf(v_row' / rcm)) rsqrtf(v_col'), or u = x rsqrtf(v'), v' = d v + (1 - d)(x^2 + eps);
#           [u *= 1 / fmaxf(1, sqrtf((float)(usq / total)) / threshold), usq = sum u^2 over the whole LEAF]; m' =
#           mom m + (1 - mom) u (stored by RNE, used unrounded); upd = -sched (lr_eff m' + wd p); p' = p + upd
#                                                                                     (adafactor.hip:53-58, 73-86, 111-139, 274-318)
# Errors are propagated as ABSOLUTE errors (b1 m + (1 - b1) g cancels).  One fp32 rounding of x is charged U |x|.
# Device sqrtf, `/` and rsqrtf are charged DEV_ULPS = 2 ulps per call: no accuracy table of the device math library is
# installed with the toolchain, so this is the fallback constant of the issue, not a figure fitted to any kernel
# output (hipcc's default is a correctly rounded `/` and sqrtf and a 1-ulp rsqrtf).  The fp64 sqrt of the clip is taken
# as correctly rounded.
DEV_ULPS = 2
Out = collections.namedtuple("Out", "ref bound lo_hi")
_TINY = 2.0 ** -150


def _rd(x):
  """One fp32 rounding of a value of magnitude |x| (half an ulp <= U |x|)."""
  return U * x.abs() + _TINY


def _dv(x):
  """One device sqrtf / divide / rsqrtf result of magnitude |x|: DEV_ULPS ulps (ulp <= 2 U |x|)."""
  return DEV_ULPS * 2 * U * x.abs() + _TINY


def f32s(x):
  """A python scalar as the C ABI receives it (float)."""
  return float(np.float32(x))


def clip_factor(gsq, clip_norm):
  """(clip, e_clip) of the global-norm clip exactly as the kernels branch: clip_norm / float32(sqrt(gsq)) only when
  float32(sqrt(gsq)) > clip_norm, else exactly 1 with no error."""
  cn = np.float32(clip_norm or 0.0)
  if not cn > 0:
    return 1.0, 0.0
  gn = np.float32(np.sqrt(np.float64(gsq)))
  if not gn > cn:
    return 1.0, 0.0
  c = float(cn / gn)
  return c, DEV_ULPS * 2 * U * c


def _t(x, like):
  return torch.as_tensor(x, dtype=F64, device=like.device) if not torch.is_tensor(x) else x.double().to(like.device)


def _scaled_grad(g, clip, e_clip):
  g = g.double()
  if clip == 1.0 and e_clip == 0.0:
    return g, torch.zeros_like(g)          # g * 1.f is exact
  gc = g * clip
  return gc, g.abs() * e_clip + _rd(gc)


def _apply(p, u, e_u, lr, wd, sched):
  """d = (lr u + wd p) sched, p' = p - d: (p', e_p, d, e_d)."""
  lr, wd, sched = _t(lr, p), _t(wd, p), _t(sched, p)
  a = lr * u
  e_a = lr.abs() * e_u + _rd(a)
  b = wd * p
  c = a + b
  e_c = e_a + _rd(b)
  e_c = e_c + _rd(c.abs() + e_c)
  d = sched * c
  e_d = sched.abs() * e_c
  e_d = e_d + _rd(d.abs() + e_d)
  pn = p - d
  e_p = e_d + _rd(pn.abs() + e_d)
  return pn, e_p, d, e_d


def _sumsq(x, e, K):
  """sum x^2 of values within e of x, fp32 partial sums of K non-negative terms, then fp64: (ref, bound)."""
  ref = (x * x).sum()
  return ref, (2 * x.abs() * e + e * e).sum() + (gamma(K) + 2) * U * ref + 1e-13 * ref + 1e-300


def _store(ref, e, bf16):
  """A stored accumulator: fp32 -> bound e; bf16 -> one RNE of a value within e of ref: bound 0.5 ulp + e and the
  interval [rne(ref - e), rne(ref + e)] (almost everywhere one bf16 number)."""
  if not bf16:
    return Out(ref, e, None)
  return Out(ref, bf16_bound(ref, e), (rne_bf16(ref - e), rne_bf16(ref + e)))


def _sqrt_err(v, e):
  """|sqrt(v~) - sqrt(v)| for |v~ - v| <= e, v >= 0 (sqrt is not Lipschitz at 0)."""
  s = v.sqrt()
  return torch.maximum((v + e).sqrt() - s, s - (v - e).clamp_min(0).sqrt())


def adam_bounds(p, g, mu, nu, lr_eff, wd_eff, sched, gsq, clip_norm, b1, b2, eps, bc1, bc2):
  """OPT_ADAM on the stored inputs (fp32 p, g, nu; mu fp32 or bf16; lr_eff / wd_eff / sched scalars or per-element
  tensors of the fp32 values the kernel reads; fp64 gsq).  Returns {"mu", "nu", "p": Out, "stats": (ref[2], bound[2])}."""
  clip, e_clip = clip_factor(gsq, clip_norm)
  mu_bf16 = mu.dtype == BF16
  p, m, v = p.double(), mu.double(), nu.double()
  b1, b2, eps, bc1, bc2 = (f32s(x) for x in (b1, b2, eps, bc1, bc2))
  ob1 = float(np.float32(1) - np.float32(b1)); ob2 = float(np.float32(1) - np.float32(b2))
  gc, e_g = _scaled_grad(g, clip, e_clip)
  t1, t2 = b1 * m, ob1 * gc
  mn = t1 + t2
  e_m = _rd(t1) + ob1 * e_g + _rd(t2)
  e_m = e_m + _rd(mn.abs() + e_m)
  s1 = ob2 * gc
  s2 = s1 * gc
  t3 = b2 * v
  vn = t3 + s2
  e_v = _rd(t3) + 2 * ob2 * gc.abs() * e_g + ob2 * e_g * e_g + _rd(s1) * gc.abs() + _rd(s2)
  e_v = e_v + _rd(vn + e_v)
  mh = mn / bc1
  e_mh = e_m / bc1 + _dv(mh)
  vh = vn / bc2
  e_vh = e_v / bc2 + _dv(vh)
  sq = vh.sqrt()
  e_sq = _sqrt_err(vh, e_vh) + _dv(sq)
  den = sq + eps
  e_den = e_sq + _rd(den)
  den_lo = (den - e_den).clamp_min(_TINY)
  u = mh / den
  e_u = e_mh / den_lo + mh.abs() * e_den / (den * den_lo) + _dv(u.abs() + e_mh / den_lo)
  pn, e_p, d, e_d = _apply(p, u, e_u, lr_eff, wd_eff, sched)
  sp, bp = _sumsq(pn, e_p, 4)
  su, bu = _sumsq(d, e_d, 4)
  return {"mu": _store(mn, e_m, mu_bf16), "nu": Out(vn, e_v, None), "p": Out(pn, e_p, None),
          "stats": (torch.stack([sp, su]), torch.stack([bp, bu]))}


def trace_bounds(p, g, trace, lr_eff, wd_eff, sched, gsq, clip_norm, beta, nesterov):
  """OPT_TRACE (trace: the stored bf16 / fp32 accumulator) or OPT_IDENTITY (trace None): {"trace" (absent for
  identity), "p": Out, "stats"}."""
  clip, e_clip = clip_factor(gsq, clip_norm)
  p = p.double()
  gc, e_g = _scaled_grad(g, clip, e_clip)
  out = {}
  if trace is None:
    u, e_u = gc, e_g
  else:
    beta = f32s(beta)
    bt = beta * trace.double()
    tn = gc + bt
    e_t = e_g + _rd(bt)
    e_t = e_t + _rd(tn.abs() + e_t)
    out["trace"] = _store(tn, e_t, trace.dtype == BF16)
    if nesterov:
      bn = beta * tn
      u = gc + bn
      e_u = e_g + abs(beta) * e_t + _rd(bn)
      e_u = e_u + _rd(u.abs() + e_u)
    else:
      u, e_u = tn, e_t
  pn, e_p, d, e_d = _apply(p, u, e_u, lr_eff, wd_eff, sched)
  sp, bp = _sumsq(pn, e_p, 4)
  su, bu = _sumsq(d, e_d, 4)
  out["p"] = Out(pn, e_p, None)
  out["stats"] = (torch.stack([sp, su]), torch.stack([bp, bu]))
  return out


def sqnorm_bound(x):
  """bv_sqnorm: float4 loads, 4 squares added per iteration into an fp32 per-thread partial over the grid-stride
  range ((count / 4) / (256 x 2048 workgroups) iterations), the scalar tail on workgroup 0, an 8-add workgroup tree,
  fp64 atomics: (ref, bound) - an fp32 sum of non-negative terms of the per-thread length."""
  n = x.numel()
  n4 = n // 4
  grid = min(max((n4 + 255) // 256, 1), 2048)
  K = 4 * (-(-n4 // (256 * grid))) + 1 + 8          # per-thread terms (+ its tail element) + the tree
  ref = (x.double() ** 2).sum()
  return ref, (gamma(K) + 1) * U * ref + 1e-13 * ref + 1e-300


def _rsqrt_err(q, e_q):
  r = q.rsqrt()
  return (q - e_q).clamp_min(_TINY).rsqrt() - r + _dv(r)


def _af_stats_K(total, cap):
  grid = min(-(-total // 1024), cap)
  return -(-total // (256 * grid)) + 8


def adafactor_bounds(p, g, mom, state, factored, gsq, clip_norm, decay, eps, momentum, lr_eff, wd, sched,
                     block_rms_clip=0.0, grid_cap=2048):
  """One Adafactor leaf.  p, g, mom: the leaf's [B1][B2][R][C] views of the buffers as stored before the step (mom
  bf16 or fp32); state: its fp32 statistics before the step (factored: v_row [B R], v_col [B C], rcm [B]; else v
  [B R C] in the view's order).  Returns {"v_row", "v_col", "rcm" | "v", "mom", "p": Out, "stats": (ref[2], bound[2]),
  and with block_rms_clip > 0 "usq": (ref, bound), "scale": (ref, bound)}, the tensors in the view's [B1][B2][R][C]
  shape ([B, R] / [B, C] / [B] for the factored statistics)."""
  clip, e_clip = clip_factor(gsq, clip_norm)
  B1, B2, R, C = p.shape
  Bn = B1 * B2
  total = Bn * R * C
  decay, eps, momentum = f32s(decay), f32s(eps), f32s(momentum)
  od = float(np.float32(1) - np.float32(decay)); om = float(np.float32(1) - np.float32(momentum))
  x, e_x = _scaled_grad(g.reshape(Bn, R, C), clip, e_clip)
  pd = p.double().reshape(Bn, R, C)
  st = state.double()
  out = {}
  sqe = x * x + eps                                  # each term: the square, the + eps
  e_sqe = 2 * x.abs() * e_x + e_x * e_x + 2 * U * sqe

  def ema(old, s, e_s, K, n):
    s_e = e_s + gamma(K) * U * s                     # K-term fp32 sum of non-negative terms
    mean = s / n
    e_mean = s_e / n + _dv(mean)
    t1, t2 = decay * old, od * mean
    new = t1 + t2
    e = _rd(t1) + od * e_mean + _rd(t2)
    return new, e + _rd(new + e)

  if factored:
    v_row, v_col = st[:Bn * R].view(Bn, R), st[Bn * R:Bn * R + Bn * C].view(Bn, C)
    vr, e_vr = ema(v_row, sqe.sum(2), e_sqe.sum(2), C, C)
    vc, e_vc = ema(v_col, sqe.sum(1), e_sqe.sum(1), R, R)
    rs = vr.sum(1)
    rcm = rs / R
    e_rcm = (e_vr.sum(1) + gamma(R) * U * rs) / R + _dv(rcm)
    out["v_row"], out["v_col"], out["rcm"] = Out(vr, e_vr, None), Out(vc, e_vc, None), Out(rcm, e_rcm, None)
    rcm_lo = (rcm - e_rcm).clamp_min(_TINY)
    q = vr / rcm[:, None]
    e_q = e_vr / rcm_lo[:, None] + vr * (e_rcm / (rcm * rcm_lo))[:, None] + _dv(q)
    rf, e_rf = q.rsqrt(), _rsqrt_err(q, e_q)
    cf, e_cf = vc.rsqrt(), _rsqrt_err(vc, e_vc)
    xr = x * rf[:, :, None]
    e_xr = e_x * rf[:, :, None] + (x.abs() + e_x) * e_rf[:, :, None] + _rd(xr)
    u = xr * cf[:, None, :]
    e_u = e_xr * cf[:, None, :] + (xr.abs() + e_xr) * e_cf[:, None, :]
    e_u = e_u + _rd(u.abs() + e_u)
  else:
    v = st[:total].view(Bn, R, C)
    t1, t2 = decay * v, od * sqe
    nv = t1 + t2
    e_nv = _rd(t1) + od * e_sqe + _rd(t2)
    e_nv = e_nv + _rd(nv + e_nv)
    out["v"] = Out(nv.view(B1, B2, R, C), e_nv.view(B1, B2, R, C), None)
    rq, e_rq = nv.rsqrt(), _rsqrt_err(nv, e_nv)
    u = x * rq
    e_u = e_x * rq + (x.abs() + e_x) * e_rq
    e_u = e_u + _rd(u.abs() + e_u)
  if block_rms_clip and block_rms_clip > 0:
    thr = f32s(block_rms_clip)
    usq, e_usq = _sumsq(u, e_u, _af_stats_K(total, 1024))
    out["usq"] = (usq, e_usq)
    def scale_of(s, sign):                           # monotone decreasing in s; sign: -1 lower / +1 upper end
      rms = (s.clamp_min(0) / total).sqrt()
      ratio = rms / thr * (1 - sign * (2 * DEV_ULPS * 2 + 1) * U)       # float(), sqrtf, the divide
      return torch.where(ratio > 1, (1 / ratio) * (1 + sign * DEV_ULPS * 2 * U), torch.ones_like(ratio))
    rms32 = np.float32(np.sqrt(np.float32(usq.item() / total)))
    ratio32 = rms32 / np.float32(thr)
    bs = float(np.float32(1) / max(np.float32(1), ratio32))
    lo, hi = scale_of(usq + e_usq, -1).item(), scale_of(usq - e_usq, +1).item()
    e_bs = max(hi - bs, bs - lo, 0.0)
    out["scale"] = (bs, e_bs)
    e_u = e_u * bs + (u.abs() + e_u) * e_bs
    u = u * bs
    if bs != 1.0 or e_bs != 0.0:
      e_u = e_u + _rd(u.abs() + e_u)
  if momentum > 0:
    m = mom.double().reshape(Bn, R, C)
    t1, t2 = momentum * m, om * u
    mn = t1 + t2
    e_m = _rd(t1) + om * e_u + _rd(t2)
    e_m = e_m + _rd(mn.abs() + e_m)
    o = _store(mn, e_m, mom.dtype == BF16)
    out["mom"] = Out(o.ref.view(B1, B2, R, C), o.bound.view(B1, B2, R, C),
                     None if o.lo_hi is None else tuple(t.view(B1, B2, R, C) for t in o.lo_hi))
    u, e_u = mn, e_m
  pn, e_p, d, e_d = _apply(pd, u, e_u, lr_eff, wd, sched)
  out["p"] = Out(pn.view(B1, B2, R, C), e_p.view(B1, B2, R, C), None)
  K = _af_stats_K(total, grid_cap)
  sp, bp = _sumsq(pn, e_p, K)
  su, bu = _sumsq(d, e_d, K)
  out["stats"] = (torch.stack([sp, su]), torch.stack([bp, bu]))
  return out


def check_out(out, o, name, legacy=NO_LEGACY):
  """A kernel output against an Out of the optimizer models; a bf16 store is held to its bound AND to the interval
  of bf16 numbers the one round-to-nearest-even can give.  Returns max err / bound."""
  w = check(out, o.ref, o.bound, legacy, name)
  if o.lo_hi is not None:
    check(out, o.ref, torch.zeros_like(o.ref), legacy, name + " (RNE interval)", lo_hi=o.lo_hi, report=False)
  return w


def check_stats(stats, ref, bound, name):
  """The two fp64 statistics (sum p'^2, sum update^2) against the models' (ref, bound)."""
  return check(stats.double(), ref, bound, NO_LEGACY, name)


# ------------------------------------------------- checkers of the GPU tests ----
def check_gemm(out, ref, a, b_t, legacy, name, n_adds=1, alpha=1.0):
  """GEMM output (bf16 or fp32 by out's dtype) of A [M][K] @ B^T [K][N] (+ n_adds fp32 epilogue adds) vs the fp64 ref."""
  K = a.shape[1]
  ap = absprod(a, b_t) * abs(alpha)
  bnd = gemm_bf16(ref, ap, K, n_adds) if out.dtype == BF16 else gemm_f32(ref, ap, K, n_adds)
  return check(out, ref, bnd, legacy, name)


def check_gelu_g(g, h, legacy, name):
  """g (bf16) against gelu_tanh of the pre-activation h as the kernel stored it."""
  ref, bnd = gelu_g(h)
  return check(g, ref, bnd, legacy, name)


def check_gelu_dg(d, h, legacy, name):
  ref, bnd = gelu_dg(h)
  return check(d, ref, bnd, legacy, name)


def check_gelu_bwd(out, a, b_t, h, legacy, name, legacy_ref=None):
  """dX = bf16(A B^T o bf16(gelu'(h))); the legacy assertion is made against legacy_ref (default: the exact product
  with the exact gelu'(h))."""
  prod = a.double() @ b_t.double()
  lo_hi, bnd = gelu_bwd(prod, absprod(a, b_t), a.shape[1], h)
  ref = prod * dgelu_tanh64(h) if legacy_ref is None else legacy_ref
  return check(out, ref, bnd, legacy, name, lo_hi=lo_hi)


def check_mul(out, a, b_t, d, legacy, name):
  ref, bnd = mul_bwd(a.double() @ b_t.double(), absprod(a, b_t), a.shape[1], d)
  return check(out, ref, bnd, legacy, name)


def check_ln_fwd(y, x, scale, bias, legacy, name):
  ref, bf, bb = ln_fwd_bounds(x, scale, bias)
  return check(y, ref, bb if y.dtype == BF16 else bf, legacy, name)


def check_ln_bwd(dx, x, scale, dy, legacy, name, dres=None):
  ref, bf, bb = ln_bwd_bounds(x, scale, dy, dres)
  return check(dx, ref, bb if dx.dtype == BF16 else bf, legacy, name)


def check_attn_fwd(o, lse, qkv, n, L, H, Dh, lens=None, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3), name="attn"):
  o_ref, ob, lse_ref, lb = attn_fwd_bounds(qkv, n, L, H, Dh, lens)
  check(lse, lse_ref, lb, legacy_lse, name + " lse")
  check(o, o_ref, ob, legacy_o, name + " out")


def check_attn_bwd(dqkv, qkv, d_o, n, L, H, Dh, lens=None, legacy=3e-2, delta=None, dbias=None, dbias_base=0.0,
                   legacy_db=2e-2, path=None, name="attn bwd", bounds=None):
  """Self-attention backward outputs against attn_bwd_bounds.  legacy / legacy_db: the flat tolerances these
  assertions had before, r meaning (rtol, atol) = (r, r max|ref|) with the maximum over the whole tensor (dqkv) /
  over the column sums of |g| (dbias) - they cap the model bound.
  delta: the buffer the backward entry point filled ([n, H, L] fp32), compared with fp64 rowsum(P o dP).  The "attn5"
  path (attention5.hip, the one-launch backward) keeps its delta partials in LDS and does NOT fill the buffer: there,
  and only there, a delta that is passed is not looked at.
  dbias: the fp32 bias-gradient vector after the launch (dbias_base + column sums); the k-bias third is 0 in exact
  arithmetic (the rows of dS sum to 0), so its bound is the model's alone - the legacy cap is far above it.
  Returns {part: max err / bound}."""
  b = attn_bwd_bounds(qkv, d_o, n, L, H, Dh, lens, path) if bounds is None else bounds
  tag = f"{name} [{b.path}]"
  leg = (legacy, legacy * b.g.abs().max().item())
  out = {}
  w = H * Dh
  for j, part in enumerate(("dq", "dk", "dv")):
    sl = slice(j * w, (j + 1) * w)
    out[part] = check(dqkv[:, sl], b.g[:, sl], b.g_bound[:, sl], leg, f"{tag} {part}")
  if delta is not None and b.path != "attn5":
    out["delta"] = check(delta, b.delta, b.delta_bound, NO_LEGACY, f"{tag} delta")
  if dbias is not None:
    ref = dbias_base + b.db
    bnd = f32_bound(ref, b.db_bound + 2 * U * (abs(dbias_base) + b.db.abs()), F32_ULPS)   # + the add onto the base
    leg_db = (legacy_db, legacy_db * b.g.abs().sum(0).max().item())
    for j, part in enumerate(("dbias q", "dbias k", "dbias v")):
      sl = slice(j * w, (j + 1) * w)
      out[part] = check(dbias[sl], ref[sl], bnd[sl], leg_db, f"{tag} {part}")
  return out


def check_map_attn_fwd(o, p, q, kv, n, L, H, Dh, lens=None, legacy_p=(1e-3, 1e-5), legacy_o=(1e-2, 1e-2),
                       name="map attn"):
  tag = f"{name} [{'map' if Dh == 64 and L <= 2048 else 'map-dh'}]"
  p_ref, pb, o_ref, ob = map_attn_fwd_bounds(q, kv, n, L, H, Dh, lens)
  check(p, p_ref, pb, legacy_p, f"{tag} p")
  check(o, o_ref, ob, legacy_o, f"{tag} o")


def check_map_attn_bwd(dq, dkv, q, kv, d_o, n, L, H, Dh, lens=None, legacy=2e-2, name="map attn"):
  """legacy: the flat tolerance r of the earlier assertions, (r, r max|ref|) per output tensor."""
  tag = f"{name} [{'map' if Dh == 64 and L <= 2048 else 'map-dh'}]"
  dq_ref, dqb, dkv_ref, dkvb = map_attn_bwd_bounds(q, kv, d_o, n, L, H, Dh, lens)
  check(dq, dq_ref, dqb, (legacy, legacy * dq_ref.abs().max().item()), f"{tag} dq")
  leg = (legacy, legacy * dkv_ref.abs().max().item())
  w = H * Dh
  check(dkv[:, :w], dkv_ref[:, :w], dkvb[:, :w], leg, f"{tag} dk")
  check(dkv[:, w:], dkv_ref[:, w:], dkvb[:, w:], leg, f"{tag} dv")


def check_ln_edge_launch(ops, x, scale, bias, dys, dres=None, strided=None, idx=LN_EDGE_IDX, name="ln edge rows"):
  """LayerNorm edge rows (ln_edge_rows) in launches of their own, at x's rows x D and dtype (the same kernel
  instantiation as the test's main launch), forward and backward against the model bounds.  These launches request
  no fused column sums: a row of std 1e-3 has rstd ~ 700 and a dx of that order, which would make the atomically
  summed dx_colsum / dscale / dbias depend on the order of the workgroups' atomics at the level of their tolerance;
  the column sums stay checked on the main launch's inputs, which hold no edge rows.  rows = 1 runs each of the three
  kinds as row 0.  idx: the rows that become edge rows; strided: (n, L, offset) for an extra strided-row launch (rows
  offset, offset + L, ... of the same edge-row x)."""
  rows, D = x.shape
  for k in ((0,) if rows > 1 else (0, 1, 2)):
    xe = x.float().clone()
    ln_edge_rows(xe, idx if rows > 1 else (0,), first_kind=k)
    xe = xe.to(x.dtype)
    tag = f"{name}, kind {k}" if rows == 1 else name
    y_bf, y_f, mean, rstd = ops.layernorm_fwd(xe, scale, bias, rows=rows, D=D, want_f32=True)
    check_ln_fwd(y_f, xe, scale, bias, legacy=(1e-5, 1e-5), name=f"{tag}: fwd f32")
    check_ln_fwd(y_bf, xe, scale, bias, legacy=(1e-2, 1e-2), name=f"{tag}: fwd bf16")
    for dy in dys:
      t2 = f"{tag} (dy {dy.dtype}, dres {dres is not None})"
      if x.dtype == F32:
        dx_bf = torch.empty((rows, D), device=x.device, dtype=BF16)
        dx = ops.layernorm_bwd(dy, xe, scale, mean, rstd, rows=rows, D=D, dres=dres, dx_bf16=dx_bf)
        check_ln_bwd(dx, xe, scale, dy, dres=dres, legacy=(1e-4, 1e-4), name=f"{t2}: dx")
        check_ln_bwd(dx_bf, xe, scale, dy, dres=dres, legacy=(1e-2, 1e-2), name=f"{t2}: dx bf16")
      else:
        dx = ops.layernorm_bwd(dy, xe, scale, mean, rstd, rows=rows, D=D, dres=dres)
        check_ln_bwd(dx, xe, scale, dy, dres=dres, legacy=(1e-2, 1e-2), name=f"{t2}: dx (bf16 stream)")
    if strided is not None:
      n, L, off = strided
      _, y, m_s, r_s = ops.layernorm_fwd(xe, scale, bias, rows=n, D=D, row_stride=L, row_offset=off, want_bf16=False,
                                         want_f32=True)
      sel = xe[:n * L].view(n, L, D)[:, off]
      check_ln_fwd(y, sel, scale, bias, legacy=(1e-5, 1e-5), name=f"{tag}: strided fwd")
      dys_ = rnd((n, D), x.device, 6)
      dxs = ops.layernorm_bwd(dys_, xe[:n * L].contiguous(), scale, m_s, r_s, rows=n, D=D, row_stride=L,
                              row_offset=off)
      others = [i for i in range(L) if i != off]
      assert (dxs.view(n, L, D)[:, others] == 0).all(), f"{tag}: strided launch wrote other rows"
      leg = (1e-4, 1e-4) if x.dtype == F32 else (1e-2, 1e-2)
      check_ln_bwd(dxs.view(n, L, D)[:, off], sel, scale, dys_, legacy=leg, name=f"{tag}: strided bwd")


def _sl(x, a, b):
  return x[a:b] if torch.is_tensor(x) and x.dim() > 0 else x


def check_chain_step(kind, new, before, lr_eff, wd_eff, sched, gsq, clip_norm, hp, name, legacy=NO_LEGACY,
                     stats=None, chunk=1 << 20):
  """One step of the fused chain (kind "adam" | "trace") against adam_bounds / trace_bounds.  new: {"p", "mu" | "trace",
  "nu"} after the step; before: {"p", "g", "mu" | "trace", "nu"} as stored before it; lr_eff / wd_eff / sched: scalars
  or per-element fp32 tensors; hp: the remaining hyper-parameters of the model (b1, b2, eps, bc1, bc2 | beta,
  nesterov).  The model is evaluated in blocks of `chunk` elements.  legacy: {operand: (rtol, atol)} or one pair.
  Returns {operand: max err / bound}."""
  n = before["p"].numel()
  worst, sref, sbnd = {}, 0.0, 0.0
  for a in range(0, n, chunk):
    b = min(n, a + chunk)
    args = (_sl(lr_eff, a, b), _sl(wd_eff, a, b), _sl(sched, a, b), gsq, clip_norm)
    if kind == "adam":
      m = adam_bounds(before["p"][a:b], before["g"][a:b], before["mu"][a:b], before["nu"][a:b], *args, **hp)
    else:
      tr = before.get("trace")
      m = trace_bounds(before["p"][a:b], before["g"][a:b], None if tr is None else tr[a:b], *args, **hp)
    for k, o in m.items():
      if k == "stats":
        sref, sbnd = sref + o[0], sbnd + o[1]
        continue
      leg = legacy.get(k, NO_LEGACY) if isinstance(legacy, dict) else legacy
      leg = (leg[0], _sl(leg[1], a, b))          # (the atol may be a per-element tensor)
      tag = f"{name} {k}" + (f" [{a}:{b}]" if n > chunk else "")
      worst[k] = max(worst.get(k, 0.0), check_out(new[k][a:b], o, tag, leg))
  if stats is not None:
    worst["stats"] = check_stats(stats, sref, sbnd, f"{name} stats")
  return worst


def af_views(bufs, view):
  """The leaf's [B1][B2][R][C] views of flat buffers, view = (off, B1, B2, R, C, sB1, sB2, sR, sC)."""
  o, B1, B2, R, C, sB1, sB2, sR, sC = (int(x) for x in view)
  return [None if t is None else t.as_strided((B1, B2, R, C), (sB1, sB2, sR, sC), o) for t in bufs]


def check_af_leaf(new, before, view, factored, gsq, clip_norm, hp, name, legacy=NO_LEGACY, stats=None,
                  block_rms_clip=0.0, usq=None, grid_cap=2048, model=None):
  """One Adafactor leaf after a step against adafactor_bounds.  new / before: {"p", "g" (before), "mom", "state"}: flat
  buffers (p, g, mom) and the leaf's fp32 statistics slice; view: the 9 view numbers; hp: decay, eps, momentum,
  lr_eff, wd, sched.  Returns ({operand: max err / bound}, model)."""
  B1, B2, R, C = (int(x) for x in view[1:5])
  Bn = B1 * B2
  pv, gv, mv = af_views([before["p"], before["g"], before["mom"]], view)
  m = model or adafactor_bounds(pv, gv, mv, before["state"], factored, gsq, clip_norm, block_rms_clip=block_rms_clip,
                                grid_cap=grid_cap, **hp)
  pn, mn = af_views([new["p"], new["mom"]], view)
  st = new["state"]
  worst = {}
  if factored:
    parts = {"v_row": st[:Bn * R].view(Bn, R), "v_col": st[Bn * R:Bn * R + Bn * C].view(Bn, C),
             "rcm": st[Bn * R + Bn * C:Bn * R + Bn * C + Bn]}
  else:
    parts = {"v": st[:Bn * R * C].view(B1, B2, R, C)}
  parts["p"] = pn
  if "mom" in m:
    parts["mom"] = mn
  for k, t in parts.items():
    leg = legacy.get(k, NO_LEGACY) if isinstance(legacy, dict) else legacy
    worst[k] = check_out(t, m[k], f"{name} {k}", leg)
  if stats is not None:
    worst["stats"] = check_stats(stats, m["stats"][0], m["stats"][1], f"{name} stats")
  if usq is not None and "usq" in m:
    worst["usq"] = check(usq, m["usq"][0], m["usq"][1], NO_LEGACY, f"{name} usq")
  return worst, m


# ---- a whole optimizer object (big_vision_amd.optax.Chain / Adafactor on one rank): the step it just made, per
# element, from the buffers it held before the step
def snapshot_opt(opt):
  """The buffers an optimizer step reads and overwrites, cloned before the step (the gradient buffer is not cloned:
  the step leaves it as it is and may be filled after this call)."""
  st = opt.store
  n = st.trainable_count
  snap = dict(p=st.master[:n].clone(), mu=None if getattr(opt, "mu", None) is None else opt.mu.clone())
  if getattr(opt, "nu", None) is not None:
    snap["nu"] = opt.nu.clone()
  if getattr(opt, "af_state", None) is not None:
    snap["state"] = opt.af_state.clone()
  return snap


def _entry_atol(st, p_before, p_after, r):
  """The max-normalised legacy tolerance r max(1, max|p| of the store entry) as a per-element atol."""
  n = st.trainable_count
  atol = torch.full((n,), r, dtype=F64, device=p_before.device)
  for e in st.entries.values():
    if e.name not in st.frozen and e.offset + e.numel <= n:
      sl = slice(e.offset, e.offset + e.numel)
      atol[sl] = r * max(1.0, p_after[sl].abs().max().item())
  return atol


def check_opt_step(opt, snap, name, legacy_p=2e-6, legacy_state=2e-5, legacy_state_bf16=1e-2):
  """The step `opt` made since snapshot_opt, operand by operand and element by element, against the chain / Adafactor
  models evaluated on the snapshot, this step's gradient buffer, gsq and schedule values.  legacy_*: the
  max-normalised tolerances of the fixture assertions (r max(1, max|p|) per store entry or Adafactor leaf for the
  parameters, r max|state| for an accumulator), which cap the model bounds.  Returns {operand: max err / bound}."""
  st = opt.store
  n = st.trainable_count
  assert not opt.sharded
  k = opt.count - 1
  sched = [f32s(fn(k)) for fn in opt.schedule_fns]
  gsq, clip_norm = opt.gsq.item(), float(opt.clip_norm or 0.0)
  p, g = st.master[:n], st.grad[:n]
  acc_leg = lambda t: (0.0, (legacy_state_bf16 if t.dtype == BF16 else legacy_state) * max(1e-30, t.double().abs().max().item()))
  if opt.kind in ("adam", "trace", "identity"):
    cs = opt.chunk_seg.long()[:n // 1024]
    el = lambda col: col[cs].repeat_interleave(1024)
    lr_t, wd_t = el(opt.segs[:, 0]), el(opt.segs[:, 1])
    si = el(opt.segs[:, 2].contiguous().view(torch.int32)).long()
    sc_t = torch.tensor(sched + [0.0] * (8 - len(sched)), dtype=F32, device=p.device)[si]
    leg = {"p": (0.0, _entry_atol(st, snap["p"], p, legacy_p))}
    if opt.kind == "adam":
      before = dict(p=snap["p"], g=g, mu=snap["mu"][:n], nu=snap["nu"][:n])
      new = dict(p=p, mu=opt.mu[:n], nu=opt.nu[:n])
      hp = dict(b1=opt.b1, b2=opt.b2, eps=opt.eps, bc1=1.0 - opt.b1 ** (k + 1), bc2=1.0 - opt.b2 ** (k + 1))
      leg["mu"], leg["nu"] = acc_leg(new["mu"]), acc_leg(new["nu"])
    else:
      tr = None if opt.kind == "identity" else snap["mu"][:n]
      before = dict(p=snap["p"], g=g, trace=tr)
      new = dict(p=p, trace=None if tr is None else opt.mu[:n])
      hp = dict(beta=opt.momentum, nesterov=opt.nesterov)
      if tr is not None:
        leg["trace"] = acc_leg(new["trace"])
    return check_chain_step("adam" if opt.kind == "adam" else "trace", new, before, lr_t, wd_t, sc_t, gsq, clip_norm, hp,
                            name, legacy=leg, stats=opt.stats)
  af = opt.af
  t = float(k - af["decay_offset"]) + 1.0
  decay = min(af["beta2_cap"], 1.0 - t ** (-af["decay_rate"]))
  worst, sref, sbnd = {}, 0.0, 0.0
  for lf in opt.af_leaves:
    sl = slice(lf["soff"], lf["soff"] + lf["n_state"])
    hp = dict(decay=decay, eps=af["eps"], momentum=af["momentum"], lr_eff=lf["lr_eff"], wd=lf["wd"],
              sched=sched[lf["sched"]])
    pv = af_views([p], lf["view"])[0]
    leg = {"p": (0.0, legacy_p * max(1.0, pv.abs().max().item()))}
    if opt.mu is not None:
      leg["mom"] = acc_leg(af_views([opt.mu], lf["view"])[0])
    br, bc = lf["B"] * lf["R"], lf["B"] * lf["C"]
    for key, a, b in ((("v_row", 0, br), ("v_col", br, br + bc)) if lf["factored"] else (("v", 0, lf["n_state"]),)):
      leg[key] = acc_leg(opt.af_state[sl][a:b])
    w, m = check_af_leaf(dict(p=p, mom=opt.mu, state=opt.af_state[sl]),
                         dict(p=snap["p"], g=g, mom=snap["mu"], state=snap["state"][sl]), lf["view"], lf["factored"], gsq,
                         clip_norm, hp, f"{name} {lf['leaf']}", legacy=leg, block_rms_clip=af["block_rms_clip"],
                         grid_cap=1024)
    for kk, v in w.items():
      worst[kk] = max(worst.get(kk, 0.0), v)
    sref, sbnd = sref + m["stats"][0], sbnd + m["stats"][1]
  worst["stats"] = check_stats(opt.stats, sref, sbnd, f"{name} stats")
  return worst
