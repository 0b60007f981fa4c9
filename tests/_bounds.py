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
import math

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
