"""Proof, on the CPU, that the bounds of tests/_bounds.py bite: for every family of tightened GPU checks, the bound
ACCEPTS an emulation of the prescribed arithmetic (fp32 / bf16 steps as the kernels promise them, on the GPU tests'
own seeded inputs) and REJECTS every mutant of that family's catalogue - an emulation that makes one plausible slip.
Each (family, mutant) prints one line with the number of elements rejected (pytest -s).

Catalogue notes:
  * "gelu' rounded to bf16 before the product" is not a slip here: it is the contract of the fused GELU' backward
    (bv_common.h mlp_act_from_h, gemm256.hip: gelu' is rounded to bf16 as GELU_GD stores it, so every context kind
    feeds the backward the same bits - test_gemm256_gpu.py asserts MUL(GELU_GD's d) == GELU_BWD bit for bit).  The
    catalogue holds the opposite slip, an unrounded fp32 gelu', which the stage bound rejects.
  * The column-sum / dW / loss outputs keep their previous tolerances: the model does not justify a tighter bound for
    them.  Their mutants below are rejected by those tolerances.
  * The attention backward (dq / dk / dv, delta, the bias gradients; MAP p / o / dq / dkv) is held to the models of
    _bounds.py's attention-backward section.  Every slip is recorded twice: the elements the model rejects and the
    elements the earlier flat tolerance (3e-2 max|g|) alone would have rejected.  Truncation instead of
    round-to-nearest-even of the bf16 operands / outputs is recorded as not separable by an elementwise bound.
  * The attention P term is 2^-8 sum P|v|: one round-to-nearest-even of each bf16 P (8 significant bits, unit
    roundoff 2^-8).  A 2^-9 term would reject the prescribed arithmetic itself (err / bound 1.04 on the inputs of
    test_kernels_gpu.py::test_attention[2-64-3]).
  No mutant of the catalogue is left unrejected.
"""
import math

import pytest
import torch

import _bounds as B

BF16, F32 = torch.bfloat16, torch.float32
CPU = "cpu"
ROWS = []


def _rec(family, mutant, n, total):
  ROWS.append((family, mutant, n, total))
  print(f"[power] {family:10s} {mutant:58s} rejected {n:>7d} / {total}")


def rne(x):
  return x.float().to(BF16).float()


def trunc(x):
  return (x.float().contiguous().view(torch.int32) & ~0xFFFF).view(F32).to(BF16).float()


def accept(family, name, out, ref, bound, legacy, lo_hi=None):
  n = B.count_rejected(out, ref, bound, legacy, lo_hi)
  _rec(family, "ACCEPT " + name, n, out.numel())
  assert n == 0, f"{family}: the bound rejects the prescribed arithmetic ({name}) on {n} elements"


def reject(family, name, out, ref, bound, legacy, lo_hi=None):
  n = B.count_rejected(out, ref, bound, legacy, lo_hi)
  _rec(family, name, n, out.numel())
  assert n > 0, f"{family}: mutant '{name}' passes the bound"
  return n


# ------------------------------------------------------------------ GEMM ----
def test_gemm_bounds_bite():
  """Inputs of test_gemm256_gpu.py::test_nt_matches_reference at 512 x 768 x 768 (bias, bf16 and fp32 out) and of the
  +residual epilogue on the fp32 stream."""
  M, N, K = 512, 768, 768
  a = B.rnd((M, K), CPU, 1, dtype=BF16)
  w = B.rnd((N, K), CPU, 2, 0.05, dtype=BF16)
  bias = B.rnd((N,), CPU, 3)
  prod64 = a.double() @ w.double().T
  ref = prod64 + bias.double()
  ap = B.absprod(a, w.T)
  bnd = B.gemm_bf16(ref, ap, K)
  leg = (1e-2, 1e-2)
  prod32 = a.float() @ w.float().T
  pre32 = prod32 + bias
  accept("gemm", "fp32 matmul + bias, RNE to bf16", rne(pre32), ref, bnd, leg)
  reject("gemm", "truncate fp32 to bf16 (no RNE)", trunc(pre32), ref, bnd, leg)
  reject("gemm", "+bias after rounding the product to bf16", rne(rne(prod32) + bias), ref, bnd, leg)
  acc = torch.zeros(M, N)
  for k0 in range(0, K, 64):
    acc = rne(acc + a[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().T)
  reject("gemm", "accumulator rounded to bf16 once per 64-wide K-tile", rne(acc + bias), ref, bnd, leg)
  tile = a[:, 320:384].float() @ w[:, 320:384].float().T
  reject("gemm", "one 64-wide K-tile dropped", rne(pre32 - tile), ref, bnd, leg)
  reject("gemm", "one 64-wide K-tile repeated", rne(pre32 + tile), ref, bnd, leg)
  o = rne(pre32)
  m1 = o.clone(); m1[255::256] = o[254::256]
  reject("gemm", "last row of each 256 tile taken from its neighbour", m1, ref, bnd, leg)
  m2 = o.clone(); m2[:, 255::256] = o[:, 254::256]
  reject("gemm", "last column of each 256 tile taken from its neighbour", m2, ref, bnd, leg)
  # fp32 outputs: bias (legacy 1e-4 / 2e-3) and +residual on the fp32 stream
  bf = B.gemm_f32(ref, ap, K)
  accept("gemm", "fp32 out: fp32 matmul + bias", pre32, ref, bf, (1e-4, 2e-3))
  reject("gemm", "fp32 out: one 64-wide K-tile dropped", pre32 - tile, ref, bf, (1e-4, 2e-3))
  res = B.rnd((M, N), CPU, 11)
  rref = ref + res.double()
  br = B.gemm_f32(rref, ap, K, n_adds=2)
  accept("gemm", "fp32 out: + fp32 residual", pre32 + res, rref, br, (1e-4, 2e-3))
  reject("gemm", "fp32 out: residual added in bf16 on the fp32 stream", pre32 + rne(res), rref, br, (1e-4, 2e-3))


# ------------------------------------------------------------------ GELU ----
K0, K1 = B._K0, B._K1
U0, U1 = 2 * 0.7978845608028654, 2 * 0.7978845608028654 * 3 * 0.044715


def gelu32(h):
  """bv_common.h's fp32 operation sequence: z = x (k0 + k1 x^2), s = 1 / (1 + 2^z), g = x s, g' = s + g (1 - s) u'."""
  x = h.float()
  z = x * (x * x * K1 + K0)
  s = 1.0 / (torch.exp2(z) + 1.0)
  g = x * s
  dg = g * (1.0 - s) * (x * x * U1 + U0) + s
  return g, dg


def test_gelu_epilogue_bounds_bite():
  """Inputs of test_gemm256_gpu.py::test_nt_epilogues (512 x 512 x 256): EPI_GELU's h and g, GELU_GD's g', and
  GELU_BWD's dX = bf16(P o bf16(gelu'(h))) on the stored pre-activation hh, each checked stage by stage."""
  M, N, K = 512, 512, 256
  x = B.rnd((M, K), CPU, 8, dtype=BF16)
  w = B.rnd((N, K), CPU, 9, 0.1, dtype=BF16)
  b = B.rnd((N,), CPU, 10)
  ap = B.absprod(x, w.T)
  prod64 = x.double() @ w.double().T
  pre64 = prod64 + b.double()
  prod32 = x.float() @ w.float().T
  pre32 = prod32 + b
  h = rne(pre32)
  accept("gelu", "h = RNE(fp32 pre)", h, pre64, B.gemm_bf16(pre64, ap, K), (1e-2, 1e-2))
  gref, gb = B.gelu_g(h)
  g32, dg32 = gelu32(h)
  accept("gelu", "g = RNE(gelu_tanh(h)) in fp32", rne(g32), gref, gb, (1e-2, 1e-2))
  reject("gelu", "erf GELU instead of the tanh form", rne(torch.nn.functional.gelu(h)), gref, gb, (1e-2, 1e-2))
  reject("gelu", "GELU of the fp32 pre-activation instead of bf16(h)", rne(gelu32(pre32)[0]), gref, gb, (1e-2, 1e-2))
  dref, db = B.gelu_dg(h)
  accept("gelu", "g' = RNE(gelu_tanh'(h)) in fp32 (GELU_GD)", rne(dg32), dref, db, (1e-2, 1e-2))
  reject("gelu", "g' of the fp32 pre-activation (GELU_GD)", rne(gelu32(pre32)[1]), dref, db, (1e-2, 1e-2))
  hh = B.rnd((M, N), CPU, 15, dtype=BF16)
  _, dgh = gelu32(hh)
  lo_hi, bb = B.gelu_bwd(prod64, ap, K, hh)
  legacy_ref = prod64 * B.dgelu_tanh64(hh)
  accept("gelu_bwd", "dX = RNE(P o RNE(gelu'(h)))", rne(prod32 * rne(dgh)), legacy_ref, bb, (1e-2, 2e-2), lo_hi)
  reject("gelu_bwd", "gelu'(h) not rounded to bf16 before the product", rne(prod32 * dgh), legacy_ref, bb, (1e-2, 2e-2),
         lo_hi)
  reject("gelu_bwd", "erf GELU' in the fused backward",
         rne(prod32 * rne(torch.func.grad(lambda t: torch.nn.functional.gelu(t).sum())(hh.float()))), legacy_ref, bb,
         (1e-2, 2e-2), lo_hi)
  g_emit = rne(gelu32(hh)[0])
  gr2, gb2 = B.gelu_g(hh)
  accept("gelu_bwd", "EMIT: g = RNE(gelu_tanh(aux))", g_emit, gr2, gb2, (1e-2, 1e-2))
  reject("gelu_bwd", "EMIT: erf GELU", rne(torch.nn.functional.gelu(hh.float())), gr2, gb2, (1e-2, 1e-2))


# ------------------------------------------------------------- LayerNorm ----
def _tree_sum(v):
  """layernorm.hip's summation order: D / 64 values per lane, then a 6-level butterfly across the 64 lanes."""
  rows, D = v.shape
  pad = (-D) % 64
  v = torch.nn.functional.pad(v, (0, pad)).view(rows, -1, 64)
  s = torch.zeros(rows, 64)
  for i in range(v.shape[1]):
    s = s + v[:, i]
  while s.shape[1] > 1:
    s = s[:, :s.shape[1] // 2] + s[:, s.shape[1] // 2:]
  return s


def ln_fwd32(x, scale, bias, eps=1e-6, two_pass=False, ddof=0):
  x = x.float(); D = x.shape[1]
  mean = _tree_sum(x) / D
  if two_pass:
    var = _tree_sum((x - mean) ** 2) / (D - ddof)
  else:
    var = (_tree_sum(x * x) / D - mean * mean).clamp_min(0) * (D / (D - ddof))
  rstd = torch.rsqrt(var + eps)
  return (x - mean) * rstd * scale + bias, mean, rstd


def ln_bwd32(dy, x, scale, mean, rstd, dres=None, drop_mean=False):
  g = dy.float() * scale
  xh = (x.float() - mean) * rstd
  D = x.shape[1]
  s1 = _tree_sum(g) / D
  s2 = _tree_sum(g * xh) / D
  dx = rstd * (g - (0 if drop_mean else s1) - xh * s2)
  return dx + (dres.float() if dres is not None else 0)


@pytest.mark.parametrize("bf16_x", [False, True], ids=["f32-stream", "bf16-stream"])
def test_layernorm_bounds_bite(bf16_x):
  """Inputs of test_kernels_gpu.py::test_layernorm (37 x 768) with the edge rows: mean ~0 and std 1e-2 / 1e-3, and
  |mean| / std = 4.  Forward fp32 / bf16 outputs, backward fp32 / bf16 dx, dscale."""
  rows, D = 37, 768
  x = B.rnd((rows, D), CPU, 1, 2.0) + 0.5
  written = B.ln_edge_rows(x)
  if bf16_x:
    x = x.to(BF16).float()
  scale = 1 + 0.1 * B.rnd((D,), CPU, 2); bias = 0.1 * B.rnd((D,), CPU, 3)
  fam = "ln" + ("-bf16x" if bf16_x else "")
  ref, bf, bb = B.ln_fwd_bounds(x, scale, bias)
  edge = torch.zeros(rows, 1, dtype=torch.bool)
  edge[[r for r, kind in written if kind.startswith("std")]] = True   # the small-std rows
  for name, two in (("Flax fast variance in fp32", False), ("two-pass variance in fp32", True)):
    y, _, _ = ln_fwd32(x, scale, bias, two_pass=two)
    accept(fam, f"y fp32: {name}", y, ref, bf, (1e-5, 1e-5))
    accept(fam, f"y bf16: {name}", rne(y), ref, bb, (1e-2, 1e-2))
  y5, _, _ = ln_fwd32(x, scale, bias, eps=1e-5)
  n_plain = B.count_rejected(y5[~edge[:, 0]], ref[~edge[:, 0]], bf[~edge[:, 0]], (1e-5, 1e-5))
  _rec(fam, "(info) eps 1e-5, rows of std ~2 only", n_plain, int((~edge).sum()) * D)
  reject(fam, "eps 1e-5 instead of 1e-6 (y fp32)", y5, ref, bf, (1e-5, 1e-5))
  reject(fam, "eps 1e-5 instead of 1e-6 (y bf16)", rne(y5), ref, bb, (1e-2, 1e-2))
  yd, _, _ = ln_fwd32(x, scale, bias, ddof=1)
  reject(fam, "variance divided by D - 1 (y fp32)", yd, ref, bf, (1e-5, 1e-5))
  reject(fam, "variance divided by D - 1 (y bf16)", rne(yd), ref, bb, (1e-2, 1e-2))
  # backward (fp32 dy and the residual gradient)
  dy = B.rnd((rows, D), CPU, 4)
  dres = B.rnd((rows, D), CPU, 5)
  if bf16_x:
    dres = dres.to(BF16).float()
  _, mean, rstd = ln_fwd32(x, scale, bias)
  dref, dbf, dbb = B.ln_bwd_bounds(x, scale, dy, dres)
  dx = ln_bwd32(dy, x, scale, mean, rstd, dres)
  if not bf16_x:
    accept(fam, "dx fp32: prescribed backward", dx, dref, dbf, (1e-4, 1e-4))
    reject(fam, "dx fp32: mean term missing", ln_bwd32(dy, x, scale, mean, rstd, dres, drop_mean=True), dref, dbf,
           (1e-4, 1e-4))
    _, m5, r5 = ln_fwd32(x, scale, bias, eps=1e-5)
    reject(fam, "dx fp32: eps 1e-5 statistics", ln_bwd32(dy, x, scale, m5, r5, dres), dref, dbf, (1e-4, 1e-4))
  accept(fam, "dx bf16: prescribed backward", rne(dx), dref, dbb, (1e-2, 1e-2))
  reject(fam, "dx bf16: mean term missing", rne(ln_bwd32(dy, x, scale, mean, rstd, dres, drop_mean=True)), dref, dbb,
         (1e-2, 1e-2))
  _, m5, r5 = ln_fwd32(x, scale, bias, eps=1e-5)
  reject(fam, "dx bf16: eps 1e-5 statistics", rne(ln_bwd32(dy, x, scale, m5, r5, dres)), dref, dbb, (1e-2, 1e-2))
  xh = (x.double() - x.double().mean(-1, keepdim=True)) * (x.double().var(-1, unbiased=False, keepdim=True)
                                                           + 1e-6).rsqrt()
  ds_ref = (dy.double() * xh).sum(0)
  xh32 = (x - mean) * rstd
  ds = (dy * xh32).sum(0)
  accept(fam, "dscale: sum dy x_hat", ds, ds_ref, ds_ref.abs() * 0 + 1, (1e-4, 1e-3))
  y32, _, _ = ln_fwd32(x, scale, bias)
  reject(fam, "dscale computed from y instead of x_hat", (dy * y32).sum(0), ds_ref, ds_ref.abs() * 0 + 1, (1e-4, 1e-3))


def _ln_dx32(x, scale, dy, dres, chunk=4096):
  """The fp32 dx of the LayerNorm backward (fp64 arithmetic, rounded once), in row chunks."""
  out = []
  for r0 in range(0, x.shape[0], chunk):
    xs = x[r0:r0 + chunk].double()
    mean = xs.mean(-1, keepdim=True)
    rstd = (xs.var(-1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
    xh = (xs - mean) * rstd
    g = dy[r0:r0 + chunk].double() * scale.double()
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dres is not None:
      dx = dx + dres[r0:r0 + chunk].double()
    out.append(dx.float())
  return torch.cat(out)


def _colsum_worst(dx32, nwg, seed, orders=40):
  """ln_bwd_kernel's fused dx_colsum (layernorm.hip): row r goes to wave r mod 4 nwg, each wave sums its rows in
  fp32 in row order, each workgroup adds its 4 wave partials, and the workgroup partials reach the column sums
  (initialised to 1) by fp32 atomics in an order the hardware chooses.  Worst err / tol, tol = 1e-3 + 1e-4 |ref| (the
  GPU tests' tolerance, ref = 1 + the fp64 sum of the fp32 dx), over `orders` random workgroup orders."""
  rows, D = dx32.shape
  nw = 4 * nwg
  v = torch.nn.functional.pad(dx32, (0, 0, 0, (-rows) % nw)).view(-1, nw, D)
  waves = torch.zeros(nw, D)
  for i in range(v.shape[0]):
    waves = waves + v[i]
  w = waves.view(nwg, 4, D)
  part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
  ref = 1.0 + dx32.double().sum(0)
  tol = 1e-3 + 1e-4 * ref.abs()
  gen = torch.Generator().manual_seed(seed)
  worst = 0.0
  for _ in range(orders):
    acc = torch.ones(D)
    for j in torch.randperm(nwg, generator=gen).tolist():
      acc = acc + part[j]
    worst = max(worst, ((acc.double() - ref).abs() / tol).max().item())
  return worst


@pytest.mark.parametrize("D", [1024, 1152])
def test_ln_colsum_is_order_independent(D):
  """The NT = 3 buckets of test_kernel_buckets_gpu.py::test_layernorm_f32_bucket (the most workgroups: 768 at D =
  1024, 512 at D = 1152): on the inputs of the launch whose fused dx_colsum is checked (no edge rows), every order of
  the workgroups' atomics stays well inside the colsum tolerance.  The same inputs with the edge rows (rstd ~ 700,
  dx ~ 700) are printed for comparison: that is why the edge rows run in launches without column sums."""
  rows = (192 << 20) // (4 * D) + 3
  nwg = 768 if D <= 1024 else 512
  x = B.rnd((rows, D), CPU, 1, 2.0) + 0.5
  scale = 1 + 0.1 * B.rnd((D,), CPU, 2)
  dy32 = B.rnd((rows, D), CPU, 4)
  xe = x.clone()
  B.ln_edge_rows(xe)
  for dy in (dy32, dy32.to(BF16).float()):
    for dres in (None, B.rnd((rows, D), CPU, 5)):
      tag = f"D{D} rows{rows} dy {'fp32' if dy is dy32 else 'bf16'}, dres {dres is not None}"
      worst = _colsum_worst(_ln_dx32(x, scale, dy, dres), nwg, seed=D)
      worst_e = _colsum_worst(_ln_dx32(xe, scale, dy, dres), nwg, seed=D)
      print(f"[colsum] {tag}: worst err/tol over 40 atomic orders {worst:.3f} (with edge rows {worst_e:.3f})")
      assert worst < 0.5, f"{tag}: the fused column sum depends on the atomic order near its tolerance ({worst:.3f})"


# ------------------------------------------------------------- attention ----
def _attn32(qkv, n, L, H, Dh, lens, scale_after_round=False):
  """fp32 forward as attention3.hip does it: S fp32, P = exp(S - max) fp32 with an fp32 row sum, bf16(P) V."""
  q, k, v = qkv.float().view(n, L, 3, H, Dh).unbind(2)
  sc = 1.0 / math.sqrt(Dh)
  s = torch.einsum("nqhd,nkhd->nhqk", q, k)
  s = (rne(s) if scale_after_round else s) * sc
  mask = torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]
  s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
  m = s.amax(-1, keepdim=True)
  p = torch.exp(s - m)
  l = p.sum(-1, keepdim=True)
  o = torch.einsum("nhqk,nkhd->nqhd", rne(p), v) / l.permute(0, 2, 1, 3)
  return rne(o.reshape(n * L, H * Dh)), (m + torch.log(l))[..., 0]


LOG2E = 1.4426950408889634


def _attn_bwd32(qkv, d_o, n, L, H, Dh, lens=None, path="attn3 dq+dkv", rb=rne, rb_out=rne, delta_from_o=False,
                dp_bf16=False, dk_scale=None, dq_scale=None, drop_dq_key=None, drop_dkv_query=None, bwd_lens=None,
                drop_dq_tail=False, drop_dkv_tail=False):
  """The backward as the kernels document it, in fp32: lse from the fp32 forward, P = exp2(S c - lse log2 e), delta =
  fp32 rowsum(P o dP) (path "attn3 dq1...": delta~ = rowsum(dO o bf16 O), eps = rowsum(dS~), the eps correction),
  dS = P o (dP - delta) ("attn5": from the bf16 P), bf16 P / dS operands, fp32 accumulation, the scale on the
  accumulator, one rounding to bf16.  Returns (dqkv, delta, bias gradients = column sums of the fp32 accumulators).
  rb / rb_out: the operand / output rounding (rne, or trunc for the truncation slips); the other keywords are the
  slips of the catalogue; bwd_lens: key-padding lengths the BACKWARD masks with (the lse stays the forward's)."""
  q, k, v = qkv.float().view(n, L, 3, H, Dh).unbind(2)
  do = d_o.float().view(n, L, H, Dh)
  sc = torch.tensor(1.0 / math.sqrt(Dh), dtype=F32)
  ar = torch.arange(L)
  lens = [L] * n if lens is None else lens

  def keymask(ls):
    return (ar[None, :] < torch.as_tensor(ls)[:, None])[:, None, None, :]
  st = torch.einsum("nqhd,nkhd->nhqk", q, k)
  sf = (st * sc).masked_fill(~keymask(lens), float("-inf"))
  mx = sf.amax(-1, keepdim=True)
  pf = torch.exp(sf - mx)
  lsum = pf.sum(-1, keepdim=True)
  lse = mx + torch.log(lsum)
  p = torch.exp2(st * (sc * LOG2E) - lse * LOG2E)
  p = p * keymask(lens if bwd_lens is None else bwd_lens)
  dp = torch.einsum("nqhd,nkhd->nhqk", do, v)
  if dp_bf16:
    dp = rne(dp)
  corr = None
  if delta_from_o or "dq1" in path:
    o = rne(torch.einsum("nhqk,nkhd->nqhd", rne(pf), v) / lsum.permute(0, 2, 1, 3))
    dt = (do * o).sum(-1).permute(0, 2, 1)[..., None]
    if delta_from_o:
      delta = dt
    else:
      eps = (p * (dp - dt)).sum(-1, keepdim=True)
      delta = dt + eps
      corr = (dt, eps)
  else:
    delta = (p * dp).sum(-1, keepdim=True)
  pb = rb(p)
  ds = (pb if path == "attn5" else p) * (dp - delta)
  if corr is None:
    dsq = rb(ds)
    if drop_dq_key is not None:
      dsq[..., drop_dq_key] = 0
    if drop_dq_tail:
      dsq[..., L - 1] = 0
    dq = torch.einsum("nhqk,nkhd->nqhd", dsq, k)
  else:
    dq = torch.einsum("nhqk,nkhd->nqhd", rb(p * (dp - corr[0])), k) - \
        corr[1].permute(0, 2, 1, 3) * torch.einsum("nhqk,nkhd->nqhd", pb, k)
  dsk, pv = rb(ds), pb.clone()
  if drop_dkv_query is not None:
    dsk[:, :, drop_dkv_query] = 0; pv[:, :, drop_dkv_query] = 0
  dk = torch.einsum("nhqk,nqhd->nkhd", dsk, q)
  dv = torch.einsum("nhqk,nqhd->nkhd", pv, do)
  dq, dk = dq * sc, dk * sc
  if dq_scale is not None:
    dq[:, :, dq_scale[0]] *= dq_scale[1]
  if dk_scale is not None:
    dk[:, :, dk_scale[0]] *= dk_scale[1]
  if drop_dkv_tail:
    dk[:, L - 1] = 0; dv[:, L - 1] = 0
  acc = torch.stack([dq, dk, dv], 2).reshape(n * L, 3 * H * Dh)
  return rb_out(acc), delta[..., 0], acc.sum(0)


def _bwd_inputs(n, L, H, Dh, seed=1, head_scale=False):
  qkv = B.rnd((n * L, 3 * H * Dh), CPU, seed, 1.5, dtype=BF16)
  d_o = B.rnd((n * L, H * Dh), CPU, seed + 1, dtype=BF16)
  return qkv, d_o


def _autograd_g(qkv, d_o, n, L, H, Dh, lens=None):
  qr = qkv.double().requires_grad_(True)
  q, k, v = qr.view(n, L, 3, H, Dh).unbind(2)
  s = torch.einsum("nqhd,nkhd->nhqk", q / math.sqrt(Dh), k)
  if lens is not None:
    s = s.masked_fill(~(torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None])[:, None, None, :], float("-inf"))
  torch.einsum("nhqk,nkhd->nqhd", torch.softmax(s, -1), v).reshape(n * L, H * Dh).backward(d_o.double())
  return qr.grad


def _bwd_accept(fam, b, out, legacy=3e-2, legacy_db=2e-2, cap_share=0.01):
  """The five outputs of an emulation against the model; the legacy cap may apply on at most cap_share of each."""
  dqkv, delta, db = out
  leg = (legacy, legacy * b.g.abs().max().item())
  w = dqkv.shape[1] // 3
  for j, part in enumerate(("dq", "dk", "dv")):
    sl = slice(j * w, (j + 1) * w)
    accept(fam, f"{part} [{b.path}]", dqkv[:, sl], b.g[:, sl], b.g_bound[:, sl], leg)
    share = B.capped_share(b.g[:, sl], b.g_bound[:, sl], leg)
    assert share <= cap_share, f"{fam} {part}: the legacy cap applies on {100 * share:.2f}% of the elements"
  accept(fam, f"delta [{b.path}]", delta, b.delta, b.delta_bound, B.NO_LEGACY)
  leg_db = (legacy_db, legacy_db * b.g.abs().sum(0).max().item())
  bnd = B.f32_bound(b.db, b.db_bound)
  accept(fam, f"bias gradients [{b.path}]", db, b.db, bnd, leg_db)
  assert B.capped_share(b.db, bnd, leg_db) <= cap_share
  return leg, leg_db, bnd


def _legacy_count(out, ref, legacy):
  return B.count_rejected(out, ref, torch.full_like(ref, float("inf")), legacy)


def _bwd_reject(fam, name, out, ref, bound, legacy):
  """The model (capped at the legacy tolerance) must reject; the legacy tolerance's own count is recorded next to it."""
  reject(fam, name, out, ref, bound, legacy)
  _rec(fam, "  (legacy tolerance alone) " + name, _legacy_count(out, ref, legacy), out.numel())


@pytest.mark.parametrize("L", [197, 576])
def test_attention_bounds_bite(L):
  """Inputs of test_kernels_gpu.py's attention cases (qkv scaled 1.5, seed 1 / 5): o and lse against the contraction
  model, dqkv against the backward model (attn_bwd_bounds, capped at the earlier 3e-2 max|g|); masked with the
  key-padding lengths of the masked test."""
  n, H, Dh = 2, 1, 64
  qkv = B.rnd((n * L, 3 * H * Dh), CPU, 5, 1.5, dtype=BF16)
  lens = [L, L // 3]
  o_ref, ob, lse_ref, lb = B.attn_fwd_bounds(qkv, n, L, H, Dh, lens)
  o, lse = _attn32(qkv, n, L, H, Dh, lens)
  fam = f"attn L{L}"
  accept(fam, "o: fp32 softmax, bf16 P V", o, o_ref, ob, (2e-2, 2e-2))
  accept(fam, "lse: fp32", lse, lse_ref, lb, (1e-4, 1e-3))
  om, lm = _attn32(qkv, n, L, H, Dh, [ln + 1 if ln < L else ln for ln in lens])
  reject(fam, "o: key mask off by one", om, o_ref, ob, (2e-2, 2e-2))
  reject(fam, "lse: key mask off by one", lm, lse_ref, lb, (1e-4, 1e-3))
  os_, ls_ = _attn32(qkv, n, L, H, Dh, lens, scale_after_round=True)
  reject(fam, "o: score scale applied after rounding S to bf16", os_, o_ref, ob, (2e-2, 2e-2))
  reject(fam, "lse: score scale applied after rounding S to bf16", ls_, lse_ref, lb, (1e-4, 1e-3))
  # backward, unmasked, at this test's own shape (the catalogue proper is test_attention_backward_bounds_bite)
  qkv1, d_o = _bwd_inputs(n, L, H, Dh)
  b = B.attn_bwd_bounds(qkv1, d_o, n, L, H, Dh)
  g = _autograd_g(qkv1, d_o, n, L, H, Dh)
  assert (b.g - g).abs().max().item() <= 1e-12 * g.abs().max().item(), "the model's reference is not the gradient"
  leg, _, _ = _bwd_accept(fam, b, _attn_bwd32(qkv1, d_o, n, L, H, Dh, path=b.path))
  _bwd_reject(fam, "dQ misses the last key", _attn_bwd32(qkv1, d_o, n, L, H, Dh, path="attn3 dq+dkv",
                                                         drop_dq_tail=True)[0], b.g, b.g_bound, leg)
  _bwd_reject(fam, "dK / dV of the last key dropped", _attn_bwd32(qkv1, d_o, n, L, H, Dh, path=b.path,
                                                                  drop_dkv_tail=True)[0], b.g, b.g_bound, leg)


@pytest.mark.parametrize("L,Dh", [(64, 64), (197, 64), (441, 64), (100, 72)])
def test_attention_backward_bounds_bite(L, Dh):
  """The backward model (attn_bwd_bounds) on the GPU tests' seeded inputs (qkv seed 1 scaled 1.5, dO seed 2), H = 2.
  Accepts the documented arithmetic, for dq / dk / dv, delta and the bias gradients, of
    * the two-sweep path "attn3 dq+dkv" (every masked launch, and unmasked under BV_OPT_ATTN_CFG bits 16 | 128) /
      "adh" at Dh = 72 - the base model, one rounding of dS;
    * the path the unmasked shape dispatches to by default (attn5 at L = 64 / 197, the one-sweep dq1 at L = 441);
    * the masked launches with the key-padding lengths [L, L // 4, L - 1].
  Rejects the catalogue of slips under the base model, each with the count of the legacy tolerance (3e-2 max|g|)
  next to it.  Under the attn5 / dq1 variants the same slips are run again: attn5 documents a second 2^-8 rounding
  of dS (from the bf16 P), which is of the size of the two subtle slips (delta from the bf16 O, dP rounded to bf16),
  so those two are recorded there without an assertion; every other slip must be rejected there too."""
  n, H = 2, 2
  qkv, d_o = _bwd_inputs(n, L, H, Dh)
  g = _autograd_g(qkv, d_o, n, L, H, Dh)
  w = H * Dh
  base = "adh" if Dh != 64 else "attn3 dq+dkv"
  for path in dict.fromkeys((base, B.attn_bwd_path(L, Dh, False))):
    fam = f"attn-bwd L{L} Dh{Dh} {path}"
    b = B.attn_bwd_bounds(qkv, d_o, n, L, H, Dh, path=path)
    assert (b.g - g).abs().max().item() <= 1e-12 * g.abs().max().item(), "the model's reference is not the gradient"
    leg, leg_db, db_bnd = _bwd_accept(fam, b, _attn_bwd32(qkv, d_o, n, L, H, Dh, path=path))

    def slip(name, subtle=False, **kw):
      out = _attn_bwd32(qkv, d_o, n, L, H, Dh, path=path, **kw)[0]
      if subtle and path != base:
        _rec(fam, "(recorded) " + name, B.count_rejected(out, b.g, b.g_bound, leg), out.numel())
        _rec(fam, "  (legacy tolerance alone) " + name, _legacy_count(out, b.g, leg), out.numel())
      else:
        _bwd_reject(fam, name, out, b.g, b.g_bound, leg)
    if "dq1" not in path:   # (dq1 builds delta from the bf16 O by design and corrects it: not a slip there)
      slip("delta = rowsum(dO o bf16 O)", subtle=True, delta_from_o=True)
      reject(fam, "the delta buffer itself = rowsum(dO o bf16 O)",
             _attn_bwd32(qkv, d_o, n, L, H, Dh, path=path, delta_from_o=True)[1], b.delta, b.delta_bound, B.NO_LEGACY)
    slip("dP rounded to bf16 before the subtraction", subtle=True, dp_bf16=True)
    slip("dK of head 1 scaled by 0.12 instead of 0.125 (4 %)", dk_scale=(1, 0.96))
    slip("dQ of head 1 scaled by 0.12 instead of 0.125 (4 %)", dq_scale=(1, 0.96))
    if "dq1" not in path:   # (the emulation of the eps correction has no per-key dS to drop)
      slip("dQ misses a middle key", drop_dq_key=L // 2)
    slip("dK / dV miss one query", drop_dkv_query=L // 2)
    db = _attn_bwd32(qkv, d_o, n, L, H, Dh, path=path)[2]
    dbk = db.clone(); dbk[w:2 * w] = db[:w]
    _bwd_reject(fam, "k-bias gradient of the size of the q-bias gradient", dbk, b.db, db_bnd, leg_db)
  fam = f"attn-bwd L{L} Dh{Dh}"
  # masked: the lengths the GPU tests use; two samples at a time (the model and the emulation are per sample)
  for lens in ([L, L // 4], [L - 1, L // 4]):
    mfam = f"{fam} lens{lens}"
    bm = B.attn_bwd_bounds(qkv, d_o, n, L, H, Dh, lens)
    lm, _, _ = _bwd_accept(mfam, bm, _attn_bwd32(qkv, d_o, n, L, H, Dh, lens, path=bm.path))
    for d in (1, -1):
      out = _attn_bwd32(qkv, d_o, n, L, H, Dh, lens, path=bm.path, bwd_lens=[min(L, ln + d) for ln in lens])[0]
      _bwd_reject(mfam, f"backward key mask off by {d:+d}", out, bm.g, bm.g_bound, lm)
      if d == 1:
        pad = out.view(n, L, 3, H, Dh)[1, lens[1]:, 1:]
        assert (pad != 0).any(), "the off-by-one mask must leave a non-zero dK / dV on a padded key"
  # truncation instead of round-to-nearest-even, three seeds: an elementwise bound of ~1 bf16 ulp cannot separate a
  # rounding-mode slip robustly (a truncated operand is off by < 1 ulp, inside 2^-8 sum |dS| |K|); recorded, not asserted
  for seed in (1, 3, 5):
    qs, gs = _bwd_inputs(n, L, H, Dh, seed)
    bs = b if seed == 1 else B.attn_bwd_bounds(qs, gs, n, L, H, Dh)
    ls = (3e-2, 3e-2 * bs.g.abs().max().item())
    for what, kw in (("bf16 P / dS operands", dict(rb=trunc)), ("dqkv output", dict(rb_out=trunc))):
      out = _attn_bwd32(qs, gs, n, L, H, Dh, path=bs.path, **kw)[0]
      _rec(fam, f"(not separable by an elementwise bound) truncated {what}, seed {seed}",
           B.count_rejected(out, bs.g, bs.g_bound, ls), out.numel())


def _map32(q, kv, d_o, n, L, H, Dh, lens=None, norm_lens=None, centre=True):
  """attention.hip's MAP kernels in fp32: p = exp(s - max) / sum over the valid keys, o = bf16(sum p v); backward from
  that p: ds = p (dp - sum p dp), dq, dk, dv rounded once.  norm_lens: lengths the softmax normalises over (slip);
  centre = False drops the dp - dsum centring of dkv (slip)."""
  qf = q.float().view(n, H, Dh)
  k, v = kv.float().view(n, L, 2, H, Dh).unbind(2)
  do = d_o.float().view(n, H, Dh)
  sc = torch.tensor(1.0 / math.sqrt(Dh), dtype=F32)
  lens = [L] * n if lens is None else lens
  s = torch.einsum("nhd,nkhd->nhk", qf, k) * sc
  valid = (torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None])[:, None, :]
  nv = valid if norm_lens is None else (torch.arange(L)[None, :] < torch.as_tensor(norm_lens)[:, None])[:, None, :]
  e = torch.exp(s.masked_fill(~nv, float("-inf")) - s.masked_fill(~nv, float("-inf")).amax(-1, keepdim=True))
  p = e * (1.0 / e.sum(-1, keepdim=True)) * valid
  o = rne(torch.einsum("nhk,nkhd->nhd", p, v)).reshape(n, H * Dh)
  dp = torch.einsum("nhd,nkhd->nhk", do, v)
  dsum = (p * dp).sum(-1, keepdim=True)
  ds = p * (dp - dsum)
  dq = rne(torch.einsum("nhk,nkhd->nhd", ds, k) * sc).reshape(n, H * Dh)
  dsk = ds if centre else p * dp
  dk = dsk.permute(0, 2, 1)[..., None] * (qf * sc)[:, None]
  dv = p.permute(0, 2, 1)[..., None] * do[:, None]
  return p, o, dq, rne(torch.stack([dk, dv], 2).reshape(n * L, 2 * H * Dh))


@pytest.mark.parametrize("Dh", [64, 72])
def test_map_attention_bounds_bite(Dh):
  """MAP attention (test_kernels_gpu.py's inputs: q seed 1, kv seed 2, dO seed 3) at n = 3, L = 70, H = 3, unmasked
  and with key-padding lengths: p, o, dq, dkv of the fp32 arithmetic are accepted; dkv without the dP - delta
  centring and p normalised over L instead of kv_len are rejected."""
  n, L, H = 3, 70, 3
  q = B.rnd((n, H * Dh), CPU, 1, dtype=BF16)
  kv = B.rnd((n * L, 2 * H * Dh), CPU, 2, dtype=BF16)
  d_o = B.rnd((n, H * Dh), CPU, 3, dtype=BF16)
  for lens in (None, [L, L // 2, L - 1]):
    fam = f"map Dh{Dh}" + (" masked" if lens else "")
    p_ref, pb, o_ref, ob = B.map_attn_fwd_bounds(q, kv, n, L, H, Dh, lens)
    dq_ref, dqb, dkv_ref, dkvb = B.map_attn_bwd_bounds(q, kv, d_o, n, L, H, Dh, lens)
    lq = (2e-2, 2e-2 * dq_ref.abs().max().item()); lkv = (2e-2, 2e-2 * dkv_ref.abs().max().item())
    p, o, dq, dkv = _map32(q, kv, d_o, n, L, H, Dh, lens)
    accept(fam, "p: fp32 softmax", p, p_ref, pb, (1e-3, 1e-5))
    accept(fam, "o: fp32 p v, one rounding", o, o_ref, ob, (1e-2, 1e-2))
    accept(fam, "dq", dq, dq_ref, dqb, lq)
    accept(fam, "dkv", dkv, dkv_ref, dkvb, lkv)
    for ref, bnd, leg in ((p_ref, pb, (1e-3, 1e-5)), (o_ref, ob, (1e-2, 1e-2)), (dq_ref, dqb, lq), (dkv_ref, dkvb, lkv)):
      assert B.capped_share(ref, bnd, leg) <= 0.01
    _bwd_reject(fam, "dkv without the dP - delta centring", _map32(q, kv, d_o, n, L, H, Dh, lens, centre=False)[3],
                dkv_ref, dkvb, lkv)
    if lens:
      _bwd_reject(fam, "p normalised over L instead of kv_len", _map32(q, kv, d_o, n, L, H, Dh, lens,
                                                                       norm_lens=[L] * n)[0], p_ref, pb, (1e-3, 1e-5))


# ---------------------------------------------------------------- losses ----
def test_loss_bounds_bite_on_extreme_rows():
  """The extreme rows the GPU loss tests gained: fp32 emulations of the stable forms pass the (unchanged) tolerances
  against fp64; the naive forms overflow and fail."""
  import bv_oracle as O
  # softmax xent, logits up to +-1e3
  logits, labels = B.softmax_xent_extreme_inputs(CPU)
  n = logits.shape[0]
  lr = logits.double().requires_grad_(True)
  ref = O.softmax_xent(lr, labels.double()); ref.backward()

  def xent32(lg, subtract_max=True):
    m = lg.amax(-1, keepdim=True) if subtract_max else torch.zeros_like(lg[:, :1])
    lse = torch.log(torch.exp(lg - m).sum(-1, keepdim=True))
    loss = (-(labels * (lg - m)).sum(-1) + labels.sum(-1) * lse[:, 0]).sum() / n
    dl = (torch.exp(lg - m - lse) * labels.sum(-1, keepdim=True) - labels) / n
    return loss, dl
  lo, dl = xent32(logits)
  one = torch.ones(1, dtype=torch.float64)
  accept("xent", "softmax xent: max subtracted", lo.reshape(1), ref.detach().reshape(1), one, (1e-5, 1e-6))
  accept("xent", "softmax xent dlogits: max subtracted", dl, lr.grad, torch.ones_like(dl.double()), (1e-4, 1e-7))
  lo2, dl2 = xent32(logits, subtract_max=False)
  reject("xent", "softmax without subtracting the max (loss)", lo2.reshape(1), ref.detach().reshape(1), one, (1e-5, 1e-6))
  reject("xent", "softmax without subtracting the max (dlogits)", dl2, lr.grad, torch.ones_like(dl.double()),
         (1e-4, 1e-7))
  # sigmoid xent, logits beyond +-90
  logits, labels = B.sigmoid_xent_extreme_inputs(CPU)
  n = logits.shape[0]
  lr = logits.double().requires_grad_(True)
  ref = O.sigmoid_xent(lr, labels.double()); ref.backward()

  def sxent32(lg, naive=False):
    if naive:
      lp, lnp = -torch.log(1 + torch.exp(-lg)), -torch.log(1 + torch.exp(lg))
    else:
      sp = torch.log1p(torch.exp(-lg.abs()))
      lp, lnp = lg.clamp(max=0) - sp, (-lg).clamp(max=0) - sp
    return (-(labels * lp + (1 - labels) * lnp)).sum() / n
  accept("sig-xent", "sigmoid xent: stable log-sigmoid", sxent32(logits).reshape(1), ref.detach().reshape(1), one,
         (1e-5, 1e-5))
  reject("sig-xent", "naive log(1 + exp(-x))", sxent32(logits, True).reshape(1), ref.detach().reshape(1), one,
         (1e-5, 1e-5))
  # SigLIP at t = 100, b = -10
  zi, zt = B.siglip_extreme_inputs(CPU)
  nn_, Bn, off = zi.shape[0], zt.shape[0], 14
  raw = zi @ zt.T
  m = -torch.ones(nn_, Bn); m[torch.arange(nn_), off + torch.arange(nn_)] = 1.0
  lg64 = 100.0 * raw.double() - 10.0
  ref = (-O.log_sigmoid(m.double() * lg64).sum(-1)).sum() / Bn
  x = m * (100.0 * raw - 10.0)
  assert x.min().item() < -88.8, "the SigLIP inputs must push exp(-x) beyond the fp32 range"
  stable = ((-x).clamp_min(0) + torch.log1p(torch.exp(-x.abs()))).sum() / Bn
  naive = torch.log(1 + torch.exp(-x)).sum() / Bn
  accept("siglip", "SigLIP loss: max(-x, 0) + log1p(exp(-|x|))", stable.reshape(1), ref.reshape(1), one, (1e-5, 1e-6))
  reject("siglip", "naive log(1 + exp(-x))", naive.reshape(1), ref.reshape(1), one, (1e-5, 1e-6))


# ------------------------------------------------------------- optimizer ----
# fp32 emulations of loss_optim.hip opt_chain and adafactor.hip with the signatures of big_vision_amd.ops: the same
# order of operations, fp32 intermediates, bf16 stores by round-to-nearest-even.  `slip` makes one catalogued mistake.
import types

import numpy as np

import _opt_cases as OC

f32 = np.float32


def _clip32(gsq, clip_norm, slip=None):
  cn = f32(clip_norm or 0.0)
  if not cn > 0:
    return 1.0
  gn = f32(np.sqrt(np.float64(gsq.item())))
  if slip == "clip applied unconditionally":
    return float(cn / gn) if gn > 0 else 1.0
  return float(cn / gn) if gn > cn else 1.0


def _store(buf, val, slip, what):
  if buf.dtype == BF16:
    buf.copy_((trunc(val) if slip == f"{what} stored by truncation" else rne(val)).to(BF16))
  else:
    buf.copy_(val)


def _one_minus(b):
  return float(f32(1) - f32(b))


def emu_chain(kind, p, g, acc, nu, shadow, segs, chunk_seg, count, sched, gsq, clip_norm, stats, slip=None, b1=0, b2=0,
              eps=0, bc1=1, bc2=1, beta=0, nesterov=False, k=None):
  arr = segs.numpy().view(OC.SEG)
  cs = chunk_seg.long()
  el = lambda a: torch.from_numpy(np.ascontiguousarray(a))[cs].repeat_interleave(1024)
  lr, wd, si = el(arr["lr"]), el(arr["wd"]), el(arr["si"]).long()
  if slip == "a segment's sched_idx off by one":
    si = (si + 1) % OC.MAX_SCHED
  sc = torch.tensor([float(f32(v)) for v in sched] + [0.0] * (OC.MAX_SCHED - len(sched)), dtype=F32)[si]
  clip = _clip32(gsq, clip_norm, slip)
  late = slip == "clip applied after the moments"
  gc = g * clip if not late else g.clone()
  pv = p.clone()
  if slip == "weight decay coupled into g before the moments":
    gc = gc + wd * pv
  if kind == "adam":
    b1, b2, eps, bc1, bc2 = (float(f32(x)) for x in (b1, b2, eps, bc1, bc2))
    if slip == "bc computed for step k rather than k + 1":
      bc1, bc2 = float(f32(1 - b1 ** k)), float(f32(1 - b2 ** k))
    m = b1 * acc.float() + _one_minus(b1) * gc
    gv = g if slip == "nu updated with the unclipped g" else gc
    v = b2 * nu + _one_minus(b2) * gv * gv
    mm = rne(m) if slip == "update formed from the bf16-rounded mu" else m
    if late:
      mm = mm * clip
    mh = mm if slip == "bias correction of mu omitted" else mm / bc1
    vh = v if slip == "bias correction of nu omitted" else v / bc2
    if slip == "eps inside the square root":
      u = mh / torch.sqrt(vh + eps)
    elif slip == "eps added before the bc2 division":
      u = mh / torch.sqrt((v + eps) / bc2)
    else:
      u = mh / (torch.sqrt(vh) + eps)
    nu.copy_(v)
    _store(acc, m, slip, "mu")
  elif kind == "trace":
    beta = float(f32(beta))
    t = gc + beta * acc.float()
    if nesterov:
      tt = rne(t) if slip == "Nesterov from the rounded t'" else t
      u = gc + beta * (acc.float() if slip == "Nesterov as g + beta t_old" else tt)
    else:
      u = rne(t) if slip == "update formed from the bf16-rounded mu" else t
    if late:
      u = u * clip
    _store(acc, t, slip, "mu")
  else:
    u = gc * (clip if late else 1.0)
  if slip == "weight decay coupled into g before the moments":
    d = (lr * u) * sc
  elif slip == "weight decay not multiplied by the schedule":
    d = (lr * u) * sc + wd * pv
  else:
    d = (lr * u + wd * pv) * sc
  p.copy_(pv - d)
  shadow.copy_(p.to(BF16))
  if stats is not None:
    stats += torch.stack([(p.double() ** 2).sum(), (d.double() ** 2).sum()])


def _af_leaf_emu(p, g, mom, shadow, view, st, factored, clip, decay, eps, momentum, lr_eff, wd, sched, stats, slip=None,
                 usq_out=None, block_rms_clip=0.0):
  o, B1, B2, R, C = (int(x) for x in view[:5])
  Bn = B1 * B2
  pv, gv, mv, sv = B.af_views([p, g, mom, shadow], view)
  x = (gv * clip).reshape(Bn, R, C)
  xs = gv.reshape(Bn, R, C) if slip == "statistics formed from the unclipped gradient" else x
  decay, momentum = float(f32(decay)), float(f32(momentum))
  e = 0.0 if slip == "eps omitted" else float(f32(eps))
  od, om = _one_minus(decay), _one_minus(momentum)
  if factored:
    v_row, v_col = st[:Bn * R].view(Bn, R), st[Bn * R:Bn * R + Bn * C].view(Bn, C)
    rcm = st[Bn * R + Bn * C:Bn * R + Bn * C + Bn]
    sq = xs * xs + e
    nC = R if slip == "the mean divided by the wrong extent (R for C)" else C
    v_row.copy_(decay * v_row + od * (sq.sum(2) / nC))
    v_col.copy_(decay * v_col + od * (sq.sum(1) / R))
    rcm.copy_(v_row.sum(1) / R)
    if slip == "row and column factors exchanged":
      assert R == C
      rf, cf = torch.rsqrt(v_col / rcm[:, None]), torch.rsqrt(v_row)
    elif slip == "row and column factors exchanged (R != C)":   # v_col read with the row index, v_row with the column's
      ci = torch.arange(C).clamp_max(R - 1)
      rf, cf = torch.rsqrt(v_col[:, torch.arange(R).clamp_max(C - 1)] / rcm[:, None]), torch.rsqrt(v_row[:, ci])
    elif slip == "row and column factors exchanged (rcm divides v_col)":
      rf, cf = torch.rsqrt(v_row), torch.rsqrt(v_col / rcm[:, None])
    elif slip == "rcm omitted":
      rf, cf = torch.rsqrt(v_row), torch.rsqrt(v_col)
    else:
      rf, cf = torch.rsqrt(v_row / rcm[:, None]), torch.rsqrt(v_col)
    u = x * rf[:, :, None] * cf[:, None, :]
  else:
    v = st[:Bn * R * C].view(Bn, R, C)
    v.copy_(decay * v + od * (xs * xs + e))
    u = x * torch.rsqrt(v)
  if block_rms_clip > 0:
    if slip == "block_rms_clip's rms taken per batch slice instead of per leaf":
      usq = (u.double() ** 2).sum((1, 2), keepdim=True)
      rms = torch.sqrt((usq / (R * C)).float())
    else:
      usq = (u.double() ** 2).sum()
      rms = torch.sqrt((usq / (Bn * R * C)).float())
    if usq_out is not None:
      usq_out.copy_(usq.sum())
    u = u * (1.0 / torch.clamp_min(rms / float(f32(block_rms_clip)), 1.0))
  if momentum > 0:
    m = momentum * mv.float().reshape(Bn, R, C) + (u if slip == "(1 - momentum) missing" else om * u)
    mst = trunc(m) if slip == "momentum stored by truncation" else rne(m)
    mv.copy_((mst if mom.dtype == BF16 else m).view(B1, B2, R, C).to(mom.dtype))
    um = rne(m) if slip == "update formed from the bf16-rounded momentum" else m
  else:
    um = u
  pd = pv.reshape(Bn, R, C).clone()
  w = (lr_eff * wd) if slip == "weight decay multiplied by lr_eff" else wd
  upd = -float(f32(sched)) * (float(f32(lr_eff)) * um + float(f32(w)) * pd)
  pn = pd + upd
  pv.copy_(pn.view(B1, B2, R, C))
  sv.copy_(pv.to(BF16))
  if stats is not None:
    stats += torch.stack([(pn.double() ** 2).sum(), (upd.double() ** 2).sum()])


def make_emu(slip=None):
  def adam_step_(p, g, mu, nu, shadow, segs, chunk_seg, count, sched, gsq, clip_norm, b1, b2, eps, bc1, bc2, stats):
    k = round(math.log(1 - bc1) / math.log(b1)) - 1
    emu_chain("adam", p, g, mu, nu, shadow, segs, chunk_seg, count, sched, gsq, clip_norm, stats, slip, b1=b1, b2=b2,
              eps=eps, bc1=bc1, bc2=bc2, k=k)

  def trace_step_(p, g, trace, shadow, segs, chunk_seg, count, sched, gsq, clip_norm, momentum, nesterov, stats):
    emu_chain("trace" if trace is not None else "identity", p, g, trace, None, shadow, segs, chunk_seg, count, sched, gsq,
              clip_norm, stats, slip, beta=momentum, nesterov=nesterov)

  def sqnorm_(x, out):
    out += (x.float() * x.float()).double().sum()

  def adafactor_leaf_(p, g, mom, shadow, view, state, factored, gsq, clip_norm, decay, eps, m, lr_eff, wd, sched, stats):
    if slip == "decay of step k + 1 at step k":
      decay = OC.af_decay(round((1 - decay) ** (-1 / 0.8)))
    _af_leaf_emu(p, g, mom, shadow, list(view), state, factored, _clip32(gsq, clip_norm), decay, eps, m, lr_eff, wd,
                 sched, stats, slip)

  def adafactor_step_(p, g, mom, shadow, leaves, nleaves, max_rows, max_cols, max_b, max_total, state, gsq, clip_norm,
                      decay, eps, m, sched, stats, block_rms_clip=0.0, block_usq=None):
    from big_vision_amd import optax as bvo
    tab = leaves.numpy().reshape(-1).view(bvo.AF_LEAF)
    for j in range(nleaves):
      L = tab[j]
      view = [int(L[n]) for n in ("off", "B1", "B2", "R", "C", "sB1", "sB2", "sR", "sC")]
      Bn = view[1] * view[2]
      n_state = Bn * (view[3] + view[4] + 1) if L["factored"] else Bn * view[3] * view[4]
      _af_leaf_emu(p, g, mom, shadow, view, state[int(L["soff"]):int(L["soff"]) + n_state], bool(L["factored"]),
                   _clip32(gsq, clip_norm), decay, eps, m, float(L["lr_eff"]), float(L["wd"]), sched[int(L["sched_idx"])],
                   stats, slip, usq_out=None if block_usq is None else block_usq[j], block_rms_clip=block_rms_clip)
  return types.SimpleNamespace(adam_step_=adam_step_, trace_step_=trace_step_, sqnorm_=sqnorm_,
                               adafactor_leaf_=adafactor_leaf_, adafactor_step_=adafactor_step_)


EMU = make_emu()


def _accepted(worst, family):
  for k, v in worst.items():
    _rec(family, f"ACCEPT {k}: max err/bound {v:.3f}", 0, 1)
    assert v <= 1.0


@pytest.mark.parametrize("mu", [F32, BF16])
@pytest.mark.parametrize("clip", [0.0, 1e-2])
@pytest.mark.parametrize("nchunks,nseg", [(1, 1), (3, 3), (8, 2)])
def test_adam_model_accepts_the_emulation(nchunks, nseg, clip, mu):
  """The drivers of the GPU file on the fp32 emulation (the 4099-chunk case at 8 chunks: the same alternating segment
  pattern; the grid-stride loop is the kernel's own matter)."""
  _accepted(OC.chain_case(EMU, CPU, "adam", nchunks, nseg, clip, mu), "adam")


@pytest.mark.parametrize("kind,nesterov,dt", [("trace", False, BF16), ("trace", False, F32), ("trace", True, BF16),
                                              ("trace", True, F32), ("identity", False, None)])
def test_trace_model_accepts_the_emulation(kind, nesterov, dt):
  _accepted(OC.chain_case(EMU, CPU, kind, 2, 2, 1e-2, dt, nesterov=nesterov), "trace")


@pytest.mark.parametrize("which", ["zero", "at", "ulp-above", "far"])
def test_clip_threshold_model_accepts_the_emulation(which):
  for kind in ("adam", "trace"):
    _accepted(OC.chain_case(EMU, CPU, kind, 1, 1, 0.5, F32, gsq_value=OC.clip_gsq(which, 0.5)), "clip")
  _accepted(OC.af_leaf_case(EMU, CPU, B.AF_SPECS[0], BF16, 0.5, gsq_value=OC.clip_gsq(which, 0.5)), "clip")
  c, e = B.clip_factor(OC.clip_gsq(which, 0.5), 0.5)
  assert (c == 1.0 and e == 0.0) == (which in ("zero", "at")), (which, c)


@pytest.mark.parametrize("mom", [BF16, F32])
@pytest.mark.parametrize("spec", B.AF_SPECS, ids=[s[0] for s in B.AF_SPECS])
def test_adafactor_model_accepts_the_emulation(spec, mom):
  _accepted(OC.af_leaf_case(EMU, CPU, spec, mom, 1e-2), "adafactor")


@pytest.mark.parametrize("mom", [BF16, F32])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("brc", [0.0, 0.7, 1e6])
def test_adafactor_batched_model_accepts_the_emulation(brc, single, mom):
  _accepted(OC.af_batched_case(EMU, CPU, mom, brc, single), "adafactor")


def test_sqnorm_model_accepts_the_emulation():
  for count in (1, 3, 4, 5, 1023, 1024 * 257 + 3, 2048 * 256 * 4 + 4 * 256 + 1):
    _accepted(OC.sqnorm_case(EMU, CPU, count), "sqnorm")
  _accepted(OC.sqnorm_case(EMU, CPU, 1023, offset=4), "sqnorm")


# ---- rejection: one step of the emulation with one slip, on the GPU cases' inputs, three seeds.  Each line prints the
# elements the model (capped at the legacy tolerance) rejects, then the elements the legacy tolerance alone rejects.
# Legacy tolerances: p (1e-5, 1e-6) for the chain (test_kernels_gpu.py), 2e-5 max(1, max|p|) for Adafactor
# (test_adafactor_gpu.py); state 2e-5 of the leaf's largest state value, 1e-2 when the accumulator is bf16.
SEEDS = (100, 1100, 2100)
# Slips recorded as not separable from rounding.  Exchanging WHICH factor carries rcm, (x rsqrt(v_row)) rsqrt(v_col /
# rcm), is the same product in exact arithmetic (on any leaf, and by symmetry on an R = C leaf in particular): only
# roundings differ, no elementwise bound can tell.  The exchange that reads v_col with the row index and v_row with
# the column index is a different slip, rejected on R != C and on R = C leaves alike, and has lines of its own.
NOT_SEPARABLE = {"adafactor": ["row and column factors exchanged (rcm divides v_col)"], "adam": [], "trace": []}


def _legacy_of(k, o, out, family):
  mx = o.ref.abs().max().item()
  if k == "p":
    return (1e-5, 1e-6) if family != "adafactor" else (0.0, 2e-5 * max(1.0, mx))
  return (0.0, (1e-2 if out.dtype == BF16 else 2e-5) * mx)


def _count(outs, m, family):
  nm = nl = tot = 0
  for k, o in m.items():
    if k in ("stats", "usq", "scale"):
      continue
    out = outs[k].reshape(o.ref.shape)
    leg = _legacy_of(k, o, out, family)
    a = B.count_rejected(out, o.ref, o.bound, leg)
    if o.lo_hi is not None:
      a = max(a, B.count_rejected(out, o.ref, torch.zeros_like(o.ref), None, o.lo_hi))
    nm += a
    nl += B.count_rejected(out, o.ref, leg[1] + leg[0] * o.ref.abs())
    tot += out.numel()
  return nm, nl, tot


def _slip_line(family, slip, counts, separable=True):
  nm = [c[0] for c in counts]; nl = [c[1] for c in counts]
  print(f"[power] {family:10s} {slip:62s} model rejects {nm} / {counts[0][2]}, legacy tolerance alone {nl}"
        + ("" if separable else "   (recorded, not separable)"))
  ROWS.append((family, slip, min(nm), counts[0][2]))
  if separable:
    assert min(nm) > 0, f"{family}: slip '{slip}' passes the model in a seed: {nm}"


def _chain_slip(kind, slip, seed, nesterov=False):
  n, count = 3, 3 * 1024
  segs, chunk_seg, lr_t, wd_t, si_t = OC.seg_setup(n, 3, CPU)
  p, _ = B.opt_inputs(count, CPU, seed)
  acc = B.rnd((count,), CPU, seed + 2, 1e-3).to(BF16)
  nu = B.rnd((count,), CPU, seed + 3, 1e-3) ** 2
  _, g = B.opt_inputs(count, CPU, seed + 10)
  gsq = (g.double() ** 2).sum().reshape(1)
  clip_norm = 0.5 * math.sqrt(gsq.item()) if slip != "clip applied unconditionally" else 2.0 * math.sqrt(gsq.item())
  k = OC.STEPS[0]
  sc_t = torch.tensor(OC.SCHED[0], dtype=F32)[si_t]
  before = dict(p=p.clone(), g=g, mu=acc.clone(), nu=nu.clone(), trace=acc.clone())
  shadow = torch.empty(count, dtype=BF16)
  if kind == "adam":
    hp = dict(OC.ADAM, bc1=1 - 0.9 ** (k + 1), bc2=1 - 0.999 ** (k + 1))
    emu_chain("adam", p, g, acc, nu, shadow, segs, chunk_seg, count, OC.SCHED[0], gsq, clip_norm, None, slip, k=k, **hp)
    m = B.adam_bounds(before["p"], g, before["mu"], before["nu"], lr_t, wd_t, sc_t, gsq.item(), clip_norm, **hp)
    return _count(dict(p=p, mu=acc, nu=nu), m, "adam")
  emu_chain("trace", p, g, acc, None, shadow, segs, chunk_seg, count, OC.SCHED[0], gsq, clip_norm, None, slip, beta=0.9,
            nesterov=nesterov)
  m = B.trace_bounds(before["p"], g, before["trace"], lr_t, wd_t, sc_t, gsq.item(), clip_norm, 0.9, nesterov)
  return _count(dict(p=p, trace=acc), m, "trace")


ADAM_SLIPS = ["eps inside the square root", "eps added before the bc2 division", "bias correction of mu omitted",
              "bias correction of nu omitted", "bc computed for step k rather than k + 1",
              "weight decay not multiplied by the schedule", "weight decay coupled into g before the moments",
              "clip applied unconditionally", "clip applied after the moments", "nu updated with the unclipped g",
              "mu stored by truncation", "update formed from the bf16-rounded mu", "a segment's sched_idx off by one"]
TRACE_SLIPS = [("Nesterov from the rounded t'", True), ("Nesterov as g + beta t_old", True),
               ("mu stored by truncation", False), ("update formed from the bf16-rounded mu", False),
               ("clip applied unconditionally", True), ("clip applied after the moments", False),
               ("weight decay not multiplied by the schedule", True), ("a segment's sched_idx off by one", False)]


def test_adam_and_trace_bounds_bite():
  assert _chain_slip("adam", None, 100)[0] == 0 and _chain_slip("trace", None, 100, True)[0] == 0
  for slip in ADAM_SLIPS:
    _slip_line("adam", slip, [_chain_slip("adam", slip, s) for s in SEEDS])
  for slip, nest in TRACE_SLIPS:
    _slip_line("trace", slip + (" (nesterov)" if nest else ""), [_chain_slip("trace", slip, s, nest) for s in SEEDS])
  assert len(NOT_SEPARABLE["adam"]) <= 2 and len(NOT_SEPARABLE["trace"]) <= 2


def _af_slip(slip, leaf, seed, brc=0.0, want_nonfinite=False):
  spec = next(s for s in B.AF_SPECS if s[0] == leaf)
  lf = OC.af_leaf_record(spec, seed, CPU)
  p, g, state, view = lf["p"], lf["g"], lf["state"], list(lf["view"])
  n = p.numel()
  mom = B.rnd((n,), CPU, seed + 5, 0.3).to(BF16)
  shadow = torch.zeros(n, dtype=BF16)
  gsq = (g.double() ** 2).sum().reshape(1)
  clip_norm = 0.5 * math.sqrt(gsq.item())
  k = OC.STEPS[0]
  decay = OC.af_decay(k)
  hp = dict(OC.AF, decay=decay, lr_eff=lf["lr_eff"], wd=lf["wd"], sched=OC.SCHED[0][0])
  before = dict(p=p.clone(), mom=mom.clone(), state=state.clone())
  _af_leaf_emu(p, g, mom, shadow, view, state, lf["factored"], _clip32(gsq, clip_norm),
               OC.af_decay(k + 1) if slip == "decay of step k + 1 at step k" else decay, 1e-30, 0.9, lf["lr_eff"],
               lf["wd"], hp["sched"], None, slip, block_rms_clip=brc)
  pv, gv, mv = B.af_views([before["p"], g, before["mom"]], view)
  m = B.adafactor_bounds(pv, gv, mv, before["state"], lf["factored"], gsq.item(), clip_norm, block_rms_clip=brc, **hp)
  Bn, R, C = lf["B"], lf["R"], lf["C"]
  pn, mn = B.af_views([p, mom], view)
  outs = dict(p=pn, mom=mn, v_row=state[:Bn * R], v_col=state[Bn * R:Bn * R + Bn * C],
              rcm=state[Bn * R + Bn * C:Bn * R + Bn * C + Bn], v=state[:Bn * R * C])
  if want_nonfinite:
    assert not bool(torch.isfinite(pn).all()), "eps omitted: the zero-gradient row should give a non-finite update"
  return _count(outs, m, "adafactor")


AF_SLIPS = [("rcm omitted", "2x3x32x40-padded", 0.0), ("statistics formed from the unclipped gradient", "2x3x32x40-padded", 0.0),
            ("the mean divided by the wrong extent (R for C)", "2x3x32x40-padded", 0.0),
            ("(1 - momentum) missing", "2x3x32x40-padded", 0.0),
            ("update formed from the bf16-rounded momentum", "2x3x32x40-padded", 0.0),
            ("momentum stored by truncation", "2x3x32x40-padded", 0.0),
            ("weight decay multiplied by lr_eff", "2x3x32x40-padded", 0.0),
            ("block_rms_clip's rms taken per batch slice instead of per leaf", "2x3x32x40-padded", 0.7),
            ("decay of step k + 1 at step k", "2x3x32x40-padded", 0.0),
            ("decay of step k + 1 at step k", "31x500", 0.0), ("statistics formed from the unclipped gradient", "257", 0.0)]


def test_adafactor_bounds_bite():
  for leaf, brc in (("2x3x32x40-padded", 0.0), ("2x3x32x40-padded", 0.7), ("64x64", 0.0), ("31x500", 0.0)):
    assert _af_slip(None, leaf, 100, brc)[0] == 0, leaf
  for slip, leaf, brc in AF_SLIPS:
    _slip_line("adafactor", f"{slip} [{leaf}]", [_af_slip(slip, leaf, s, brc) for s in SEEDS])
  _slip_line("adafactor", "eps omitted [40x48-zero-row-col: non-finite]",
             [_af_slip("eps omitted", "40x48-zero-row-col", s, want_nonfinite=True) for s in SEEDS])
  _slip_line("adafactor", "row and column factors exchanged [32x33]",
             [_af_slip("row and column factors exchanged (R != C)", "32x33", s) for s in SEEDS])
  _slip_line("adafactor", "row and column factors exchanged [64x64, R = C]",
             [_af_slip("row and column factors exchanged", "64x64", s) for s in SEEDS])
  for slip in NOT_SEPARABLE["adafactor"]:
    _slip_line("adafactor", f"{slip} [64x64, R = C]", [_af_slip(slip, "64x64", s) for s in SEEDS], separable=False)
  assert len(NOT_SEPARABLE["adafactor"]) <= 2


def test_gpu_checker_calls_name_the_operand():
  """The GPU file's own checker calls (the drivers of _opt_cases.py) reject an emulated slip with the operand named:
  one slip each for Adam, trace and Adafactor."""
  with pytest.raises(AssertionError, match=r"adam .* p:"):
    OC.chain_case(make_emu("eps inside the square root"), CPU, "adam", 3, 3, 1e-2, F32)
  with pytest.raises(AssertionError, match=r"trace .* p:"):
    OC.chain_case(make_emu("Nesterov from the rounded t'"), CPU, "trace", 2, 2, 1e-2, BF16, nesterov=True)
  with pytest.raises(AssertionError, match=r"adafactor leaf 2x3x32x40-padded .* (p|mom):"):
    OC.af_leaf_case(make_emu("rcm omitted"), CPU, next(s for s in B.AF_SPECS if s[0] == "2x3x32x40-padded"), BF16, 1e-2)
