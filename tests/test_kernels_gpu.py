"""Per-kernel parity tests: every libbvhip entry point (through the C ABI) vs a
plain fp32/fp64 PyTorch statement of the same op on identical inputs.

Tolerances: bf16-input MFMA kernels are compared against fp32 math on the SAME
bf16-rounded inputs, so the only differences are accumulation order and the
final rounding of the output dtype (bf16: 2^-8 relative).  fp32 HBM-bound
kernels: rtol 1e-5 / atol 1e-6.
"""
import math

import pytest
import torch

import _bounds as B

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def rnd(shape, dev, seed, scale=1.0, dtype=F32):
  g = torch.Generator(device="cpu").manual_seed(seed)
  return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dev).to(dtype)


def assert_close(a, b, rtol, atol, name=""):
  a = a.double(); b = b.double()
  err = (a - b).abs()
  tol = atol + rtol * b.abs()
  bad = err > tol
  assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err "
                         f"{err.max().item():.3e} (ref max {b.abs().max().item():.3e})")


# ----------------------------------------------------------------- GEMM ------
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (1568, 768, 768), (130, 136, 72), (5, 8, 8)])
def test_gemm_forward_layout(dev, M, N, K):
  """Y = X W (+bias): A k-major, B k-minor (Flax (in,out) kernel)."""
  from big_vision_amd import ops
  x = rnd((M, K), dev, 0, dtype=BF16)
  w = rnd((K, N), dev, 1, 0.05, dtype=BF16)   # asymmetric: catches transposes
  b = rnd((N,), dev, 2)
  ref = x.double() @ w.double() + b.double()
  y = ops.gemm(x, w, a_kmajor=True, b_kmajor=False, bias=b, out_dtype=F32)
  B.check_gemm(y, ref, x, w, legacy=(1e-4, 1e-3), name="gemm f32")
  y16 = ops.gemm(x, w, a_kmajor=True, b_kmajor=False, bias=b, out_dtype=BF16)
  B.check_gemm(y16, ref, x, w, legacy=(1e-2, 1e-2), name="gemm bf16")


@pytest.mark.parametrize("M,N,K", [(256, 128, 256), (1568, 768, 3072), (77, 64, 128)])
def test_gemm_dx_layout(dev, M, N, K):
  """dX = dY W^T: A k-major, B k-major (W stored [N=in][K=out])."""
  from big_vision_amd import ops
  dy = rnd((M, K), dev, 3, dtype=BF16)
  w = rnd((N, K), dev, 4, 0.05, dtype=BF16)
  ref = dy.double() @ w.double().T
  dx = ops.gemm(dy, w, a_kmajor=True, b_kmajor=True, out_dtype=BF16)
  B.check_gemm(dx, ref, dy, w.T, legacy=(1e-2, 1e-2), name="gemm dx", n_adds=0)


@pytest.mark.parametrize("T,Din,Dout,split", [(512, 128, 256, 0), (1568, 768, 2304, 0), (333, 64, 72, 3), (64, 8, 8, 1)])
def test_gemm_dw_layout(dev, T, Din, Dout, split):
  """dW = X^T dY: both operands k-minor, split-K with fp32 atomics, accumulating."""
  from big_vision_amd import ops
  x = rnd((T, Din), dev, 5, dtype=BF16)
  dy = rnd((T, Dout), dev, 6, dtype=BF16)
  base = rnd((Din, Dout), dev, 7)
  ref = base.double() + x.double().T @ dy.double()
  out = base.clone()
  ops.gemm(x, dy, a_kmajor=False, b_kmajor=False, out=out, epilogue=ops.EPI_ATOMIC, split_k=split)
  # fp32 atomics: the base and every split-K partial are one more fp32 add each
  B.check_gemm(out, ref, x.T, dy, legacy=(1e-4, 1e-4 * math.sqrt(T) * 4), name="gemm dw", n_adds=2 + max(split, 1))


def test_gemm_epilogues(dev):
  from big_vision_amd import ops
  M, N, K, L = 392, 256, 128, 196
  x = rnd((M, K), dev, 8, dtype=BF16)
  w = rnd((K, N), dev, 9, 0.1, dtype=BF16)
  b = rnd((N,), dev, 10)
  pre = x.double() @ w.double() + b.double()
  res = rnd((M, N), dev, 11)
  y = ops.gemm(x, w, bias=b, out_dtype=F32, epilogue=ops.EPI_RESIDUAL, aux=res)
  B.check_gemm(y, pre + res.double(), x, w, legacy=(1e-4, 1e-3), name="residual", n_adds=2)
  resb = res.to(BF16)   # bf16 residual stream: aux and C bf16
  yb = ops.gemm(x, w, bias=b, out_dtype=BF16, epilogue=ops.EPI_RESIDUAL, aux=resb)
  B.check_gemm(yb, pre + resb.double(), x, w, legacy=(1e-2, 1e-2), name="residual (bf16 stream)", n_adds=2)
  pos = rnd((L, N), dev, 12)
  y = ops.gemm(x, w, bias=b, out_dtype=F32, epilogue=ops.EPI_POS, aux=pos, aux_rows=L)
  B.check_gemm(y, pre + pos.double().repeat(M // L, 1), x, w, legacy=(1e-4, 1e-3), name="pos", n_adds=2)
  g = torch.empty((M, N), device=dev, dtype=BF16)
  h = ops.gemm(x, w, bias=b, out_dtype=BF16, epilogue=ops.EPI_GELU, out2=g)
  B.check_gemm(h, pre, x, w, legacy=(1e-2, 1e-2), name="gelu pre")
  # g = gelu of the bf16 h the kernel stored (bv_common.h), checked stage by stage (the check against gelu(pre) stays)
  assert_close(g, B.gelu_tanh64(pre), 1e-2, 1e-2, "gelu out")
  B.check_gelu_g(g, h, legacy=(1e-2, 1e-2), name="gelu out (of the stored h)")
  # the single-output epilogue of a forward that saves no context writes the same activation bits and nothing else
  g1 = ops.gemm(x, w, bias=b, out_dtype=BF16, epilogue=ops.EPI_GELU_G)
  assert torch.equal(g1, g), "BV_EPI_GELU_G differs from the activation BV_EPI_GELU writes"
  # gelu backward epilogue: dH = (dG W2^T) * gelu'(h)
  dg_in = rnd((M, K), dev, 13, dtype=BF16)
  w2 = rnd((N, K), dev, 14, 0.1, dtype=BF16)
  hh = rnd((M, N), dev, 15, dtype=BF16)
  ref = (dg_in.double() @ w2.double().T) * B.dgelu_tanh64(hh)
  out = ops.gemm(dg_in, w2, a_kmajor=True, b_kmajor=True, out_dtype=BF16,
                 epilogue=ops.EPI_GELU_BWD, aux=hh)
  B.check_gelu_bwd(out, dg_in, w2.T, hh, legacy=(1e-2, 2e-2), name="gelu bwd")
  g2 = torch.empty((M, N), device=dev, dtype=BF16)
  out2 = ops.gemm(dg_in, w2, a_kmajor=True, b_kmajor=True, out_dtype=BF16,
                  epilogue=ops.EPI_GELU_BWD_EMIT, aux=hh, out2=g2)
  B.check_gelu_bwd(out2, dg_in, w2.T, hh, legacy=(1e-2, 2e-2), name="gelu bwd (emit)")
  B.check_gelu_g(g2, hh, legacy=(1e-2, 1e-2), name="emitted gelu")
  g3 = torch.empty((M, N), device=dev, dtype=BF16)
  ops.gemm(dg_in, w2, a_kmajor=True, b_kmajor=True, out_dtype=BF16, epilogue=ops.EPI_GELU_BWD_EMIT, aux=h, out2=g3)
  assert torch.equal(g3, g), "gelu(h) re-emitted by the backward differs from the forward's"
  cs = torch.ones((N,), device=dev, dtype=F32)
  ops.gemm(dg_in, w2, a_kmajor=True, b_kmajor=True, out_dtype=BF16, epilogue=ops.EPI_GELU_BWD, aux=hh, colsum=cs)
  assert_close(cs, 1.0 + ref.sum(0), 1e-3, 1e-3 * ref.abs().sum(0).max().item(), "fused colsum")


def test_gemm_rejects_bad_args(dev):
  from big_vision_amd import ops
  x = rnd((16, 12), dev, 0, dtype=BF16)   # K=12 not a multiple of 8
  w = rnd((12, 16), dev, 1, dtype=BF16)
  with pytest.raises(RuntimeError):
    ops.gemm(x, w)
  with pytest.raises(RuntimeError):
    ops.gemm(x.cpu(), w.cpu())


def test_sgemm_strided(dev):
  from big_vision_amd import ops
  M, N, K = 70, 133, 96
  a = rnd((M, K), dev, 1); b = rnd((N, K), dev, 2)
  out = torch.zeros((M, N), device=dev)
  ops.sgemm(a, K, 1, b, 1, K, out, M, N, K, alpha=2.0)       # A B^T
  assert_close(out, 2.0 * a @ b.T, 1e-5, 1e-4, "sgemm NT")
  g = rnd((M, N), dev, 3)
  out2 = torch.zeros((N, K), device=dev)
  ops.sgemm(g, 1, N, a, K, 1, out2, N, K, M)                 # G^T A
  assert_close(out2, g.T @ a, 1e-5, 1e-4, "sgemm TN")


@pytest.mark.parametrize("n,B,E", [(512, 1024, 768), (300, 700, 136), (1024, 1024, 768)])
def test_sgemm_matrix_pipe_equals_the_valu_kernel(dev, n, B, E):
  """The three products of the sigmoid loss (logits = zimg ztxt^T, dzimg = G ztxt, dztxt = G^T zimg) on the fp32 MFMA
  kernel: bit-identical to the VALU kernel (both are k-ordered fmaf chains), and both match fp64."""
  from big_vision_amd import ops, _lib
  lib = _lib.load()
  zi = rnd((n, E), dev, 1); zt = rnd((B, E), dev, 2); G = rnd((n, B), dev, 3, 0.01)
  la = torch.tensor([0.7], device=dev)

  def run():
    raw = torch.empty((n, B), device=dev)
    ops.sgemm(zi, E, 1, zt, 1, E, raw, n, B, E)
    dzi = torch.empty((n, E), device=dev)
    ops.sgemm(G, B, 1, zt, E, 1, dzi, n, E, B, log_alpha=la)
    dzt = torch.full((B, E), 0.5, device=dev)
    ops.sgemm(G, 1, B, zi, E, 1, dzt, B, E, n, alpha=2.0, beta=1.0)
    return raw, dzi, dzt
  new = run()
  with ops.option("sgemm_mfma", 0):
    ref = run()
  for a, b, name in zip(new, ref, ("logits", "dzimg", "dztxt")):
    assert torch.equal(a, b), f"{name}: matrix-pipe kernel differs from the VALU kernel"
  assert_close(new[0], zi.double() @ zt.double().T, 1e-5, 1e-4, "logits vs fp64")
  assert_close(new[1], math.exp(0.7) * (G.double() @ zt.double()), 1e-5, 1e-4, "dzimg vs fp64")
  assert_close(new[2], 0.5 + 2.0 * (G.double().T @ zi.double()), 1e-5, 1e-4, "dztxt vs fp64")


# ------------------------------------------------------------- LayerNorm -----
# (70 001 x 768 fp32 = 215 MB: above the size at which the kernels switch to non-temporal loads, layernorm.hip ln_nt_for)
@pytest.mark.parametrize("rows,D", [(1568, 768), (37, 128), (64, 1024), (9, 384), (70001, 768)])
def test_layernorm(dev, rows, D):
  from big_vision_amd import ops
  x = rnd((rows, D), dev, 1, 2.0) + 0.5
  scale = 1 + 0.1 * rnd((D,), dev, 2); bias = 0.1 * rnd((D,), dev, 3)
  xr = x.double().requires_grad_(True); sr = scale.double().requires_grad_(True)
  br = bias.double().requires_grad_(True)
  ref = torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6)
  y_bf, y_f, mean, rstd = ops.layernorm_fwd(x, scale, bias, rows=rows, D=D, want_f32=True)
  B.check_ln_fwd(y_f, x, scale, bias, legacy=(1e-5, 1e-5), name="ln fwd f32")
  B.check_ln_fwd(y_bf, x, scale, bias, legacy=(1e-2, 1e-2), name="ln fwd bf16")
  dy = rnd((rows, D), dev, 4)
  dres = rnd((rows, D), dev, 5)
  ref.backward(dy.double())
  dscale = torch.zeros(D, device=dev); dbias = torch.zeros(D, device=dev)
  dx_bf = torch.empty((rows, D), device=dev, dtype=BF16)
  dxsum = torch.ones(D, device=dev)          # accumulated (+=) into
  dx = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres, dx_bf16=dx_bf,
                         dscale=dscale, dbias=dbias, dx_colsum=dxsum)
  B.check_ln_bwd(dx, x, scale, dy, dres=dres, legacy=(1e-4, 1e-4), name="ln dx")
  assert_close(dxsum, 1.0 + dx.double().sum(0), 1e-4, 1e-3, "ln dx colsum (fused bias grad)")
  B.check_ln_bwd(dx_bf, x, scale, dy, dres=dres, legacy=(1e-2, 1e-2), name="ln dx bf16")
  assert_close(dscale, sr.grad, 1e-4, 1e-3, "ln dscale")
  assert_close(dbias, br.grad, 1e-4, 1e-3, "ln dbias")
  # bv_layernorm_bwd_y: the same backward that also re-emits the forward's bf16 output (light contexts):
  # y bit-identical to bv_layernorm_fwd's, every other output bit-identical to the plain backward
  y_re = torch.zeros((rows, D), device=dev, dtype=BF16)
  dx_bf2 = torch.empty((rows, D), device=dev, dtype=BF16)
  dx_y = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres, dx_bf16=dx_bf2, bias=bias, y_out=y_re)
  assert torch.equal(y_re, y_bf), "re-emitted LayerNorm output differs from the forward's"
  assert torch.equal(dx_y, dx) and torch.equal(dx_bf2, dx_bf)
  # bf16 upstream gradient variant
  dyb = dy.to(BF16)
  dx2 = ops.layernorm_bwd(dyb, x, scale, mean, rstd, rows=rows, D=D)
  xr.grad = None
  torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6).backward(dyb.double())
  B.check_ln_bwd(dx2, x, scale, dyb, legacy=(1e-4, 1e-4), name="ln dx (bf16 dy)")
  # rows of std 1e-2 / 1e-3 (pin eps) and |mean| / std = 4 (fast-variance cancellation), in launches of their own
  # that fuse no column sums (_bounds.check_ln_edge_launch)
  B.check_ln_edge_launch(ops, x, scale, bias, (dy, dyb), dres=dres)


@pytest.mark.parametrize("rows,D", [(1568, 768), (37, 128), (64, 1024), (9, 384), (5, 1152), (3, 2048)])
def test_layernorm_bf16_stream(dev, rows, D):
  """bv_layernorm_fwd_bf16x / bv_layernorm_bwd_bf16x: x, dres, dx in bf16 (config.residual_stream =
  "bfloat16"), arithmetic and statistics fp32 - against fp64 LayerNorm of the same bf16 inputs."""
  from big_vision_amd import ops
  x = (rnd((rows, D), dev, 1, 2.0) + 0.5).to(BF16)
  scale = 1 + 0.1 * rnd((D,), dev, 2); bias = 0.1 * rnd((D,), dev, 3)
  xr = x.double().requires_grad_(True); sr = scale.double().requires_grad_(True)
  br = bias.double().requires_grad_(True)
  ref = torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6)
  y_bf, y_f, mean, rstd = ops.layernorm_fwd(x, scale, bias, rows=rows, D=D, want_f32=True)
  B.check_ln_fwd(y_f, x, scale, bias, legacy=(1e-5, 1e-5), name="ln fwd f32 (bf16 x)")
  B.check_ln_fwd(y_bf, x, scale, bias, legacy=(1e-2, 1e-2), name="ln fwd bf16 (bf16 x)")
  assert_close(mean, xr.mean(-1), 1e-5, 1e-5, "mean")
  for dy in (rnd((rows, D), dev, 4), rnd((rows, D), dev, 4).to(BF16)):
    dres = rnd((rows, D), dev, 5).to(BF16)
    xr.grad = sr.grad = br.grad = None
    torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6).backward(dy.double())
    dscale = torch.zeros(D, device=dev); dbias = torch.zeros(D, device=dev)
    dxsum = torch.ones(D, device=dev)
    dx = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres, dscale=dscale, dbias=dbias,
                           dx_colsum=dxsum)
    assert dx.dtype == BF16
    want = xr.grad + dres.double()
    B.check_ln_bwd(dx, x, scale, dy, dres=dres, legacy=(1e-2, 1e-2), name="ln dx (bf16 stream)")
    assert_close(dxsum, 1.0 + want.sum(0), 1e-4, 1e-3, "ln dx colsum is summed in fp32, before the rounding")
    assert_close(dscale, sr.grad, 1e-4, 1e-3, "ln dscale")
    assert_close(dbias, br.grad, 1e-4, 1e-3, "ln dbias")
  # no residual gradient, strided rows (encoder_norm on the pooled token)
  n, L = 3, rows // 3 if rows >= 3 else 1
  if L >= 1 and n * L <= rows:
    _, y, mean, rstd = ops.layernorm_fwd(x, scale, bias, rows=n, D=D, row_stride=L, row_offset=L - 1,
                                         want_bf16=False, want_f32=True)
    sel = x[:n * L].view(n, L, D)[:, -1].double()
    B.check_ln_fwd(y, sel, scale, bias, legacy=(1e-5, 1e-5), name="strided ln (bf16 x)")
    dy = rnd((n, D), dev, 6)
    dxs = ops.layernorm_bwd(dy, x[:n * L].contiguous(), scale, mean, rstd, rows=n, D=D, row_stride=L, row_offset=L - 1)
    xq = x[:n * L].double().requires_grad_(True)
    torch.nn.functional.layer_norm(xq.view(n, L, D)[:, -1], (D,), scale.double(), bias.double(), eps=1e-6).backward(dy.double())
    assert_close(dxs, xq.grad, 1e-2, 1e-2, "strided ln bwd (bf16 stream): other rows stay 0")
    B.check_ln_bwd(dxs.view(n, L, D)[:, -1], sel, scale, dy, legacy=(1e-2, 1e-2), name="strided ln bwd (bf16 stream)")
  # the edge rows, including the rows the strided launch selects, in launches without fused column sums
  dy32 = rnd((rows, D), dev, 4)
  B.check_ln_edge_launch(ops, x, scale, bias, (dy32, dy32.to(BF16)), dres=rnd((rows, D), dev, 5).to(BF16),
                         strided=(n, L, L - 1), idx=sorted(set(B.LN_EDGE_IDX) | {L - 1, 2 * L - 1, 3 * L - 1}))


def test_cast_f32(dev):
  from big_vision_amd import ops
  for count in (8, 4096, 1000003 // 8 * 8, 24):
    x = rnd((count,), dev, 9).to(BF16)
    assert torch.equal(ops.cast_f32(x), x.float())


def test_layernorm_strided_rows(dev):
  """encoder_norm applied to the pooled (last) token only."""
  from big_vision_amd import ops
  n, L, D = 6, 16, 128
  x = rnd((n * L, D), dev, 1)
  scale = 1 + 0.1 * rnd((D,), dev, 2); bias = 0.1 * rnd((D,), dev, 3)
  _, y, mean, rstd = ops.layernorm_fwd(x, scale, bias, rows=n, D=D, row_stride=L, row_offset=L - 1,
                                       want_bf16=False, want_f32=True)
  sel = x.view(n, L, D)[:, -1]
  B.check_ln_fwd(y, sel, scale, bias, legacy=(1e-5, 1e-5), name="strided ln")
  dy = rnd((n, D), dev, 4)
  dxsum = torch.zeros(D, device=dev)
  dx = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=n, D=D, row_stride=L, row_offset=L - 1,
                         dx_colsum=dxsum)
  assert_close(dxsum, dx.double().sum(0), 1e-4, 1e-4, "strided ln dx colsum")
  xr = x.clone().requires_grad_(True)
  torch.nn.functional.layer_norm(xr.view(n, L, D)[:, -1], (D,), scale, bias, eps=1e-6).backward(dy)
  assert_close(dx, xr.grad, 1e-4, 1e-5, "strided ln bwd")
  B.check_ln_bwd(dx.view(n, L, D)[:, -1], sel, scale, dy, legacy=(1e-4, 1e-5), name="strided ln bwd")
  # all six selected rows as edge rows, in launches without the fused column sums
  B.check_ln_edge_launch(ops, x, scale, bias, (rnd((n * L, D), dev, 4),), strided=(n, L, L - 1),
                         idx=[L - 1 + i * L for i in range(n)])


# ------------------------------------------------------------- Attention -----
def _attn_ref(qkv, n, L, H):
  q, k, v = qkv.double().view(n, L, 3, H, 64).unbind(2)
  s = torch.einsum("nqhd,nkhd->nhqk", q / 8.0, k)
  p = torch.softmax(s, -1)
  o = torch.einsum("nhqk,nkhd->nqhd", p, v)
  return o.reshape(n * L, H * 64), torch.logsumexp(s, -1)


@pytest.mark.parametrize("n,L,H", [(3, 196, 2), (2, 64, 3), (2, 5, 1), (1, 197, 2), (1, 441, 1), (1, 576, 1),
                                   (2, 224, 1), (1, 33, 2), (2, 257, 1), (3, 208, 1), (2, 272, 2)])
def test_attention(dev, n, L, H):
  """The Dh = 64 kernels behind bv_attn_fwd / bv_attn_bwd (attention3.hip, attention5.hip) vs fp64.  (Rounds 1-4 ran
  the same cases on two superseded kernel sets as well; those left the library in round 5.)"""
  _attention_case(dev, n, L, H)


@pytest.mark.parametrize("n,L,H", [(4, 196, 2), (3, 64, 1), (2, 441, 1), (3, 256, 2)])
def test_attention_key_padding_mask(dev, n, L, H):
  """bv_attn_fwd/bwd_masked (NaFlex, naflex_vit.py:84-293: mask = valid patches, padding at the end)
  vs fp64 torch attention with the same key-padding mask; dK / dV of masked keys are exactly 0."""
  from big_vision_amd import ops
  qkv = rnd((n * L, 3 * H * 64), dev, 5, 1.5, dtype=BF16)
  lens = [L, max(1, L // 3), L - 1, 17][:n]
  kv_len = torch.tensor(lens, device=dev, dtype=torch.int32)
  o, lse = ops.attn_fwd(qkv, n, L, H, kv_len=kv_len)
  B.check_attn_fwd(o, lse, qkv, n, L, H, 64, lens, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3), name="masked attn")
  d_o = rnd((n * L, H * 64), dev, 6, dtype=BF16)
  db = torch.zeros((3 * H * 64,), device=dev)
  delta = torch.full((n, H, L), float("nan"), device=dev)
  dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len, dbias=db, delta=delta)
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, 64, lens, legacy=3e-2, delta=delta, dbias=db, legacy_db=2e-2,
                   name="masked attn")
  dk = dqkv.view(n, L, 3, H, 64)[:, :, 1:]
  for i, ln in enumerate(lens):
    assert (dk[i, ln:] == 0).all(), "masked keys must get zero dK / dV"
  # no mask given == plain attention
  o2, lse2 = ops.attn_fwd(qkv, n, L, H, kv_len=torch.full((n,), L, device=dev, dtype=torch.int32))
  o3, lse3 = ops.attn_fwd(qkv, n, L, H)
  # (the unmasked launch takes the tail-only instantiation: same values, another summation order)
  assert_close(lse2, lse3, 1e-6, 1e-5, "full-length mask lse")
  assert_close(o2, o3, 8e-3, 1e-3, "full-length mask out")


def test_attention_delta_is_exact_for_near_uniform_rows(dev):
  """Repeated keys / tiny logits (random init, sticky-EOS padding): dP - delta cancels to a fraction
  of delta.  attention3 computes delta = rowsum(P o dP) in fp32; rowsum(dO o O) with the bf16 O
  (the round-2 kernels, attention2.hip) loses the q / k gradients there.  Measured against fp64 on the same bf16 inputs."""
  from big_vision_amd import ops, _lib
  n, L, H = 2, 64, 2
  base = rnd((n, 1, 3 * H * 64), dev, 9, 1.0)
  qkv = (base + 0.02 * rnd((n, L, 3 * H * 64), dev, 10)).reshape(n * L, -1)
  qkv[:, :H * 64] *= 0.1            # small queries: nearly uniform attention
  qkv = qkv.to(BF16)
  qr = qkv.double().requires_grad_(True)
  o_ref, _ = _attn_ref(qr, n, L, H)
  d_o = rnd((n * L, H * 64), dev, 11, dtype=BF16)
  o_ref.backward(d_o.double())
  g = qr.grad.view(n * L, 3, H * 64)
  o, lse = ops.attn_fwd(qkv, n, L, H)
  dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H)
  # (the cancellation dP - delta is what the model's e_delta term pays for; exempt from the 1 % legacy-cap share, which
  #  the [bounds] lines print)
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, 64, legacy=3e-2, name="near-uniform attn")
  d = dqkv.double().view(n * L, 3, H * 64)
  rel = [((d[:, j] - g[:, j]).norm() / g[:, j].norm()).item() for j in range(3)]
  print("rel-L2 of dq/dk/dv:", rel)
  # measured on MI355X: dq 0.079 / dk 0.0023 / dv 0.0023; the rowsum(dO o O) shortcut with the bf16 O (the round-2
  # kernels) gave dq 32 (!) / dk 0.036 on the same inputs
  assert rel[0] <= 0.15 and rel[1] <= 1e-2 and rel[2] <= 1e-2, rel


def _attention_case(dev, n, L, H):
  from big_vision_amd import ops
  qkv = rnd((n * L, 3 * H * 64), dev, 1, 1.5, dtype=BF16)
  o, lse = ops.attn_fwd(qkv, n, L, H)
  B.check_attn_fwd(o, lse, qkv, n, L, H, 64, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3))
  d_o = rnd((n * L, H * 64), dev, 2, dtype=BF16)
  dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H)
  # fused q/k/v bias gradient: column sums of dqkv, accumulated in place
  db = torch.full((3 * H * 64,), 0.5, device=dev)
  delta = torch.full((n, H, L), float("nan"), device=dev)
  dqkv2 = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, dbias=db, delta=delta)
  assert torch.equal(dqkv2, dqkv)
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, 64, legacy=3e-2, delta=delta, dbias=db, dbias_base=0.5, legacy_db=2e-2)


@pytest.mark.parametrize("n,L,H", [(48, 196, 12), (40, 197, 12), (160, 64, 12), (30, 208, 4), (300, 33, 3)])
def test_attention_one_launch_backward_walks_many_pairs(dev, n, L, H):
  """attention5.hip (the backward in one launch: persistent workgroups, loader waves prefetching the next
  (sample, head) pair) on more pairs than workgroups, so every workgroup walks 2-3 pairs: vs fp64 on the same
  bf16 inputs, vs the two-launch kernels of attention3.hip (BV_OPT_ATTN_CFG bit 128), run-to-run bit-equal (the delta
  partials are summed in a fixed order), and the fused q/k/v bias gradients."""
  from big_vision_amd import ops, _lib
  lib = _lib.load()
  qkv = rnd((n * L, 3 * H * 64), dev, 21, 1.5, dtype=BF16)
  d_o = rnd((n * L, H * 64), dev, 22, dtype=BF16)
  o, lse = ops.attn_fwd(qkv, n, L, H)
  b5 = B.attn_bwd_bounds(qkv, d_o, n, L, H, 64)
  assert b5.path == "attn5"
  g = b5.g
  db = torch.zeros((3 * H * 64,), device=dev)
  d5 = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, dbias=db)
  d5b = ops.attn_bwd(qkv, o, d_o, lse, n, L, H)
  assert torch.equal(d5, d5b), "run-to-run / dbias-variant difference"
  old = ops.ctx_get("attn_cfg")
  with ops.option("attn_cfg", old | 128):
    db3 = torch.zeros((3 * H * 64,), device=dev)
    delta3 = torch.full((n, H, L), float("nan"), device=dev)
    d3 = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, dbias=db3, delta=delta3)
  B.check_attn_bwd(d5, qkv, d_o, n, L, H, 64, legacy=3e-2, dbias=db, legacy_db=2e-2, bounds=b5,
                   name="one-launch (identities)")
  B.check_attn_bwd(d3, qkv, d_o, n, L, H, 64, legacy=3e-2, delta=delta3, dbias=db3, legacy_db=2e-2,
                   path=B.attn_bwd_path(L, 64, False, one_launch=False), name="two-launch")
  gv = g.view(n * L, 3, H * 64)
  for j, name in enumerate(("dq", "dk", "dv")):
    r5 = ((d5.double().view(n * L, 3, -1)[:, j] - gv[:, j]).norm() / gv[:, j].norm()).item()
    r3 = ((d3.double().view(n * L, 3, -1)[:, j] - gv[:, j]).norm() / gv[:, j].norm()).item()
    print(f"rel-L2 {name}: one launch {r5:.5f}, two launches {r3:.5f}")
    assert r5 <= max(1.15 * r3, 6e-3), (name, r5, r3)
  cs = g.sum(0)
  # the bias gradients came from the identities (attention5.hip BM = 2 for L % 16 != 0, BM = 3 otherwise): same
  # again by DPP column sums of dq / dk / dv (BM = 1)
  with ops.option("attn_cfg", old | 256):
    dbd = torch.zeros((3 * H * 64,), device=dev)
    d5d = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, dbias=dbd)
  assert torch.equal(d5d, d5)
  B.check_attn_bwd(d5d, qkv, d_o, n, L, H, 64, legacy=3e-2, dbias=dbd, legacy_db=2e-2, bounds=b5,
                   name="one-launch (DPP column sums)")
  for j, name in enumerate(("q", "k", "v")):
    sl = slice(j * H * 64, (j + 1) * H * 64)
    e_id = (db[sl].double() - cs[sl]).norm().item(); e_cs = (dbd[sl].double() - cs[sl]).norm().item()
    print(f"{name}-bias gradient: |err| identities {e_id:.3e}, column sums {e_cs:.3e}, |ref| {cs[sl].norm().item():.3e}")


@pytest.mark.parametrize("L", [196, 197, 33, 64])
def test_attention_backward_with_hugely_negative_scores(dev, L):
  """Every score of a row around -250 (lse ~ -245): exp2(-lse) of a PADDED key (k = v = 0, S = 0) would be 2^353 =
  inf.  The one-launch backward masks padded keys through the accumulator init of S^T (attention5.hip), so it stays
  finite and exact for any lse; checked against fp64."""
  from big_vision_amd import ops
  n, H = 3, 2
  u = rnd((1, 64), dev, 31)
  u = u / u.norm() * 32.0
  q = -2.0 * u + 0.05 * rnd((n * L, H, 64), dev, 32)          # q . k / 8 ~ -256 for every key
  k = u + 0.05 * rnd((n * L, H, 64), dev, 33)
  v = rnd((n * L, H, 64), dev, 34)
  qkv = torch.stack([q, k, v], 1).reshape(n * L, 3 * H * 64).to(BF16)
  o_ref, lse_ref = _attn_ref(qkv, n, L, H)
  assert lse_ref.max().item() < -150
  o, lse = ops.attn_fwd(qkv, n, L, H)
  assert_close(lse, lse_ref, 1e-4, 5e-2, "lse")
  d_o = rnd((n * L, H * 64), dev, 35, dtype=BF16)
  db = torch.zeros((3 * H * 64,), device=dev)
  dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, dbias=db)
  assert torch.isfinite(dqkv.float()).all() and torch.isfinite(db).all()
  # (exempt from the 1 % legacy-cap share; the [bounds] lines print it)
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, 64, legacy=5e-2, name="attn at lse ~ -245")


def test_attention_peaked_softmax(dev):
  """One key dominates each row (large logits): exercises the max-subtraction."""
  from big_vision_amd import ops
  n, L, H = 1, 196, 1
  qkv = rnd((n * L, 3 * 64), dev, 3, 1.0, dtype=BF16).float()
  qkv[:, :64] *= 8.0
  qkv[7, 64:128] *= 10.0
  qkv = qkv.to(BF16)
  o_ref, lse_ref = _attn_ref(qkv, n, L, H)
  o, lse = ops.attn_fwd(qkv, n, L, H)
  assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
  B.check_attn_fwd(o, lse, qkv, n, L, H, 64, legacy_o=(3e-2, 3e-2), legacy_lse=(1e-3, 1e-2), name="attn peaked")


@pytest.mark.parametrize("n,L,H", [(4, 196, 2), (3, 16, 1), (5, 70, 3)])
def test_map_attention(dev, n, L, H):
  from big_vision_amd import ops
  q = rnd((n, H * 64), dev, 1, dtype=BF16)
  kv = rnd((n * L, 2 * H * 64), dev, 2, dtype=BF16)
  o, pp = ops.map_attn_fwd(q, kv, n, L, H)
  B.check_map_attn_fwd(o, pp, q, kv, n, L, H, 64, legacy_p=(1e-3, 1e-5), legacy_o=(1e-2, 1e-2))
  d_o = rnd((n, H * 64), dev, 3, dtype=BF16)
  dq, dkv = ops.map_attn_bwd(q, kv, pp, d_o, n, L, H)
  B.check_map_attn_bwd(dq, dkv, q, kv, d_o, n, L, H, 64, legacy=2e-2)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,L,H,Dh", [(2, 256, 2, 72), (3, 64, 2, 16), (1, 300, 1, 128), (2, 729, 1, 72),
                                       (3, 33, 2, 32), (2, 196, 3, 80), (2, 5, 1, 8), (1, 1000, 1, 64),
                                       (2, 100, 2, 104)])
def test_attention_other_head_dims(dev, n, L, H, Dh, masked):
  """bv_attn_fwd_dh / bv_attn_bwd_dh (attention_dh.hip): head dims of So400m (72), `mu` (16), H (80),
  G (104) ... and sequences beyond the LDS-resident kernels' 576 (Dh = 64 at L = 1000), with and without
  key-padding lengths, vs fp64 torch attention; per-sample bias-gradient rows through the colsum."""
  from big_vision_amd import ops
  qkv = rnd((n * L, 3 * H * Dh), dev, 11, 1.5, dtype=BF16)
  lens = [L, max(1, L // 3), L - 1][:n] if masked else [L] * n
  kv_len = torch.tensor(lens, device=dev, dtype=torch.int32) if masked else None
  o, lse = ops.attn_fwd(qkv, n, L, H, kv_len=kv_len)
  assert o.shape == (n * L, H * Dh)
  B.check_attn_fwd(o, lse, qkv, n, L, H, Dh, lens if masked else None, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3))
  d_o = rnd((n * L, H * Dh), dev, 12, dtype=BF16)
  db = torch.full((3 * H * Dh,), 0.25, device=dev)
  delta = torch.full((n, H, L), float("nan"), device=dev)
  dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len, dbias=db, delta=delta)
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, Dh, lens if masked else None, legacy=3e-2, delta=delta, dbias=db,
                   dbias_base=0.25, legacy_db=2e-2)
  dkv = dqkv.view(n, L, 3, H, Dh)[:, :, 1:]
  for i, ln in enumerate(lens):
    assert (dkv[i, ln:] == 0).all(), "masked keys must get zero dK / dV"
  # run-to-run bit-equality of everything but the atomically summed bias rows
  o2, lse2 = ops.attn_fwd(qkv, n, L, H, kv_len=kv_len)
  assert torch.equal(o, o2) and torch.equal(lse, lse2)
  assert torch.equal(dqkv, ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len))


@pytest.mark.parametrize("n,L,H,Dh", [(4, 256, 2, 72), (3, 16, 2, 16), (2, 70, 1, 128), (2, 3000, 1, 64)])
def test_map_attention_other_head_dims(dev, n, L, H, Dh):
  from big_vision_amd import ops
  q = rnd((n, H * Dh), dev, 1, dtype=BF16)
  kv = rnd((n * L, 2 * H * Dh), dev, 2, dtype=BF16)
  ll = [L, max(1, L // 2), L - 1, 1][:n]
  lens = torch.tensor(ll, device=dev, dtype=torch.int32)
  o, pp = ops.map_attn_fwd(q, kv, n, L, H, kv_len=lens)
  B.check_map_attn_fwd(o, pp, q, kv, n, L, H, Dh, ll, legacy_p=(1e-3, 1e-5), legacy_o=(1e-2, 1e-2))
  d_o = rnd((n, H * Dh), dev, 3, dtype=BF16)
  dq, dkv = ops.map_attn_bwd(q, kv, pp, d_o, n, L, H)
  B.check_map_attn_bwd(dq, dkv, q, kv, d_o, n, L, H, Dh, ll, legacy=2e-2)


# ------------------------------------ inputs the flat tolerance hid ----------
def _scaled_heads(dev, n, L, H, Dh, seed):
  """Head h's dO scaled by 100^-h, sample 1's qkv by 0.25: under one tensor-wide max|g| the small heads / the flat
  sample were never checked at their own scale."""
  qkv = rnd((n, L, 3 * H * Dh), dev, seed, 1.5)
  qkv[1] *= 0.25
  d_o = rnd((n * L, H, Dh), dev, seed + 1)
  d_o *= torch.tensor([100.0 ** -h for h in range(H)], device=dev)[None, :, None]
  return qkv.reshape(n * L, 3 * H * Dh).to(BF16), d_o.reshape(n * L, H * Dh).to(BF16)


@pytest.mark.parametrize("L,Dh,masked", [(64, 64, False), (196, 64, False), (257, 64, False), (441, 64, False),
                                         (196, 64, True), (100, 72, False)],
                         ids=["attn5-L64", "attn5-L196", "dq1+dkv-L257", "dq1+dkv32-L441", "masked-L196", "adh-Dh72-L100"])
def test_attention_backward_heads_and_samples_at_different_scales(dev, L, Dh, masked):
  """dq / dk / dv, delta and the bias gradients (the k-bias gradient against its fp64 reference ~ 0 and the model's
  bound) with gradients spanning four orders of magnitude across heads and a near-uniform sample."""
  from big_vision_amd import ops
  n, H = 3, 3
  qkv, d_o = _scaled_heads(dev, n, L, H, Dh, 41)
  lens = [L, max(1, L // 4), L - 1] if masked else None
  kv_len = torch.tensor(lens, device=dev, dtype=torch.int32) if masked else None
  o, lse = ops.attn_fwd(qkv, n, L, H, kv_len=kv_len)
  B.check_attn_fwd(o, lse, qkv, n, L, H, Dh, lens, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3))
  db = torch.zeros((3 * H * Dh,), device=dev)
  delta = torch.full((n, H, L), float("nan"), device=dev)
  dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len, dbias=db, delta=delta)
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, Dh, lens, legacy=3e-2, delta=delta, dbias=db, legacy_db=2e-2,
                   name="scaled heads")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Dh", [64, 72])
def test_map_attention_heads_at_different_scales(dev, Dh, masked):
  from big_vision_amd import ops
  n, L, H = 3, 70, 3
  q = rnd((n, H * Dh), dev, 43, dtype=BF16)
  kv = rnd((n * L, 2 * H * Dh), dev, 44, dtype=BF16)
  d_o = rnd((n, H, Dh), dev, 45) * torch.tensor([100.0 ** -h for h in range(H)], device=dev)[None, :, None]
  d_o = d_o.reshape(n, H * Dh).to(BF16)
  ll = [L, L // 2, L - 1] if masked else None
  kv_len = torch.tensor(ll, device=dev, dtype=torch.int32) if masked else None
  o, pp = ops.map_attn_fwd(q, kv, n, L, H, kv_len=kv_len)
  B.check_map_attn_fwd(o, pp, q, kv, n, L, H, Dh, ll, name="map scaled heads")
  dq, dkv = ops.map_attn_bwd(q, kv, pp, d_o, n, L, H)
  B.check_map_attn_bwd(dq, dkv, q, kv, d_o, n, L, H, Dh, ll, legacy=2e-2, name="map scaled heads")


# ----------------------------------------------------------- data movers -----
@pytest.mark.parametrize("P,res", [(16, 64), (8, 32), (14, 28)])
def test_patchify(dev, P, res):
  import bv_oracle as O
  from big_vision_amd import ops
  img = torch.rand((3, res, res, 3), device=dev) * 2 - 1
  ref, (h, w) = O.extract_patches(img.cpu(), (P, P))
  out, hw = ops.patchify(img, P)
  assert hw == (h, w)
  K = P * P * 3   # rows are padded with zeros to a multiple of 8 columns (14 x 14 x 3 = 588 -> 592)
  assert out.shape[1] == (K + 7) // 8 * 8
  assert torch.equal(out.cpu()[:, :K], ref.reshape(-1, K).to(BF16))
  assert (out[:, K:] == 0).all()


def test_embed(dev):
  from big_vision_amd import ops
  n, L, D, V = 5, 16, 128, 50
  g = torch.Generator().manual_seed(0)
  ids = torch.randint(0, V, (n, L), generator=g, dtype=torch.int32)
  ids[:, 10:] = 1  # heavy duplicates (sticky EOS)
  ids = ids.to(dev)
  table = rnd((V, D), dev, 1); pos = rnd((L, D), dev, 2)
  x = ops.embed_fwd(ids, table, pos, n, L)
  ref = table[ids.long().view(-1)] + pos.repeat(n, 1)
  assert torch.equal(x, ref)
  dx = rnd((n * L, D), dev, 3)
  dt = torch.zeros((V, D), device=dev)
  ops.embed_bwd(ids.view(-1), dx, dt)
  ref_dt = torch.zeros((V, D), device=dev, dtype=torch.float64).index_add_(0, ids.long().view(-1), dx.double())
  assert_close(dt, ref_dt, 1e-5, 1e-5, "embed bwd")
  # several workgroup chunks, ragged tail, D > one pass of the workgroup, out-of-range ids clamp
  n, L, D, V = 7, 37, 1536, 23
  ids = torch.randint(0, V, (n, L), generator=g, dtype=torch.int32)
  ids[:, 20:] = 1
  ids[0, 0] = -5; ids[1, 1] = V + 3
  ids = ids.to(dev)
  dx = rnd((n * L, D), dev, 4)
  dt = torch.zeros((V, D), device=dev)
  ops.embed_bwd(ids.view(-1), dx, dt)
  idc = ids.long().view(-1).clamp(0, V - 1)
  ref_dt = torch.zeros((V, D), device=dev, dtype=torch.float64).index_add_(0, idc, dx.double())
  assert_close(dt, ref_dt, 1e-5, 1e-4, "embed bwd (chunks)")


def test_reductions_and_casts(dev):
  from big_vision_amd import ops
  rows, cols = 3000, 200
  x = rnd((rows, cols), dev, 1)
  out = torch.ones(cols, device=dev)
  ops.colsum(x, out)
  assert_close(out, 1 + x.double().sum(0), 1e-5, 1e-3, "colsum f32")
  xb = x.to(BF16)
  out = torch.zeros(cols, device=dev)
  ops.colsum(xb, out)
  assert_close(out, xb.double().sum(0), 1e-5, 1e-3, "colsum bf16")
  # strided view (columns of a wider matrix)
  wide = rnd((rows, 3 * cols), dev, 2).to(BF16)
  out = torch.zeros(cols, device=dev)
  ops.colsum(wide[:, cols:2 * cols], out)
  assert_close(out, wide[:, cols:2 * cols].double().sum(0), 1e-5, 1e-3, "colsum view")
  n, L, D = 70, 9, 32
  y = rnd((n, L, D), dev, 3)
  acc = torch.zeros((L, D), device=dev)
  ops.batchsum(y, acc, n, L, D)
  assert_close(acc, y.double().sum(0), 1e-5, 1e-4, "batchsum")
  z = rnd((1000003,), dev, 4)
  assert torch.equal(ops.cast_bf16(z), z.to(BF16))
  cls = rnd((D,), dev, 5)
  cat = ops.concat_cls(cls, y.view(n * L, D), n, L, D).view(n, L + 1, D)
  assert torch.equal(cat[:, 0], cls.expand(n, D)) and torch.equal(cat[:, 1:], y)
  gp = ops.pool_gap_fwd(y.view(n * L, D), n, L, D)
  assert_close(gp, y.mean(1), 1e-5, 1e-6, "gap")
  gb = ops.pool_gap_bwd(gp, n, L, D).view(n, L, D)
  assert_close(gb, (gp / L)[:, None, :].expand(n, L, D), 1e-6, 1e-7, "gap bwd")


def test_l2norm(dev):
  from big_vision_amd import ops
  z = rnd((33, 768), dev, 1, 3.0)
  zr = z.double().requires_grad_(True)
  nr = torch.linalg.norm(zr, dim=1, keepdim=True)
  ref = zr / (nr + 1e-8)
  zn, norm = ops.l2norm_fwd(z)
  assert_close(zn, ref, 1e-5, 1e-6, "l2norm")
  assert_close(norm, nr[:, 0], 1e-5, 1e-6, "norm")
  g = rnd((33, 768), dev, 2)
  ref.backward(g.double())
  dz = ops.l2norm_bwd(z, norm, g)
  assert_close(dz, zr.grad, 1e-4, 1e-6, "l2norm bwd")


# ------------------------------------------------------------------ loss -----
@pytest.mark.parametrize("n,B,off,t0,b0", [(64, 64, 0, 10.0, -10.0), (48, 192, 96, 10.0, -2.71), (7, 21, 14, 3.0, 0.5)])
def test_siglip_loss_kernel_vs_oracle(dev, n, B, off, t0, b0):
  import bv_oracle as O
  from big_vision_amd import ops
  zi = torch.nn.functional.normalize(rnd((n, 32), dev, 1), dim=1)
  zt = torch.nn.functional.normalize(rnd((B, 32), dev, 2), dim=1)
  zt[off:off + n] = 0.7 * zt[off:off + n] + 0.3 * zi  # make positives informative
  tp = torch.tensor([math.log(t0)], device=dev); bp = torch.tensor([b0], device=dev)
  # oracle: rows [off, off+n) of the global loss (siglip.py:291-306), fp64
  zi_all = torch.zeros((B, 32), dtype=torch.float64); zi_all[off:off + n] = zi.double().cpu()
  zid = zi.double().cpu().requires_grad_(True); ztd = zt.double().cpu().requires_grad_(True)
  tpd = tp.double().cpu().requires_grad_(True); bpd = bp.double().cpu().requires_grad_(True)
  logits = zid @ ztd.T * torch.exp(tpd) + bpd
  m = -torch.ones_like(logits); m[torch.arange(n), off + torch.arange(n)] = 1.0
  loss_ref = (-O.log_sigmoid(m * logits).sum(-1)).sum() / B
  loss_ref.backward()
  raw = torch.zeros((n, B), device=dev)
  ops.sgemm(zi, 32, 1, zt, 1, 32, raw, n, B, 32)
  stats = torch.zeros(3, device=dev, dtype=torch.float64)
  ops.siglip_loss_(raw, tp, bp, stats, off, B)
  t = math.exp(tp.item())
  assert_close(stats[0].cpu(), loss_ref.detach(), 1e-5, 1e-6, "loss")
  assert_close(stats[1].cpu(), tpd.grad[0], 1e-4, 1e-6, "dt'")
  assert_close(stats[2].cpu(), bpd.grad[0], 1e-4, 1e-6, "db")
  dzi = t * raw.double().cpu() @ ztd.detach()
  dzt = t * raw.double().cpu().T @ zid.detach()
  assert_close(dzi, zid.grad, 1e-4, 1e-7, "dzimg")
  assert_close(dzt, ztd.grad, 1e-4, 1e-7, "dztxt")


def test_siglip_loss_kernel_extreme_logits(dev):
  """t = 100 (t' is not clipped) and b = -10: logits from about -110 to +90, where exp(-m s) of the naive
  log(1 + exp(.)) overflows fp32; loss, dt', db and G vs fp64."""
  import bv_oracle as O
  from big_vision_amd import ops
  zi, zt = B.siglip_extreme_inputs(dev)
  n, Bn, off = zi.shape[0], zt.shape[0], 14
  tp = torch.tensor([math.log(100.0)], device=dev); bp = torch.tensor([-10.0], device=dev)
  raw = torch.zeros((n, Bn), device=dev)
  ops.sgemm(zi, zi.shape[1], 1, zt, 1, zt.shape[1], raw, n, Bn, zi.shape[1])
  rawd = raw.double().cpu()
  tpd = tp.double().cpu().requires_grad_(True); bpd = bp.double().cpu().requires_grad_(True)
  logits = rawd * torch.exp(tpd) + bpd
  assert logits.max().item() > 88.8 and logits.min().item() < -100
  m = -torch.ones_like(logits); m[torch.arange(n), off + torch.arange(n)] = 1.0
  lg = logits.detach().requires_grad_(True)
  loss_ref = (-O.log_sigmoid(m * lg).sum(-1)).sum() / Bn
  loss_ref.backward()
  (dt_ref,) = torch.autograd.grad(((-O.log_sigmoid(m * logits).sum(-1)).sum() / Bn), tpd, retain_graph=True)
  (db_ref,) = torch.autograd.grad(((-O.log_sigmoid(m * logits).sum(-1)).sum() / Bn), bpd)
  stats = torch.zeros(3, device=dev, dtype=torch.float64)
  ops.siglip_loss_(raw, tp, bp, stats, off, Bn)
  assert torch.isfinite(raw).all() and torch.isfinite(stats).all()
  B.check(stats[0:1].cpu(), loss_ref.detach().reshape(1), None, legacy=(1e-5, 1e-6), name="siglip loss (t = 100)")
  B.check(stats[1:2].cpu(), dt_ref.reshape(1), None, legacy=(1e-4, 1e-6), name="siglip dt' (t = 100)")
  B.check(stats[2:3].cpu(), db_ref.reshape(1), None, legacy=(1e-4, 1e-6), name="siglip db (t = 100)")
  B.check(raw.cpu(), lg.grad, None, legacy=(1e-4, 1e-7), name="siglip G = dL/dlogits (t = 100)")


def test_softmax_xent_extreme_logits(dev):
  """Logits up to +-1e3: the max subtraction keeps every exp finite; loss and dlogits vs fp64."""
  import bv_oracle as O
  from big_vision_amd import ops
  logits, labels = B.softmax_xent_extreme_inputs(dev)
  lr = logits.double().cpu().requires_grad_(True)
  ref = O.softmax_xent(lr, labels.double().cpu())
  ref.backward()
  acc = torch.zeros(1, device=dev, dtype=torch.float64)
  dl = ops.softmax_xent(logits, labels, acc)
  B.check(acc.cpu(), ref.detach().reshape(1), None, legacy=(1e-5, 1e-6), name="xent (|logits| <= 1e3)")
  B.check(dl.cpu(), lr.grad, None, legacy=(1e-4, 1e-7), name="dlogits (|logits| <= 1e3)")


def test_sigmoid_xent_extreme_logits(dev):
  """Logits beyond +-90 (exp overflows fp32 above 88.7) up to +-1e3; loss (with and without the gradient) and dlogits
  vs fp64."""
  import bv_oracle as O
  from big_vision_amd import ops
  logits, labels = B.sigmoid_xent_extreme_inputs(dev)
  lr = logits.double().cpu().requires_grad_(True)
  ref = O.sigmoid_xent(lr, labels.double().cpu())
  ref.backward()
  acc = torch.zeros(1, device=dev, dtype=torch.float64)
  dl = ops.sigmoid_xent(logits, labels, acc)
  B.check(acc.cpu(), ref.detach().reshape(1), None, legacy=(1e-5, 1e-5), name="sigmoid xent (|logits| > 90)")
  B.check(dl.cpu(), lr.grad, None, legacy=(1e-4, 1e-7), name="sigmoid dlogits (|logits| > 90)")
  acc2 = torch.zeros(1, device=dev, dtype=torch.float64)
  assert ops.sigmoid_xent(logits, labels, acc2, want_grad=False) is None
  B.check(acc2.cpu(), ref.detach().reshape(1), None, legacy=(1e-5, 1e-5), name="sigmoid xent fwd-only (|logits| > 90)")


def test_softmax_xent(dev):
  import bv_oracle as O
  from big_vision_amd import ops
  n, C = 8, 1000
  logits = rnd((n, C), dev, 1, 3.0)
  labels = torch.softmax(rnd((n, C), dev, 2, 2.0), -1)  # soft labels (mixup)
  lr = logits.double().cpu().requires_grad_(True)
  ref = O.softmax_xent(lr, labels.double().cpu())
  ref.backward()
  acc = torch.zeros(1, device=dev, dtype=torch.float64)
  dl = ops.softmax_xent(logits, labels, acc)
  assert_close(acc.cpu()[0], ref.detach(), 1e-5, 1e-6, "xent")
  assert_close(dl.cpu(), lr.grad, 1e-4, 1e-7, "dlogits")
  # data-parallel normaliser: a rank holding n of n_global rows contributes n/n_global of the mean
  acc2 = torch.zeros(1, device=dev, dtype=torch.float64)
  dl2 = ops.softmax_xent(logits, labels, acc2, n_global=4 * n)
  assert_close(acc2.cpu()[0], ref.detach() / 4, 1e-5, 1e-6, "xent n_global")
  assert_close(dl2.cpu(), lr.grad / 4, 1e-4, 1e-7, "dlogits n_global")


def test_sigmoid_xent(dev):
  """utils.py:236-243, incl. saturated logits (the stable log-sigmoid form) and forward-only."""
  import bv_oracle as O
  from big_vision_amd import ops
  n, C = 5, 777
  logits = rnd((n, C), dev, 4, 6.0)
  logits[0, :4] = torch.tensor([80.0, -80.0, 1e-3, 30.0], device=dev)  # (not exactly 0: the oracle's min/abs form has a kink there)
  labels = torch.rand((n, C), device=dev)
  lr = logits.double().cpu().requires_grad_(True)
  ref = O.sigmoid_xent(lr, labels.double().cpu())
  ref.backward()
  acc = torch.zeros(1, device=dev, dtype=torch.float64)
  dl = ops.sigmoid_xent(logits, labels, acc)
  assert_close(acc.cpu()[0], ref.detach(), 1e-5, 1e-5, "sigmoid xent")
  assert_close(dl.cpu(), lr.grad, 1e-4, 1e-7, "sigmoid dlogits")
  acc2 = torch.zeros(1, device=dev, dtype=torch.float64)
  assert ops.sigmoid_xent(logits, labels, acc2, want_grad=False) is None
  assert_close(acc2.cpu()[0], ref.detach(), 1e-5, 1e-5, "sigmoid xent fwd-only")


def test_tanh_and_mixup(dev):
  import bv_oracle as O
  from big_vision_amd import ops
  x = rnd((7, 384), dev, 5, 2.0)
  y = ops.tanh_fwd(x)
  assert_close(y, torch.tanh(x.double()), 1e-6, 1e-6, "tanh")
  dy = rnd((7, 384), dev, 6)
  assert_close(ops.tanh_bwd(y, dy), dy.double() * (1 - torch.tanh(x.double()) ** 2), 1e-5, 1e-6, "tanh bwd")
  img = rnd((5, 8, 8, 3), dev, 7)
  ref = O.mixup(0.7, img.double().cpu())[0]
  assert_close(ops.mixup(img, 0.7).cpu(), ref, 1e-6, 1e-6, "mixup (roll by one along the batch)")
  one = rnd((1, 12), dev, 8)
  assert_close(ops.mixup(one, 0.3), one, 1e-6, 1e-6, "mixup n=1")


# ------------------------------------------------------------- optimizer -----
def test_sqnorm_and_adam_vs_oracle(dev):
  import bv_oracle as O
  from big_vision_amd import ops
  import ctypes, struct
  count = 4096
  g = torch.Generator().manual_seed(0)
  p0 = torch.randn(count, generator=g); steps = 3
  grads = [torch.randn(count, generator=g) * 3 for _ in range(steps)]
  # oracle: two tensors, "a/kernel" (wd) = first 3072 elements, "a/bias" = rest
  params = {"a": {"kernel": p0[:3072].clone().double(), "bias": p0[3072:].clone().double()}}
  cfg = dict(lr=1e-2, wd=1e-2, schedule=dict(decay_type="cosine", warmup_steps=2),
             optax_name="scale_by_adam", grad_clip_norm=1.0)
  orc = O.OptaxOracle(cfg, params, sched_kw=dict(total_steps=10, batch_size=8))
  p = p0.clone().to(dev); mu = torch.zeros(count, device=dev); nu = torch.zeros(count, device=dev)
  shadow = torch.empty(count, device=dev, dtype=BF16)
  chunk_seg = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=dev)
  for k in range(steps):
    gk = grads[k]
    upd = orc.update({"a": {"kernel": gk[:3072].double(), "bias": gk[3072:].double()}}, params)
    params = O.tree_map(lambda a, u: a + u, params, upd)
    sched = orc.schedule_fns[0](k)
    segs = torch.tensor([cfg["lr"], cfg["wd"], 0.0, 0.0, cfg["lr"], 0.0, 0.0, 0.0], device=dev)  # sched_idx 0
    gd = gk.to(dev)
    gsq = torch.zeros(1, device=dev, dtype=torch.float64)
    ops.sqnorm_(gd, gsq)
    assert_close(gsq.cpu()[0], (gk.double() ** 2).sum(), 1e-6, 0, "sqnorm")
    stats = torch.zeros(2, device=dev, dtype=torch.float64)
    before = dict(p=p.clone(), g=gd, mu=mu.clone(), nu=nu.clone())
    ops.adam_step_(p, gd, mu, nu, shadow, segs, chunk_seg, count, [sched], gsq, 1.0, 0.9, 0.999, 1e-8,
                   1 - 0.9 ** (k + 1), 1 - 0.999 ** (k + 1), stats)
    ref = torch.cat([params["a"]["kernel"], params["a"]["bias"]])
    assert_close(p.cpu(), ref, 1e-5, 1e-6, f"adam params step {k}")
    # per element, p, mu and nu of THIS step from the state the kernel stored before it (tests/_bounds.py adam_bounds)
    wd_t = torch.cat([torch.full((3072,), cfg["wd"]), torch.zeros(1024)]).to(dev)
    B.check_chain_step("adam", dict(p=p, mu=mu, nu=nu), before, B.f32s(cfg["lr"]), wd_t, B.f32s(sched), gsq.item(), 1.0,
                       dict(b1=0.9, b2=0.999, eps=1e-8, bc1=1 - 0.9 ** (k + 1), bc2=1 - 0.999 ** (k + 1)),
                       f"adam vs oracle inputs, step {k}", legacy=(1e-5, 1e-6), stats=stats)
    assert torch.equal(shadow, p.to(BF16))
    assert_close(stats.cpu()[0], (ref ** 2).sum(), 1e-5, 0, "l2_params^2")
    u = torch.cat([upd["a"]["kernel"], upd["a"]["bias"]])
    assert_close(stats.cpu()[1], (u ** 2).sum(), 1e-4, 1e-12, "l2_updates^2")


@pytest.mark.parametrize("rows,cols", [(768, 2304), (64, 64), (70, 130), (3072, 768)])
def test_transpose_bf16(dev, rows, cols):
  from big_vision_amd import ops
  x = rnd((rows, cols), dev, 3, dtype=BF16)
  y = ops.transpose_bf16(x)
  assert torch.equal(y, x.t().contiguous())
  wide = rnd((rows, cols + 8), dev, 4, dtype=BF16)
  assert torch.equal(ops.transpose_bf16(wide[:, :cols]), wide[:, :cols].t().contiguous())


def test_transpose_bf16_batched(dev):
  """One launch for a table of matrices (ragged shapes, a padded destination pitch, a strided source): every
  destination is bit-equal to the transpose, pad columns and neighbours untouched."""
  from big_vision_amd import ops
  shapes = [(768, 2304), (64, 64), (70, 130), (3072, 768), (588, 1152), (1, 8), (768, 768)]
  pairs, checks = [], []
  for i, (rows, cols) in enumerate(shapes):
    src = rnd((rows, cols + (8 if i % 2 else 0)), dev, 10 + i, dtype=BF16)[:, :cols]
    pitch = (rows + 7) // 8 * 8 + (8 if i % 3 == 0 else 0)
    dst = torch.full((cols, pitch), 7.0, device=dev, dtype=BF16)
    pairs.append((src, dst[:, :rows]))
    checks.append((src, dst, rows))
  table, n, tiles = ops.transpose_table(pairs, dev)
  ops.transpose_bf16_batched(table, n, tiles)
  for src, dst, rows in checks:
    assert torch.equal(dst[:, :rows], src.t())
    assert bool((dst[:, rows:] == 7.0).all())


def test_weight_images_follow_the_optimizer(dev):
  """engine._W.bf_t after an optimizer step (one batched refresh) == the transpose of the new bf16 shadow, for every
  projection kernel of both towers."""
  import bv_oracle as O
  from big_vision_amd import engine
  from big_vision_amd.compat.ml_collections import ConfigDict
  from big_vision_amd.models.proj.image_text import two_towers
  from big_vision_amd.trainers.proj.image_text import siglip
  cfg = dict(width=128, depth=2, mlp_dim=256, num_heads=2)
  model = two_towers.Model(image=dict(cfg, patch_size=(16, 16), pool_type="map"), text=dict(cfg, vocab_size=100),
                           out_dim=(None, 128), temperature_init=10.0, bias_init=-10.0)
  c = ConfigDict()
  c.lr, c.wd, c.optax_name, c.total_steps, c.grad_clip_norm = 1e-2, 1e-2, "scale_by_adam", 10, 1.0
  c.schedule = dict(decay_type="cosine", warmup_steps=0)
  image, text = O.synthetic_batch(1, 8, 64, 16, 100)
  image, text = image.to(dev), text.to(dev)
  state, _ = siglip.make_train_state(model, c, tuple(image.shape), tuple(text.shape), rng=0, total_steps=10)
  fn = siglip.make_update_fn(model, c)
  store = state["params"].store
  seen = []
  for step in range(3):
    state, _ = fn(state, None, {"image": image, "labels": text})
    tw = engine._Twins.of(store)
    ws = [r() for r in tw.members[False]]
    assert len(ws) >= 4 * 4 and all(w is not None for w in ws)
    store.refresh_shadow()
    ws[0].bf_t()              # first stale image of the "next step": refreshes all of them
    for w in ws:
      assert w._t_ver == store.shadow_version
      assert torch.equal(w._t[:, :w.bf.shape[0]], w.bf.t()), w.name
    seen.append(ws[0]._t.float().clone())
  assert not torch.equal(seen[0], seen[1]), "the optimizer did not move the weights: the test checks nothing"


@pytest.mark.parametrize("n,L,D", [(3, 16, 128), (2, 64, 768), (5, 7, 36)])
def test_pool_max_is_exact(dev, n, L, D):
  """bv_pool_max_fwd / _bwd (text pool_type "max" / "gmp", text_transformer.py:89-90) vs torch: the maximum and its
  position bit for bit, the backward = autograd of x.max(dim=1) (no ties in random floats)."""
  from big_vision_amd import ops
  x = rnd((n * L, D), dev, 71)
  y, arg = ops.pool_max_fwd(x, n, L, D)
  ref, idx = x.view(n, L, D).max(dim=1)
  assert torch.equal(y, ref) and torch.equal(arg.long(), idx)
  dy = rnd((n, D), dev, 72)
  dx = ops.pool_max_bwd(dy, arg, n, L, D)
  xr = x.clone().requires_grad_(True)
  xr.view(n, L, D).max(dim=1).values.backward(dy)
  assert torch.equal(dx, xr.grad)
  # NaN propagates like x.max(axis=1) (advisor r5): wherever it sits in the sequence, the pooled value is NaN
  for pos in (0, L // 2, L - 1):
    xn = x.clone()
    xn.view(n, L, D)[0, pos, 1] = float("nan")
    yn, argn = ops.pool_max_fwd(xn, n, L, D)
    assert torch.isnan(yn[0, 1]) and int(argn[0, 1]) == pos
    keep = torch.ones_like(yn, dtype=torch.bool); keep[0, 1] = False
    assert torch.equal(yn[keep], y[keep])
