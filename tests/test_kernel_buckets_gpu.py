"""Dispatch-bucket parity: one row per kernel instantiation of libbvhip.so (or per dispatch row that selects it)
that the workload-shaped tests of test_kernels_gpu.py / test_gemm256_gpu.py do not reach, each compared with a
plain fp64 statement of the op on the same bf16-rounded inputs.

Every row id names the instantiation and the host branch that selects it, so the tables below read against the
dispatchers without running anything:
  attention3.hip, attention5.hip: csrc/attn_route.h attn_route() names the instantiation for every (L, Dh, masked,
                  BV_OPT_ATTN_CFG); tests/test_attn_route_cpu.py holds the ATTN64 / ATTN_CFG tables below to it.
                  attention5.hip launch_bwd5 adds BM: 0 no dbias, 1 DPP, 2 L % 16, 3 identities
  attention_dh.hip BV_ADH_DISPATCH: (Dh + 15) / 16 = 1..8; entered where attn_route_is_adh() says so
  layernorm.hip   bv_layernorm_fwd / _bwd_y: NV = 3 (D <= 768) / 4 (<= 1024) / 8, NT = ln_nt_for (rows * D * 4 > 192 MiB);
                  bv_layernorm_bwd_bf16x: bf16 dy -> ln_bwd_bfx2_kernel<nv4 = 3/4/5/8, FULL = D == NV * 256, RES>,
                  fp32 dy -> ln_bwd_bfx_kernel<true, D <= 1024 ? 2 : 4>; bv_layernorm_fwd_bf16x NV = 3/4/5/8
  gemm_bf16.hip   gemm_bf16_kernel<A_KM, B_KM> where csrc/gemm_route.h gives the call to GEMM_128 (GEMM_256: M, N % 256, K % 64, same layout)
  gemm256.hip     gemm256r_kernel<EPI, F32, 1> under BV_OPT_GEMM_ROLL bit 8

Tolerances are those of the same family in test_kernels_gpu.py: attention o 2e-2, lse 1e-4 / 1e-3, dqkv the backward model of
_bounds.py capped at 3e-2 x max|g|;
LayerNorm fp32 forward 1e-5, backward 1e-4, bf16 outputs 1e-2; GEMM as test_gemm256_gpu.py.  Shapes are small: the
bucket is chosen by L / D / Dh, not by the batch.
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
  bad = err > atol + rtol * b.abs()
  assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err "
                         f"{err.max().item():.3e} (ref max {b.abs().max().item():.3e})")


# ------------------------------------------------------------- attention ----
def _attn_check(dev, n, L, H, Dh, masked, cfg=None, seed=0):
  """o / lse / dqkv / fused bias gradient vs fp64, dqkv with and without dbias bit-equal, zero dK/dV on masked keys,
  run-to-run bit-equality.  cfg: BV_OPT_ATTN_CFG bits OR-ed into the context's value.  Returns (o, lse, dqkv, dbias)."""
  from big_vision_amd import ops
  qkv = rnd((n * L, 3 * H * Dh), dev, 100 + seed, 1.5, dtype=BF16)
  d_o = rnd((n * L, H * Dh), dev, 200 + seed, dtype=BF16)
  # masks: full, a quarter (another bucket's length) and one short of L (cuts the tail fragment)
  lens = [L, max(1, L // 4), max(1, L - 1)][:n] if masked else [L] * n
  kv_len = torch.tensor(lens, device=dev, dtype=torch.int32) if masked else None
  # the kernel family the launch dispatches to under these A/B bits (csrc/attn_route.h)
  c = cfg or 0
  path = B.attn_bwd_path(L, Dh, masked, one_launch=not (c & 128))
  if "dq1" in path and (c & 16):
    path = "attn3 dq+dkv"
  with ops.option("attn_cfg", ops.ctx_get("attn_cfg") | (cfg or 0)):
    o, lse = ops.attn_fwd(qkv, n, L, H, kv_len=kv_len)
    o2, lse2 = ops.attn_fwd(qkv, n, L, H, kv_len=kv_len)
    db = torch.full((3 * H * Dh,), 0.5, device=dev)
    dqkv = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len)
    delta = torch.full((n, H, L), float("nan"), device=dev)
    dqkv_b = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len, dbias=db, delta=delta)
    dqkv2 = ops.attn_bwd(qkv, o, d_o, lse, n, L, H, kv_len=kv_len)
  B.check_attn_fwd(o, lse, qkv, n, L, H, Dh, lens, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3))
  B.check_attn_bwd(dqkv, qkv, d_o, n, L, H, Dh, lens if masked else None, legacy=3e-2, delta=delta, dbias=db,
                   dbias_base=0.5, legacy_db=2e-2, path=path)
  assert torch.equal(o, o2) and torch.equal(lse, lse2), "forward: run-to-run difference"
  assert torch.equal(dqkv, dqkv2), "backward: run-to-run difference"
  assert torch.equal(dqkv, dqkv_b), "backward: dqkv changes when the bias gradient is requested"
  dkv = dqkv.view(n, L, 3, H, Dh)[:, :, 1:]
  for i, ln in enumerate(lens):
    assert (dkv[i, ln:] == 0).all(), f"sample {i}: masked keys must get zero dK / dV"
  return o, lse, dqkv, db


# Dh = 64, both sides of every threshold.  Columns: L, unmasked forward / backward, masked forward / backward.
# fwd = attn3_fwd_kernel<KF, NW, WPS, TAIL>; one-launch = attn5_bwd_kernel<KF, LW, BM>; dq1 = attn3_bwd_dq1_kernel
# <KF, NW, WPS, TAIL>, dq = attn3_bwd_dq_kernel (two sweeps), dkv = attn3_bwd_dkv_kernel, dkv32 = attn4_bwd_dkv_kernel
ATTN64 = [
  (48, "fwd<4,4,4,0>", "attn5<4,1>", "fwd<4,4,4,0>", "dq<4,4,4>+dkv<4,4,4>"),
  (49, "fwd<4,4,4,1>", "attn5<4,1>", "fwd<4,4,4,0>", "dq<4,4,4>+dkv<4,4,4>"),
  (64, "fwd<4,4,4,1>", "attn5<4,1>", "fwd<4,4,4,0>", "dq<4,4,4>+dkv<4,4,4>"),
  (65, "fwd<13,4,3,0>", "dq1<13,8,4,0>+dkv<13,8,4>", "fwd<13,4,3,0>", "dq<13,8,4>+dkv<13,8,4>"),
  (192, "fwd<13,4,3,0>", "dq1<13,8,4,0>+dkv<13,8,4>", "fwd<13,4,3,0>", "dq<13,8,4>+dkv<13,8,4>"),
  (193, "fwd<13,4,3,1>", "attn5<13,3>", "fwd<13,4,3,0>", "dq<13,8,4>+dkv<13,8,4>"),
  (208, "fwd<13,4,3,1>", "attn5<13,3>", "fwd<13,4,3,0>", "dq<13,8,4>+dkv<13,8,4>"),
  (209, "fwd<17,8,4,0>", "dq1<17,8,4,0>+dkv<17,8,4>", "fwd<17,8,4,0>", "dq<17,8,4>+dkv<17,8,4>"),
  (256, "fwd<17,8,4,0>", "dq1<17,8,4,0>+dkv<17,8,4>", "fwd<17,8,4,0>", "dq<17,8,4>+dkv<17,8,4>"),
  (257, "fwd<17,8,4,1>", "dq1<17,8,4,1>+dkv<17,8,4>", "fwd<17,8,4,0>", "dq<17,8,4>+dkv<17,8,4>"),
  (272, "fwd<17,8,4,1>", "dq1<17,8,4,1>+dkv<17,8,4>", "fwd<17,8,4,0>", "dq<17,8,4>+dkv<17,8,4>"),
  (273, "fwd<28,8,2,0>", "dq1<28,8,2,0>+dkv32<28,7>", "fwd<28,8,2,0>", "dq<28,8,2>+dkv<28,8,2>"),
  (432, "fwd<28,8,2,0>", "dq1<28,8,2,0>+dkv32<28,7>", "fwd<28,8,2,0>", "dq<28,8,2>+dkv<28,8,2>"),
  (433, "fwd<28,8,2,1>", "dq1<28,16,4,1>+dkv32<28,7>", "fwd<28,8,2,0>", "dq<28,8,2>+dkv<28,8,2>"),
  (448, "fwd<28,8,2,1>", "dq1<28,16,4,1>+dkv32<28,7>", "fwd<28,8,2,0>", "dq<28,8,2>+dkv<28,8,2>"),
  (449, "fwd<36,8,2,0>", "dq1<36,8,2,0>+dkv32<36,7>", "fwd<36,8,2,0>", "dq<36,8,2>+dkv<36,8,2>"),
  (560, "fwd<36,8,2,0>", "dq1<36,8,2,0>+dkv32<36,7>", "fwd<36,8,2,0>", "dq<36,8,2>+dkv<36,8,2>"),
  (561, "fwd<36,8,2,1>", "dq1<36,8,2,1>+dkv32<36,7>", "fwd<36,8,2,0>", "dq<36,8,2>+dkv<36,8,2>"),
  (576, "fwd<36,8,2,1>", "dq1<36,8,2,1>+dkv32<36,7>", "fwd<36,8,2,0>", "dq<36,8,2>+dkv<36,8,2>"),
]
ATTN64_ROWS = ([pytest.param(L, False, id=f"L{L}-unmasked-{f}-{b}") for L, f, b, _, _ in ATTN64] +
               [pytest.param(L, True, id=f"L{L}-masked-{f}-{b}") for L, _, _, f, b in ATTN64])


@pytest.mark.parametrize("L,masked", ATTN64_ROWS)
def test_attention_dh64_bucket(dev, L, masked):
  _attn_check(dev, 3 if masked else 2, L, 2, 64, masked)


# BV_OPT_ATTN_CFG A/B bits, one shape per bucket each bit changes.  Columns: L, masked, bit, what it selects.
ATTN_CFG = [
  (100, False, 8, "fwd<13,8,4,0>"), (200, False, 8, "fwd<13,8,4,1>"), (150, True, 8, "fwd<13,8,4,0>-masked"),
  (100, False, 16, "dq<13,8,4>-unmasked"), (240, False, 16, "dq<17,8,4>-unmasked"),
  (300, False, 16, "dq<28,8,2>-unmasked"), (500, False, 16, "dq<36,8,2>-unmasked"),
  (100, False, 32, "dkv32<13,4>"), (240, False, 32, "dkv32<17,4>"), (300, False, 32, "dkv32<28,4>"),
  (500, False, 32, "dkv32<36,4>"), (240, True, 32, "dkv32<17,4>-masked"), (441, True, 32, "dkv32<28,4>-masked"),
  (100, False, 64, "dkv32<13,7>"), (240, False, 64, "dkv32<17,7>"), (150, True, 64, "dkv32<13,7>-masked"),
  (500, True, 64, "dkv32<36,7>-masked"),
  (48, False, 128, "no-attn5:dq1<4,4,4,0>+dkv<4,4,4>"), (64, False, 128, "no-attn5:dq1<4,4,4,1>+dkv<4,4,4>"),
  (200, False, 128, "no-attn5:dq1<13,8,4,1>+dkv<13,8,4>"),
  (64, False, 256, "attn5<4,1,BM=1>"), (200, False, 256, "attn5<13,3,BM=1>"),
  (441, False, 1024, "dkv<28,8,2>-classic"), (576, False, 1024, "dkv<36,8,2>-classic"),
]


@pytest.mark.parametrize("L,masked,bit", [pytest.param(L, m, b, id=f"bit{b}-L{L}-{what}") for L, m, b, what in ATTN_CFG])
def test_attention_cfg_bit(dev, L, masked, bit):
  """Each A/B variant vs fp64.  Where the sources state bit-identical results, also bit-compared with the default
  launch: the DPP bias reduction (bit 256) leaves dqkv unchanged (test_kernels_gpu.py one-launch test), and the
  classic dK/dV kernel of the long sequences (bit 1024) equals the 32-key-block default (csrc/attn_route.h)."""
  n = 3 if masked else 2
  o, lse, dqkv, _ = _attn_check(dev, n, L, 2, 64, masked, cfg=bit, seed=1)
  if bit in (256, 1024):
    o0, lse0, dqkv0, _ = _attn_check(dev, n, L, 2, 64, masked, seed=1)
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    assert torch.equal(dqkv, dqkv0), f"attn_cfg bit {bit} changed dqkv"


# attention_dh.hip: BV_ADH_DISPATCH case (Dh + 15) / 16; adh_{fwd,bwd_dq,bwd_dkv}_kernel<NS>
ADH = [(24, 2, 100), (40, 3, 130), (48, 3, 70), (56, 4, 100), (88, 6, 90), (96, 6, 100), (112, 7, 60),
       (120, 8, 50), (64, 4, 600)]


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("Dh,ns,L", [pytest.param(d, c, L, id=f"Dh{d}-adh<{c}>-L{L}") for d, c, L in ADH])
def test_attention_dh_bucket(dev, Dh, ns, L, masked):
  assert (Dh + 15) // 16 == ns
  _attn_check(dev, 3 if masked else 2, L, 2, Dh, masked, seed=2)


@pytest.mark.parametrize("Dh,L", [(8, 40), (48, 100), (88, 196), (96, 77), (120, 33)])
def test_map_attention_dh_bucket(dev, Dh, L):
  """adh_map_fwd_kernel / adh_map_bwd_kernel (bv_map_attn_*_dh: every Dh != 64) vs fp64, with and without a mask."""
  from big_vision_amd import ops
  n, H = 3, 2
  q = rnd((n, H * Dh), dev, 1, dtype=BF16)
  kv = rnd((n * L, 2 * H * Dh), dev, 2, dtype=BF16)
  d_o = rnd((n, H * Dh), dev, 3, dtype=BF16)
  for lens in ([L] * n, [L, max(1, L // 2), 1]):
    kv_len = torch.tensor(lens, device=dev, dtype=torch.int32)
    o, pp = ops.map_attn_fwd(q, kv, n, L, H, kv_len=kv_len)
    B.check_map_attn_fwd(o, pp, q, kv, n, L, H, Dh, lens, legacy_p=(1e-3, 1e-5), legacy_o=(1e-2, 1e-2))
    dq, dkv = ops.map_attn_bwd(q, kv, pp, d_o, n, L, H)
    B.check_map_attn_bwd(dq, dkv, q, kv, d_o, n, L, H, Dh, lens, legacy=2e-2)
    dq2, dkv2 = ops.map_attn_bwd(q, kv, pp, d_o, n, L, H)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)


# ------------------------------------------------------------- LayerNorm ----
def _ln_ref(x, scale, bias, D):
  xr = x.double().requires_grad_(True); sr = scale.double().requires_grad_(True); br = bias.double().requires_grad_(True)
  return xr, sr, br, torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6)


def _nt3_rows(D):
  """Smallest ragged row count whose fp32 rows * D * 4 bytes exceed 192 MiB (layernorm.hip ln_nt_for -> NT = 3)."""
  return (192 << 20) // (4 * D) + 3


def _nv(D):
  return 3 if D <= 768 else (4 if D <= 1024 else 8)


LN_F32 = [(4, 1), (4, 37), (772, 1), (772, 37), (1024, 1), (1028, 37), (1152, 1), (1152, 37), (1408, 37),
          (2048, 1), (2048, 37), (1024, _nt3_rows(1024)), (1152, _nt3_rows(1152))]


@pytest.mark.parametrize("D,rows", [pytest.param(D, r, id=f"D{D}-rows{r}-ln_fwd<{_nv(D)},{3 if r > 1000 else 2}>")
                                    for D, r in LN_F32])
def test_layernorm_f32_bucket(dev, D, rows):
  """fp32 residual stream: ln_fwd_kernel<NV, NT>, ln_bwd_kernel<DY_F32, NV, NT> for both dy dtypes, with and
  without dres, the bv_layernorm_bwd_y re-emit; vs fp64."""
  from big_vision_amd import ops
  x = rnd((rows, D), dev, 1, 2.0) + 0.5
  scale = 1 + 0.1 * rnd((D,), dev, 2); bias = 0.1 * rnd((D,), dev, 3)
  xr, sr, br, ref = _ln_ref(x, scale, bias, D)
  y_bf, y_f, mean, rstd = ops.layernorm_fwd(x, scale, bias, rows=rows, D=D, want_f32=True)
  B.check_ln_fwd(y_f, x, scale, bias, legacy=(1e-5, 1e-5), name="ln fwd f32")
  B.check_ln_fwd(y_bf, x, scale, bias, legacy=(1e-2, 1e-2), name="ln fwd bf16")
  y_bf2, y_f2, mean2, rstd2 = ops.layernorm_fwd(x, scale, bias, rows=rows, D=D, want_f32=True)
  assert torch.equal(y_f, y_f2) and torch.equal(y_bf, y_bf2) and torch.equal(rstd, rstd2)
  dy32 = rnd((rows, D), dev, 4)
  for dy in (dy32, dy32.to(BF16)):
    xr.grad = sr.grad = br.grad = None
    torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6).backward(dy.double(), retain_graph=True)
    for with_res in (False, True):
      dres = rnd((rows, D), dev, 5) if with_res else None
      want = xr.grad + (dres.double() if with_res else 0)
      dscale = torch.zeros(D, device=dev); dbias = torch.zeros(D, device=dev); dxsum = torch.ones(D, device=dev)
      dx_bf = torch.empty((rows, D), device=dev, dtype=BF16)
      dx = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres, dx_bf16=dx_bf, dscale=dscale,
                             dbias=dbias, dx_colsum=dxsum)
      tag = f"(dy {dy.dtype}, dres {with_res})"
      B.check_ln_bwd(dx, x, scale, dy, dres=dres, legacy=(1e-4, 1e-4), name=f"ln dx {tag}")
      B.check_ln_bwd(dx_bf, x, scale, dy, dres=dres, legacy=(1e-2, 1e-2), name=f"ln dx bf16 {tag}")
      assert_close(dxsum, 1.0 + dx.double().sum(0), 1e-4, 1e-3, f"ln dx colsum {tag}")
      assert_close(dscale, sr.grad, 1e-4, 1e-3, f"ln dscale {tag}")
      assert_close(dbias, br.grad, 1e-4, 1e-3, f"ln dbias {tag}")
      # bv_layernorm_bwd_y: y re-emitted bit-equal to the forward's, dx bit-equal to the plain backward
      y_re = torch.zeros((rows, D), device=dev, dtype=BF16)
      dx_bf2 = torch.empty((rows, D), device=dev, dtype=BF16)
      dx_y = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres, dx_bf16=dx_bf2, bias=bias, y_out=y_re)
      assert torch.equal(y_re, y_bf), f"re-emitted LayerNorm output differs {tag}"
      assert torch.equal(dx_y, dx) and torch.equal(dx_bf2, dx_bf), f"bwd_y differs from the plain backward {tag}"
  if rows > 1:   # strided rows: every third row from the second (an encoder_norm on one token per sample)
    n, L = rows // 3, 3
    _, y, m_s, r_s = ops.layernorm_fwd(x, scale, bias, rows=n, D=D, row_stride=L, row_offset=1, want_bf16=False,
                                       want_f32=True)
    sel = x[:n * L].view(n, L, D)[:, 1].double()
    B.check_ln_fwd(y, sel, scale, bias, legacy=(1e-5, 1e-5), name="strided ln fwd")
    dys = rnd((n, D), dev, 6)
    xs = x[:n * L].contiguous()
    dxs = ops.layernorm_bwd(dys, xs, scale, m_s, r_s, rows=n, D=D, row_stride=L, row_offset=1)
    xq = xs.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xq.view(n, L, D)[:, 1], (D,), scale.double(), bias.double(),
                                   eps=1e-6).backward(dys.double())
    assert_close(dxs, xq.grad, 1e-4, 1e-4, "strided ln bwd: other rows stay 0")
    B.check_ln_bwd(dxs.view(n, L, D)[:, 1], sel, scale, dys, legacy=(1e-4, 1e-4), name="strided ln bwd")
  # rows of std 1e-2 / 1e-3 (pin eps) and |mean| / std = 4 in launches of their own without the fused column sums
  # (rows 1, 4, 7, 10 feed the strided launch; rows = 1 runs each kind as row 0)
  for dres in (None, rnd((rows, D), dev, 5)):
    B.check_ln_edge_launch(ops, x, scale, bias, (dy32, dy32.to(BF16)), dres=dres,
                           strided=(rows // 3, 3, 1) if rows > 1 and dres is None else None)


def _bfx2(D):
  nv = min(8, max(3, (D + 255) // 256))
  nv = 8 if nv > 5 else nv
  return nv, int(D == nv * 256)


LN_BF16 = [512, 768, 776, 1024, 1152, 1280, 1408, 1536, 2048]


@pytest.mark.parametrize("D", [pytest.param(D, id=f"D{D}-bfx2<{_bfx2(D)[0]},{_bfx2(D)[1]},*>-bfx<1,{2 if D <= 1024 else 4}>")
                               for D in LN_BF16])
@pytest.mark.parametrize("rows", [1, 37])
def test_layernorm_bf16_stream_bucket(dev, D, rows):
  """bf16 residual stream: ln_fwd_bfx_kernel<NV>, ln_bwd_bfx2_kernel<NV, FULL, RES> (bf16 dy, with and without
  dres) and ln_bwd_bfx_kernel<true, NV> (fp32 dy); vs fp64 LayerNorm of the same bf16 inputs."""
  from big_vision_amd import ops
  x = (rnd((rows, D), dev, 1, 2.0) + 0.5).to(BF16)
  scale = 1 + 0.1 * rnd((D,), dev, 2); bias = 0.1 * rnd((D,), dev, 3)
  xr, sr, br, ref = _ln_ref(x, scale, bias, D)
  y_bf, y_f, mean, rstd = ops.layernorm_fwd(x, scale, bias, rows=rows, D=D, want_f32=True)
  B.check_ln_fwd(y_f, x, scale, bias, legacy=(1e-5, 1e-5), name="ln fwd f32 (bf16 x)")
  B.check_ln_fwd(y_bf, x, scale, bias, legacy=(1e-2, 1e-2), name="ln fwd bf16 (bf16 x)")
  dy32 = rnd((rows, D), dev, 4)
  for dy in (dy32.to(BF16), dy32):
    xr.grad = sr.grad = br.grad = None
    torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6).backward(dy.double(), retain_graph=True)
    for with_res in (False, True):
      dres = rnd((rows, D), dev, 5).to(BF16) if with_res else None
      want = xr.grad + (dres.double() if with_res else 0)
      dscale = torch.zeros(D, device=dev); dbias = torch.zeros(D, device=dev); dxsum = torch.ones(D, device=dev)
      dx = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres, dscale=dscale, dbias=dbias,
                             dx_colsum=dxsum)
      tag = f"(dy {dy.dtype}, dres {with_res})"
      assert dx.dtype == BF16
      B.check_ln_bwd(dx, x, scale, dy, dres=dres, legacy=(1e-2, 1e-2), name=f"ln dx (bf16 stream) {tag}")
      assert_close(dxsum, 1.0 + want.sum(0), 1e-4, 1e-3, f"ln dx colsum {tag}")
      assert_close(dscale, sr.grad, 1e-4, 1e-3, f"ln dscale {tag}")
      assert_close(dbias, br.grad, 1e-4, 1e-3, f"ln dbias {tag}")
      dx2 = ops.layernorm_bwd(dy, x, scale, mean, rstd, rows=rows, D=D, dres=dres)
      assert torch.equal(dx, dx2), f"run-to-run / colsum-variant difference {tag}"
  # the edge rows in launches of their own without the fused column sums (rows = 1: each kind as row 0)
  for dres in (None, rnd((rows, D), dev, 5).to(BF16)):
    B.check_ln_edge_launch(ops, x, scale, bias, (dy32.to(BF16), dy32), dres=dres)


# ------------------------------------------------------------------ GEMM ----
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (136, 144, 72), (520, 264, 200), (8, 8, 8)])
def test_gemm_general_fourth_layout(dev, M, N, K):
  """gemm_bf16_kernel<false, true>: A k-minor ([K][M]), B k-major ([N][K]); never taken by the 256 x 256 path
  (a_kmajor != b_kmajor), with and without bias, bf16 and fp32 out."""
  from big_vision_amd import ops
  a = rnd((K, M), dev, 7, dtype=BF16)
  b = rnd((N, K), dev, 8, 0.05, dtype=BF16)
  bias = rnd((N,), dev, 9)
  prod = a.double().T @ b.double().T
  kw = dict(a_kmajor=False, b_kmajor=True)
  for bb in (None, bias):
    ref = prod + (bb.double() if bb is not None else 0)
    y = ops.gemm(a, b, bias=bb, out_dtype=F32, **kw)
    B.check_gemm(y, ref, a.T, b.T, legacy=(1e-4, 1e-3), name="gemm<0,1> f32")
    assert torch.equal(y, ops.gemm(a, b, bias=bb, out_dtype=F32, **kw))
    y16 = ops.gemm(a, b, bias=bb, out_dtype=BF16, **kw)
    B.check_gemm(y16, ref, a.T, b.T, legacy=(1e-2, 1e-2), name="gemm<0,1> bf16")


@pytest.mark.parametrize("epi", ["none", "gelu"])
def test_rolling_epilogue_bit8(dev, epi):
  """gemm256r_kernel<EPI, false, 1> (BV_OPT_GEMM_ROLL bit 8) vs the full-epilogue gemm256_kernel (roll 0): bit-identical
  for the bf16 epilogues as test_gemm256_gpu.py's rolling-epilogue test states for the other variant; vs fp32 too."""
  from big_vision_amd import ops
  M, N, K = 2048, 768, 256
  a = rnd((M, K), dev, 21, dtype=BF16)
  w = rnd((N, K), dev, 22, 0.05, dtype=BF16)
  b = rnd((N,), dev, 23)
  kw = dict(a_kmajor=True, b_kmajor=True)
  pre = a.double() @ w.double().T + b.double()

  def run():
    if epi == "none":
      return (ops.gemm(a, w, bias=b, out_dtype=BF16, **kw), ops.gemm(a, w, out_dtype=BF16, alpha=0.5, **kw))
    g = torch.empty((M, N), device=dev, dtype=BF16)
    h = ops.gemm(a, w, bias=b, out_dtype=BF16, epilogue=ops.EPI_GELU, out2=g, **kw)
    return h, g

  with ops.option("fast_path", 1):
    with ops.option("gemm_roll", 0):
      ref = run()
    with ops.option("gemm_roll", (2 if epi == "none" else 4) | 8):
      new = [run() for _ in range(3)]
  for r in new:
    for x, y in zip(r, ref):
      assert torch.equal(x, y), f"gemm_roll bit 8 ({epi}) differs from the full-epilogue kernel"
  if epi == "none":
    B.check_gemm(new[0][0], pre, a, w.T, legacy=(1e-2, 1e-2), name="roll8 bias bf16")
    B.check_gemm(new[0][1], 0.5 * (pre - b.double()), a, w.T, legacy=(1e-2, 1e-2), name="roll8 alpha bf16", n_adds=0,
                 alpha=0.5)
  else:
    B.check_gemm(new[0][0], pre, a, w.T, legacy=(1e-2, 1e-2), name="roll8 gelu pre")
    assert_close(new[0][1], B.gelu_tanh64(pre), 1e-2, 1e-2, "roll8 gelu out")
    B.check_gelu_g(new[0][1], new[0][0], legacy=(1e-2, 1e-2), name="roll8 gelu out (of the stored h)")


# M or N = 256 k +- 8 and K = 64 k +- 8: only (512, 768, 128) and its dW transpose qualify for the 256 x 256 path
EDGES = [(512, 768, 128, True), (504, 768, 128, False), (520, 768, 128, False), (512, 760, 128, False),
         (512, 776, 128, False), (512, 768, 120, False), (512, 768, 136, False)]


@pytest.mark.parametrize("M,N,K,fast", [pytest.param(*e, id=f"M{e[0]}-N{e[1]}-K{e[2]}-{'gemm256' if e[3] else 'general'}")
                                        for e in EDGES])
def test_gemm_fast_path_edges(dev, M, N, K, fast):
  """csrc/gemm_route.h gives the 256 x 256 kernels exactly M, N % 256 == 0 and K % 64 == 0 (their launch counter moves); both sides vs fp32 on
  the same bf16 inputs, the accepted one also vs the general kernel, for the k-major forward / dX layout and the
  k-minor dW layout (fp32 atomic accumulation)."""
  from big_vision_amd import ops
  a = rnd((M, K), dev, 31, dtype=BF16)
  w = rnd((N, K), dev, 32, 0.05, dtype=BF16)
  bias = rnd((N,), dev, 33)
  ref = a.double() @ w.double().T + bias.double()
  with ops.option("fast_path", 1):
    c0 = ops.ctx_get("gemm256_calls")
    outs = [ops.gemm(a, w, a_kmajor=True, b_kmajor=True, bias=bias, out_dtype=F32) for _ in range(3)]
    assert (ops.ctx_get("gemm256_calls") > c0) == fast, "fast-path selection"
    o16 = ops.gemm(a, w, a_kmajor=True, b_kmajor=True, bias=bias, out_dtype=BF16)
    # dW = A^T B with both operands k-minor ([K][M] x [K][N]) into an fp32 accumulator
    x = rnd((K, M), dev, 34, dtype=BF16); dy = rnd((K, N), dev, 35, dtype=BF16)
    base = rnd((M, N), dev, 36)
    dw = base.clone()
    c1 = ops.ctx_get("gemm256_calls")
    ops.gemm(x, dy, a_kmajor=False, b_kmajor=False, out=dw, epilogue=ops.EPI_ATOMIC)
    assert (ops.ctx_get("gemm256_calls") > c1) == fast, "fast-path selection (dW layout)"
  close_ref = dict(rtol=1e-4, atol=2e-3)
  B.check_gemm(outs[0], ref, a, w.T, legacy=(close_ref["rtol"], close_ref["atol"]), name="f32")
  for o in outs[1:]:
    assert torch.equal(o, outs[0]), "run-to-run difference"
  B.check_gemm(o16, ref, a, w.T, legacy=(1e-2, 1e-2), name="bf16")
  B.check_gemm(dw, base.double() + x.double().T @ dy.double(), x.T, dy, legacy=(1e-4, 1e-4 * K ** 0.5 * 4), name="dW",
               n_adds=2 + 8)
  if fast:
    with ops.option("fast_path", 0):
      gen = ops.gemm(a, w, a_kmajor=True, b_kmajor=True, bias=bias, out_dtype=F32)
    assert_close(outs[0], gen, 1e-5, 1e-3, "256 x 256 vs general kernel")


# ------------------------------------------------- elementwise / loss rows ----
@pytest.mark.parametrize("n,L,D", [(3, 7, 36), (5, 196, 768), (1, 1, 4)])
def test_pool_gap_masked(dev, n, L, D):
  """pool_gap_masked_fwd_kernel / _bwd_kernel (bv_pool_gap_masked_*: NaFlex "gap" over the first lens[b] tokens) vs
  fp64, lengths 1, L and in between; rows past a length get a zero gradient."""
  from big_vision_amd import ops
  x = rnd((n * L, D), dev, 41)
  lens = [L, 1, max(1, L // 2), max(1, L - 1), min(2, L)][:n]
  lt = torch.tensor(lens, device=dev, dtype=torch.int32)
  xr = x.double().view(n, L, D).requires_grad_(True)
  mask = (torch.arange(L, device=dev)[None, :] < lt[:, None].long()).double()
  ref = (xr * mask[:, :, None]).sum(1) / lt.double()[:, None]
  y = ops.pool_gap_fwd(x, n, L, D, lens=lt)
  assert_close(y, ref, 1e-5, 1e-6, "masked gap")
  dy = rnd((n, D), dev, 42)
  ref.backward(dy.double())
  dx = ops.pool_gap_bwd(dy, n, L, D, lens=lt)
  assert_close(dx, xr.grad.view(n * L, D), 1e-6, 1e-7, "masked gap bwd")
  for i, ln in enumerate(lens):
    assert (dx.view(n, L, D)[i, ln:] == 0).all()
  assert torch.equal(y, ops.pool_gap_fwd(x, n, L, D, lens=lt))


@pytest.mark.parametrize("P,grids", [(16, [(8, 12), (16, 16), (3, 1)]), (64, [(20, 31), (64, 64)]), (7, [(13, 2)])])
def test_naflex_posemb_weights(dev, P, grids):
  """naflex_posw_kernel (bv_naflex_posemb_weights, P <= 64): per example the [P*P] resize-and-gather weights of every
  token, vs the oracle's fp64 restatement of jax.image.scale_and_translate weights (bv_oracle.scale_and_translate_weights,
  the separable factors of bv_oracle.naflex_pos_emb_resize); grids smaller and larger than P (down- and up-sampling),
  and padding tokens at (0, 0)."""
  import bv_oracle as O
  from big_vision_amd import ops
  n, N = len(grids), max(h * w for h, w in grids) + 3
  yabs = torch.zeros((n, N), dtype=torch.int32); xabs = torch.zeros((n, N), dtype=torch.int32)
  for e, (h, w) in enumerate(grids):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    yabs[e, :h * w] = yy.flatten(); xabs[e, :h * w] = xx.flatten()
  W = ops.naflex_posemb_weights(yabs.to(dev), xabs.to(dev), P)
  assert W.shape == (n * N, P * P) and W.dtype == BF16
  # token t of example e reads pos_emb[i, j] with weight wy[i, yabs[t]] * wx[j, xabs[t]] (64 x 64 canvas, grid h x w)
  ref = []
  for e, (h, w) in enumerate(grids):
    wy = O.scale_and_translate_weights(P, 64, h / P)[:, yabs[e].long()]
    wx = O.scale_and_translate_weights(P, 64, w / P)[:, xabs[e].long()]
    ref.append((wy[:, None, :] * wx[None, :, :]).reshape(P * P, N).T)
  ref = torch.cat(ref).to(dev)
  assert_close(W, ref, 1e-2, 1e-3, "naflex position-embedding weights")
  assert torch.equal(W, ops.naflex_posemb_weights(yabs.to(dev), xabs.to(dev), P))


@pytest.mark.parametrize("n,B,off", [(8, 8, 0), (7, 21, 14), (33, 1000, 500)])
def test_logit_stats(dev, n, B, off):
  """logit_stats_kernel + logit_stats_finish (bv_logit_stats: the contrastive trainer's per-device measurements) vs
  fp64: min / max / mean of the positives (the diagonal at row_offset), the local negatives (other columns of the
  local block) and all negatives, logits = exp(t') raw + b."""
  from big_vision_amd import ops
  raw = rnd((n, B), dev, 51)
  tp = torch.tensor([math.log(7.0)], device=dev); bp = torch.tensor([-1.5], device=dev)
  out = ops.logit_stats(raw, tp, bp, off)
  lg = 7.0 * raw.double() - 1.5
  rows = torch.arange(n, device=dev)
  pos = torch.zeros((n, B), dtype=torch.bool, device=dev); pos[rows, off + rows] = True
  loc = torch.zeros_like(pos); loc[:, off:off + n] = True
  sel = [lg[pos], lg[loc & ~pos], lg[~pos]]
  ref = torch.stack([f(s) if s.numel() else torch.zeros((), dtype=torch.float64, device=dev)
                     for s in sel for f in (torch.min, torch.max, torch.mean)])
  assert_close(out, ref, 1e-5, 1e-5, "logit stats " + str(ops.LOGIT_STATS_NAMES))
  assert torch.equal(out, ops.logit_stats(raw, tp, bp, off))


@pytest.mark.parametrize("count", [1, 1023, 4096 * 257 + 5])
def test_dot(dev, count):
  """dot_kernel (bv_dot_f32: out += sum a b in an fp64 accumulator, the softmax contrastive loss's dL/dt') vs fp64."""
  from big_vision_amd import ops
  a = rnd((count,), dev, 61); b = rnd((count,), dev, 62)
  out = torch.full((1,), 0.25, device=dev, dtype=torch.float64)
  ops.dot_(a, b, out)
  ref = 0.25 + (a.double() * b.double()).sum()
  assert_close(out, ref.reshape(1), 1e-6, 1e-6 * count ** 0.5, "dot")


@pytest.mark.parametrize("C", [10, 255, 256, 257])
def test_softmax_xent_small_classes_and_saturated_logits(dev, C):
  """softmax_xent_kernel with fewer classes than a workgroup's 256 lanes and around it, one-hot and soft labels, and a
  saturated row (one logit 100 above the rest) vs the oracle's fp64 statement (utils.py:276-281)."""
  import bv_oracle as O
  from big_vision_amd import ops
  n = 6
  logits = rnd((n, C), dev, 71, 3.0)
  logits[0, C // 2] = 100.0
  logits[1] = -50.0; logits[1, 0] = 50.0
  labels = torch.softmax(rnd((n, C), dev, 72, 2.0), -1)
  labels[0] = 0; labels[0, C // 2] = 1.0
  labels[2] = 0; labels[2, C - 1] = 1.0
  lr = logits.double().cpu().requires_grad_(True)
  ref = O.softmax_xent(lr, labels.double().cpu())
  ref.backward()
  acc = torch.zeros(1, device=dev, dtype=torch.float64)
  dl = ops.softmax_xent(logits, labels, acc)
  assert torch.isfinite(dl).all()
  assert_close(acc.cpu()[0], ref.detach(), 1e-5, 1e-6, "xent")
  assert_close(dl.cpu(), lr.grad, 1e-4, 1e-7, "dlogits")
