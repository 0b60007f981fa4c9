"""Memory footprint of every compute entry point of libbvhip (include/bvhip.h): one table, one row per case.  Each row
carves the operands of ONE call out of a guarded 0xFF arena (tests/_footprint.py), passes raw pointers through
`_lib.call` on the current stream and holds the call to the four-point contract of DESIGN.md "Memory footprint": no
byte changes outside the declared write extents (inputs, pitch gaps, unselected rows, guard bands and the bytes behind
the declared workspace stay bit-identical), no output depends on a byte outside an input extent, every output element
is written, and the values meet the bound the entry point's parity test already uses (tests/_bounds.py models, else
the rtol / atol of test_kernels_gpu.py / test_kernel_buckets_gpu.py / test_adafactor_gpu.py / test_dropout_gpu.py).

Inputs that a backward takes from its forward (lse, o, mean, rstd, p, argmax, norm) are computed on the CPU in fp64
and rounded once: every row is a single guarded call.  Shapes are the smallest at which the mechanism can go wrong.
Deviations from the case list that the entry points themselves force (each is rejected with BV_ERR_INVALID_ARG otherwise):
  * bv_gemm_bf16 with A stored [K][M] needs M % 8 == 0: those two layouts run (136, 136, 72) and (8, 8, 8) / (8, 8, 5);
  * bv_adam_step / bv_trace_step take count % 1024 == 0 and one segment per 1024-element chunk: the three segments
    cover 2 + 1 + 2 chunks;
  * bv_colsum takes cols % 8 == 0: 37 x 136 instead of 37 x 130;
  * masked attention rows use n = 3 so that kv_len holds 1, L and a middle value at once.

test_footprint_cpu.py::test_every_compute_entry_point_has_a_footprint_row holds this table to `_lib.PROTOTYPES` (it
needs no GPU).  Measured on an MI355X: 295 rows, no finding, 9.5 s for the file (the -m gpu suite without it: 564 s).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _bounds as B
import _footprint as F
from _footprint import Op, mat

pytestmark = pytest.mark.gpu

BF16, F32, F64, I32, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.uint8

ROWS = []   # (entry points covered, case id, fn(dev))
ARGS = {}   # case id -> (row function, args, kw) of the rows made by add(): test_gemm_route_cpu.py reads the GEMM rows


def row(entries, case):
  def deco(fn):
    ROWS.append((tuple(entries.split()), case, fn))
    return fn
  return deco


def add(entries, case, fn, *args, **kw):
  ROWS.append((tuple(entries.split()), case, lambda dev: fn(dev, *args, **kw)))
  ARGS[case] = (fn, args, kw)


def stream():
  return torch.cuda.current_stream().cuda_stream


def call(name, *args):
  from big_vision_amd import _lib
  return _lib.call(name, *args)


def gen(seed):
  return torch.Generator(device="cpu").manual_seed(seed)


def randn(shape, seed, scale=1.0, dtype=F32):
  return (torch.randn(shape, generator=gen(seed), dtype=F32) * scale).to(dtype)


def assert_close(a, b, rtol, atol, name=""):
  a = a.double(); b = b.double()
  err = (a - b).abs()
  bad = ~(err <= atol + rtol * b.abs())
  assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err "
                         f"{err.nan_to_num(float('inf')).max().item():.3e} (ref max {b.abs().max().item():.3e})")


# ---------------------------------------------------------------- GEMM ------
E = dict(NONE=0, RESIDUAL=1, POS=2, GELU=3, GELU_BWD=4, ATOMIC=5, GELU_BWD_EMIT=6, GELU_GD=7, MUL=8, GELU_G=9)
PAD = 8


def _gemm_call(dev, tag, M, N, K, akm, bkm, out_f32, epi, *, bias=True, aux_rows=0, colsum=False, split_k=0, opts=None,
               ws="none", stat=(0, 0, 0)):
  """One guarded bv_gemm_bf16[_colsum] launch; every pitch is its minimum + 8 elements.  ws: "none" (no workspace:
  atomics) or "exact" (bv_gemm_workspace_bytes, declared to the byte).  stat: expected increments of the context's
  BV_STAT_GEMM256_CALLS / MULTI / FUSED.  Returns the harness result."""
  from big_vision_amd import ops
  e = E[epi]
  cdt = F32 if out_f32 else BF16
  ctx = ops.Context()
  for k, v in (opts or {}).items():
    ctx.set(k, v)
  wsb = call("bv_gemm_workspace_bytes", M, N, K) if ws == "exact" else 0
  assert ws != "exact" or wsb > 0
  auxdt = {"RESIDUAL": cdt, "POS": F32, "GELU_BWD": BF16, "GELU_BWD_EMIT": BF16, "MUL": BF16}.get(epi)
  c2role = {"GELU": "out", "GELU_BWD_EMIT": "out", "GELU_GD": "out", "GELU_G": "in"}.get(epi)

  def make():
    a = (M, K) if akm else (K, M)
    b = (N, K) if bkm else (K, N)
    o = [mat("A", BF16, *a, a[1] + PAD), mat("B", BF16, *b, b[1] + PAD, fill=0.05),
         mat("C", cdt, M, N, N + PAD, role="inout" if epi == "ATOMIC" else "out", fill=randn((M, N), 7))]
    if bias:
      o.append(Op("bias", F32, (N,)))
    if auxdt is not None:
      o.append(mat("aux", auxdt, aux_rows or M, N, N + PAD))
    if c2role:
      o.append(mat("C2", BF16, M, N, N + PAD, role=c2role))
    if colsum:
      o.append(Op("colsum", F32, (N,), "inout"))
    if wsb:
      o.append(Op("ws", U8, (wsb,), "scratch"))
    return o

  def launch(ar):
    call("bv_ctx_set_workspace", ctx.ptr, ar.ptr("ws") if wsb else None, wsb)
    args = [int(akm), int(bkm), ar.ptr("A"), (K if akm else M) + PAD, ar.ptr("B"), (K if bkm else N) + PAD, ar.ptr("C"),
            N + PAD, int(out_f32), M, N, K, e, ar.ptr("bias") if bias else None, ar.ptr("aux") if auxdt is not None else None,
            N + PAD if auxdt is not None else 0, aux_rows, ar.ptr("C2") if c2role else None, 1.0, split_k]
    if colsum:
      call("bv_gemm_bf16_colsum", *args, ar.ptr("colsum"), stream(), ctx.ptr)
    else:
      call("bv_gemm_bf16", *args, stream(), ctx.ptr)

  before = [ctx.get(s) for s in ("gemm256_calls", "gemm256_multi", "gemm256_fused")]
  r = F.run("bv_gemm_bf16_colsum" if colsum else "bv_gemm_bf16", tag, make, launch, dev)
  after = [ctx.get(s) for s in ("gemm256_calls", "gemm256_multi", "gemm256_fused")]
  assert tuple(x - y for x, y in zip(after, before)) == stat, (tag, "dispatch", before, after, stat)
  return r


def _gemm_operands(r, akm, bkm):
  a = r["A"] if akm else r["A"].T
  bt = r["B"].T if bkm else r["B"]
  return a, bt


def gemm_row(dev, tag, M, N, K, akm, bkm, out_f32, epi="NONE", **kw):
  r = _gemm_call(dev, tag, M, N, K, akm, bkm, out_f32, epi, **kw)
  a, bt = _gemm_operands(r, akm, bkm)
  bias = kw.get("bias", True)
  acc = a.double() @ bt.double()
  pre = acc + (r["bias"].double() if bias else 0.0)
  leg = (1e-4, 1e-3) if out_f32 else (1e-2, 1e-2)
  C = r["C"]
  if epi == "NONE":
    B.check_gemm(C, pre, a, bt, legacy=leg, name=tag, n_adds=int(bias))
  elif epi == "RESIDUAL":
    B.check_gemm(C, pre + r["aux"].double(), a, bt, legacy=leg, name=tag, n_adds=2)
  elif epi == "POS":
    rows = kw["aux_rows"]
    B.check_gemm(C, pre + r["aux"].double()[torch.arange(M) % rows], a, bt, legacy=leg, name=tag, n_adds=2)
  elif epi == "ATOMIC":
    # the base and every split-K partial are one more fp32 add each (test_gemm_dw_layout); 256 x 256 kernel, auto: 2
    splits = kw.get("split_k", 0) or (2 if kw.get("stat", (0,))[0] else 1)
    B.check_gemm(C, r.inp["C"].double() + acc, a, bt, legacy=(1e-4, 1e-4 * math.sqrt(K) * 4), name=tag, n_adds=2 + splits)
  elif epi == "GELU":
    B.check_gemm(C, pre, a, bt, legacy=leg, name=tag + " h")
    B.check_gelu_g(r["C2"], C, legacy=(1e-2, 1e-2), name=tag + " g")
  elif epi in ("GELU_G", "GELU_GD"):
    # the activation of the bf16-rounded pre-activation, which these epilogues do not store: taken from a guarded
    # BV_EPI_GELU launch on the same operands (bit-identical, include/bvhip.h)
    r0 = _gemm_call(dev, tag + "/gelu", M, N, K, akm, bkm, out_f32, "GELU", **kw)
    assert torch.equal(r0["A"], r["A"]) and torch.equal(r0["B"], r["B"])
    assert torch.equal(C, r0["C2"]), f"{tag}: activation differs from the one BV_EPI_GELU writes"
    B.check_gelu_g(C, r0["C"], legacy=(1e-2, 1e-2), name=tag + " g")
    if epi == "GELU_GD":
      B.check_gelu_dg(r["C2"], r0["C"], legacy=(1e-2, 1e-2), name=tag + " g'")
  elif epi in ("GELU_BWD", "GELU_BWD_EMIT"):
    hh = r["aux"]
    B.check_gelu_bwd(C, a, bt, hh, legacy=(1e-2, 2e-2), name=tag)
    if epi == "GELU_BWD_EMIT":
      B.check_gelu_g(r["C2"], hh, legacy=(1e-2, 1e-2), name=tag + " emitted g")
    if kw.get("colsum"):
      ref = acc * B.dgelu_tanh64(hh)
      assert_close(r["colsum"], 0.5 + ref.sum(0), 1e-3, 1e-3 * ref.abs().sum(0).max().item(), tag + " colsum")
  elif epi == "MUL":
    B.check_mul(C, a, bt, r["aux"], legacy=(1e-2, 2e-2), name=tag)
    if kw.get("colsum"):
      ref = acc * r["aux"].double()
      assert_close(r["colsum"], 0.5 + ref.sum(0), 1e-3, 2e-3 * ref.abs().sum(0).max().item(), tag + " colsum")


def _gemm_rows():
  G = "bv_gemm_bf16"
  for akm, bkm in ((1, 0), (1, 1), (0, 0), (0, 1)):
    big = (130, 136, 72) if akm else (136, 136, 72)
    small = (5, 8, 8) if akm else ((8, 8, 5) if not bkm else (8, 8, 8))
    for shp in (big, small):
      for f32 in (1, 0):
        add(G, f"general-a{akm}b{bkm}-{'x'.join(map(str, shp))}-{'f32' if f32 else 'bf16'}", gemm_row,
            "general", *shp, akm, bkm, f32)
  add(G, "general-atomic-split3-64x72x333", gemm_row, "atomic split 3", 64, 72, 333, 0, 0, 1, "ATOMIC", bias=False, split_k=3)
  M, N, K = 130, 136, 72
  add(G, "general-residual-f32", gemm_row, "residual f32", M, N, K, 1, 0, 1, "RESIDUAL")
  add(G, "general-residual-bf16", gemm_row, "residual bf16", M, N, K, 1, 0, 0, "RESIDUAL")
  add(G, "general-pos-auxrows65", gemm_row, "pos", M, N, K, 1, 0, 1, "POS", aux_rows=65)
  add(G, "general-gelu-c2", gemm_row, "gelu", M, N, K, 1, 0, 0, "GELU")
  add(G, "general-gelu_bwd", gemm_row, "gelu'", M, N, K, 1, 1, 0, "GELU_BWD", bias=False)
  add("bv_gemm_bf16_colsum", "general-gelu_bwd-colsum", gemm_row, "gelu' colsum", M, N, K, 1, 1, 0, "GELU_BWD", bias=False,
      colsum=True)
  add(G, "general-gelu_bwd_emit", gemm_row, "gelu' emit", M, N, K, 1, 1, 0, "GELU_BWD_EMIT", bias=False)
  add(G, "general-gelu_gd", gemm_row, "gelu_gd", M, N, K, 1, 0, 0, "GELU_GD")
  add("bv_gemm_bf16_colsum", "general-mul-colsum", gemm_row, "mul colsum", M, N, K, 1, 1, 0, "MUL", bias=False, colsum=True)
  add(G, "general-gelu_g-c2-untouched", gemm_row, "gelu_g", M, N, K, 1, 0, 0, "GELU_G")
  # ---- 256 x 256 x 64 path
  M, N, K = 512, 512, 128
  one = (1, 0, 0)
  for epi, f32 in (("NONE", 0), ("NONE", 1), ("RESIDUAL", 1), ("RESIDUAL", 0), ("GELU", 0)):
    add(G, f"g256-{epi.lower()}-{'f32' if f32 else 'bf16'}", gemm_row, "g256", M, N, K, 1, 1, f32, epi, stat=one)
  for mask, epi, f32 in ((1, "RESIDUAL", 1), (2, "NONE", 0), (4, "GELU", 0), (8 | 2, "NONE", 0), (8 | 4, "GELU", 0)):
    add(G, f"g256-roll{mask}-{epi.lower()}", gemm_row, f"g256 roll {mask}", M, N, K, 1, 1, f32, epi, stat=one,
        opts=dict(gemm_roll=mask))
  for pre in (1, 2):
    add(G, f"g256-pre_issue{pre}", gemm_row, f"g256 pre_issue {pre}", M, N, K, 1, 1, 0, "GELU", stat=one,
        opts=dict(gemm_pre_issue=pre, gemm_roll=0))
    add(G, f"g256-pre_issue{pre}-roll", gemm_row, f"g256 pre_issue {pre} roll", M, N, K, 1, 1, 1, "RESIDUAL", stat=one,
        opts=dict(gemm_pre_issue=pre))
  for nt in (1, 2, 3):
    add(G, f"g256-nt{nt}", gemm_row, f"g256 nt {nt}", M, N, K, 1, 1, 0, "RESIDUAL", stat=one, opts=dict(gemm_nt=nt))
  add(G, "g256-group_n1", gemm_row, "g256 group_n 1", M, N, K, 1, 1, 0, "NONE", stat=one, opts=dict(gemm_group_n=1))
  # multi-tile: 33 x 4 = 132 tiles on the 128 CUs that gemm_reserve_cus = 128 leaves (BV_STAT_GEMM256_MULTI increments)
  M, N, K = 8448, 1024, 128
  for pre in (0, 2):
    add(G, f"g256-multi-pre_issue{pre}", gemm_row, f"g256 multi pre_issue {pre}", M, N, K, 1, 1, 0, "NONE", stat=(1, 1, 0),
        opts=dict(gemm_reserve_cus=128, gemm_pre_issue=pre))
    add("bv_gemm_bf16_colsum", f"g256-multi-colsum-pre_issue{pre}", gemm_row, f"g256 multi colsum pre_issue {pre}", M, N, K,
        1, 1, 0, "GELU_BWD", bias=False, colsum=True, stat=(1, 1, 1), opts=dict(gemm_reserve_cus=128, gemm_pre_issue=pre))
  # dW layout
  M, N, K = 256, 256, 1024
  add(G, "g256-dw-atomics", gemm_row, "g256 dW atomics", M, N, K, 0, 0, 1, "ATOMIC", bias=False, stat=one)
  add(G, "g256-dw-workspace-exact", gemm_row, "g256 dW workspace", M, N, K, 0, 0, 1, "ATOMIC", bias=False, ws="exact", stat=one)
  add(G, "g256-dw-workspace-exact-split3", gemm_row, "g256 dW workspace split 3", M, N, K, 0, 0, 1, "ATOMIC", bias=False,
      ws="exact", split_k=3, stat=one)


_gemm_rows()


def sgemm_row(dev, ta, tb, mfma):
  """A stored [K][M] (ta: sam = 1, sak = pitch) or [M][K]; B stored [K][N] (tb: sbk = pitch, sbn = 1) or [N][K]."""
  from big_vision_amd import ops
  M, N, K = 70, 133, 96
  ctx = ops.Context()
  ctx.set("sgemm_mfma", mfma)
  ash, bsh = ((K, M) if ta else (M, K)), ((K, N) if tb else (N, K))
  lda, ldb, ldc = ash[1] + PAD, bsh[1] + PAD, N + PAD

  def make():
    return [mat("A", F32, *ash, lda, tile_rows=64), mat("B", F32, *bsh, ldb, tile_rows=64),
            mat("C", F32, M, N, ldc, role="inout", fill=randn((M, N), 3), tile_rows=64),
            Op("log_alpha", F32, (1,), fill=torch.tensor([0.7]))]

  def launch(ar):
    sam, sak = (1, lda) if ta else (lda, 1)
    sbk, sbn = (ldb, 1) if tb else (1, ldb)
    call("bv_sgemm_strided", ar.ptr("A"), sam, sak, ar.ptr("B"), sbk, sbn, ar.ptr("C"), ldc, M, N, K, 2.0, 0.5,
         ar.ptr("log_alpha"), stream(), ctx.ptr)

  r = F.run("bv_sgemm_strided", f"ta{ta} tb{tb} mfma{mfma}", make, launch, dev)
  a = r["A"].double().T if ta else r["A"].double()
  b = r["B"].double() if tb else r["B"].double().T
  assert_close(r["C"], 0.5 * r.inp["C"].double() + 2.0 * math.exp(0.7) * (a @ b), 1e-5, 1e-4, "sgemm")


for _ta, _tb in ((1, 1), (0, 0), (1, 0)):
  for _m in (0, 1):
    add("bv_sgemm_strided", f"70x133x96-ta{_ta}-tb{_tb}-mfma{_m}", sgemm_row, _ta, _tb, _m)


# ----------------------------------------------------------- LayerNorm ------
def _ln_inputs(rows, D, xdt, seed=1):
  x = (randn((rows, D), seed, 2.0) + 0.5).to(xdt)
  scale = 1 + 0.1 * randn((D,), seed + 1)
  bias = 0.1 * randn((D,), seed + 2)
  return x, scale, bias


def _sel(rows, D, stride, offset):
  """Extent of the rows a strided launch selects in a [rows * stride][D] buffer."""
  return dict(strides=(stride * D, 1), offset=offset * D, alloc=rows * stride * D) if stride > 1 else {}


def ln_fwd_row(dev, entry, rows, D, stride=1, offset=0, want=("bf16", "f32")):
  xdt = BF16 if entry.endswith("bf16x") else F32
  x, scale, bias = _ln_inputs(rows, D, xdt)

  def make():
    o = [Op("x", xdt, (rows, D), fill=x, **_sel(rows, D, stride, offset)), Op("scale", F32, (D,), fill=scale),
         Op("bias", F32, (D,), fill=bias), Op("mean", F32, (rows,), "out"), Op("rstd", F32, (rows,), "out")]
    if "bf16" in want:
      o.append(Op("y_bf16", BF16, (rows, D), "out"))
    if "f32" in want:
      o.append(Op("y_f32", F32, (rows, D), "out"))
    return o

  def launch(ar):
    call(entry, ar.ptr("x"), ar.ptr("scale"), ar.ptr("bias"), ar.ptr("y_bf16") if "bf16" in want else None,
         ar.ptr("y_f32") if "f32" in want else None, ar.ptr("mean"), ar.ptr("rstd"), rows, D, stride, offset, 1e-6, stream())

  r = F.run(entry, f"{rows}x{D} stride {stride}", make, launch, dev)
  if "f32" in want:
    B.check_ln_fwd(r["y_f32"], r["x"], scale, bias, legacy=(1e-5, 1e-5), name="ln fwd f32")
  if "bf16" in want:
    B.check_ln_fwd(r["y_bf16"], r["x"], scale, bias, legacy=(1e-2, 1e-2), name="ln fwd bf16")
  mean, rstd, dmean, r_rel = B._ln_stats(r["x"])
  B.check(r["mean"], mean[:, 0], B.f32_bound(mean[:, 0], dmean[:, 0]), (1e-5, 1e-5), "ln mean")
  B.check(r["rstd"], rstd[:, 0], B.f32_bound(rstd[:, 0], (rstd * r_rel)[:, 0]), B.NO_LEGACY, "ln rstd")


def ln_bwd_row(dev, entry, rows, D, dy_f32, full, stride=1, offset=0):
  """full: dres, dx_bf16 (fp32 stream), dscale / dbias and dx_colsum all present; else none of them."""
  bfx = entry.endswith("bf16x")
  xdt = BF16 if bfx else F32
  x, scale, bias = _ln_inputs(rows, D, xdt)
  mean64, rstd64, _, _ = B._ln_stats(x)
  dy = randn((rows, D), 4, dtype=F32 if dy_f32 else BF16)
  dres = randn((rows, D), 5, dtype=xdt)
  sel = _sel(rows, D, stride, offset)
  with_y = entry == "bv_layernorm_bwd_y"

  def make():
    o = [Op("dy", dy.dtype, (rows, D), fill=dy), Op("x", xdt, (rows, D), fill=x, **sel), Op("scale", F32, (D,), fill=scale),
         Op("mean", F32, (rows,), fill=mean64[:, 0]), Op("rstd", F32, (rows,), fill=rstd64[:, 0])]
    if not bfx:
      o.append(Op("dx", F32, (rows, D), "out", **sel))
    if bfx or full:
      o.append(Op("dx_bf16", BF16, (rows, D), "out", **sel))
    if full:
      o += [Op("dres", xdt, (rows, D), fill=dres, **sel), Op("dscale", F32, (D,), "inout"), Op("dbias", F32, (D,), "inout"),
            Op("dx_colsum", F32, (D,), "inout")]
    if with_y:
      o += [Op("bias", F32, (D,), fill=bias), Op("y_bf16", BF16, (rows, D), "out")]
    return o

  def launch(ar):
    opt = lambda n: ar.ptr(n) if n in ar.ops else None
    head = [ar.ptr("dy"), int(dy_f32), ar.ptr("x"), ar.ptr("scale"), ar.ptr("mean"), ar.ptr("rstd"), opt("dres")]
    tail = [opt("dscale"), opt("dbias"), opt("dx_colsum"), rows, D, stride, offset]
    if bfx:
      call(entry, *head, ar.ptr("dx_bf16"), *tail, stream())
    elif with_y:
      call(entry, *head, ar.ptr("dx"), opt("dx_bf16"), *tail, ar.ptr("bias"), ar.ptr("y_bf16"), stream())
    else:
      call(entry, *head, ar.ptr("dx"), opt("dx_bf16"), *tail, stream())

  r = F.run(entry, f"{rows}x{D} dy {'f32' if dy_f32 else 'bf16'} full {full} stride {stride}", make, launch, dev)
  dr = dres if full else None
  if not bfx:
    B.check_ln_bwd(r["dx"], x, scale, dy, dres=dr, legacy=(1e-4, 1e-4), name="ln dx")
  if bfx or full:
    B.check_ln_bwd(r["dx_bf16"], x, scale, dy, dres=dr, legacy=(1e-2, 1e-2), name="ln dx bf16")
  if with_y:
    B.check_ln_fwd(r["y_bf16"], x, scale, bias, legacy=(1e-2, 1e-2), name="ln re-emitted y")
  if full:
    xr, sr, br = x.double().requires_grad_(True), scale.double().requires_grad_(True), bias.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), sr, br, eps=1e-6).backward(dy.double())
    assert_close(r["dscale"], 0.5 + sr.grad, 1e-4, 1e-3, "ln dscale")
    assert_close(r["dbias"], 0.5 + br.grad, 1e-4, 1e-3, "ln dbias")
    assert_close(r["dx_colsum"], 0.5 + (xr.grad + dres.double()).sum(0), 1e-4, 1e-3, "ln dx colsum")


def _ln_rows():
  for rows, D in ((9, 128), (9, 1152), (37, 384), (37, 2048)):
    for entry in ("bv_layernorm_fwd", "bv_layernorm_fwd_bf16x"):
      add(entry, f"{rows}x{D}", ln_fwd_row, entry, rows, D)
    for entry in ("bv_layernorm_bwd", "bv_layernorm_bwd_y", "bv_layernorm_bwd_bf16x"):
      add(entry, f"{rows}x{D}-dyf32-all-optionals", ln_bwd_row, entry, rows, D, 1, True)
      add(entry, f"{rows}x{D}-dybf16-no-optionals", ln_bwd_row, entry, rows, D, 0, False)
  add("bv_layernorm_fwd", "9x384-f32-only", ln_fwd_row, "bv_layernorm_fwd", 9, 384, want=("f32",))
  add("bv_layernorm_fwd", "9x384-bf16-only", ln_fwd_row, "bv_layernorm_fwd", 9, 384, want=("bf16",))
  # row_stride = 16, row_offset = 15 on 6 rows: only the selected rows of x are read and of dx written
  for entry in ("bv_layernorm_fwd", "bv_layernorm_fwd_bf16x"):
    add(entry, "strided-6x128-stride16-offset15", ln_fwd_row, entry, 6, 128, 16, 15)
  for entry in ("bv_layernorm_bwd", "bv_layernorm_bwd_bf16x"):
    add(entry, "strided-6x128-stride16-offset15", ln_bwd_row, entry, 6, 128, 1, False, 16, 15)


_ln_rows()


# ----------------------------------------------------------- attention ------
def _attn_ops(n, L, H, Dh, lens, seed):
  qkv = randn((n * L, 3 * H * Dh), seed, 1.5, BF16)
  band = L * 3 * H * Dh * 2     # one sample
  o = [Op("qkv", BF16, (n * L, 3 * H * Dh), fill=qkv, band=band)]
  if lens is not None:
    o.append(Op("kv_len", I32, (n,), fill=torch.tensor(lens, dtype=I32)))
  return qkv, band, o


def _lens(n, L, masked):
  return [1, L, max(1, L // 2), max(1, L - 1), 2][:n] if masked else None


def attn_fwd_row(dev, entry, n, L, H, Dh, masked, cfg=0):
  from big_vision_amd import ops
  lens = _lens(n, L, masked)
  ctx = ops.Context()
  ctx.set("attn_cfg", cfg)

  def make():
    _, band, o = _attn_ops(n, L, H, Dh, lens, 11)
    return o + [Op("o", BF16, (n * L, H * Dh), "out", band=band // 3), Op("lse", F32, (n, H, L), "out")]

  def launch(ar):
    a = [ar.ptr("qkv"), ar.ptr("o"), ar.ptr("lse")]
    if entry == "bv_attn_fwd":
      call(entry, *a, n, L, H, stream(), ctx.ptr)
    elif entry == "bv_attn_fwd_masked":
      call(entry, *a, ar.ptr("kv_len"), n, L, H, stream(), ctx.ptr)
    else:
      call(entry, *a, ar.ptr("kv_len") if masked else None, n, L, H, Dh, stream())

  r = F.run(entry, f"n{n} L{L} H{H} Dh{Dh} lens {lens} cfg {cfg}", make, launch, dev)
  B.check_attn_fwd(r["o"], r["lse"], r["qkv"], n, L, H, Dh, lens, legacy_o=(2e-2, 2e-2), legacy_lse=(1e-4, 1e-3))


def attn_bwd_row(dev, entry, n, L, H, Dh, masked, cfg=0):
  from big_vision_amd import ops
  lens = _lens(n, L, masked)
  ctx = ops.Context()
  ctx.set("attn_cfg", cfg)
  path = B.attn_bwd_path(L, Dh, masked, one_launch=not (cfg & 128))
  if "dq1" in path and (cfg & 16):
    path = "attn3 dq+dkv"
  qkv, band, _ = _attn_ops(n, L, H, Dh, lens, 11)
  o_ref, _, lse_ref, _ = B.attn_fwd_bounds(qkv, n, L, H, Dh, lens)
  d_o = randn((n * L, H * Dh), 12, dtype=BF16)

  def make():
    o = _attn_ops(n, L, H, Dh, lens, 11)[2]
    o += [Op("d_o", BF16, (n * L, H * Dh), fill=d_o, band=band // 3), Op("lse", F32, (n, H, L), fill=lse_ref),
          # the one-launch backward keeps delta in LDS and leaves the buffer alone (include/bvhip.h, ops.attn_bwd)
          Op("delta", F32, (n, H, L), "scratch" if path == "attn5" else "out"),
          Op("dqkv", BF16, (n * L, 3 * H * Dh), "out", band=band), Op("dbias_rows", F32, (n, 3 * H * Dh), "out")]
    if entry == "bv_attn_bwd":
      o.append(Op("o", BF16, (n * L, H * Dh), fill=o_ref, band=band // 3))
    return o

  def launch(ar):
    tail = [ar.ptr("delta"), ar.ptr("dqkv"), ar.ptr("dbias_rows"), n, L, H]
    if entry == "bv_attn_bwd":
      call(entry, ar.ptr("qkv"), ar.ptr("o"), ar.ptr("d_o"), ar.ptr("lse"), *tail, stream(), ctx.ptr)
    elif entry == "bv_attn_bwd_masked":
      call(entry, ar.ptr("qkv"), ar.ptr("d_o"), ar.ptr("lse"), ar.ptr("kv_len"), *tail, stream(), ctx.ptr)
    else:
      call(entry, ar.ptr("qkv"), ar.ptr("d_o"), ar.ptr("lse"), ar.ptr("kv_len") if masked else None, *tail, Dh, stream())

  r = F.run(entry, f"n{n} L{L} H{H} Dh{Dh} lens {lens} cfg {cfg} [{path}]", make, launch, dev)
  B.check_attn_bwd(r["dqkv"], qkv, d_o, n, L, H, Dh, lens, legacy=3e-2, delta=r.out.get("delta"),
                   dbias=r["dbias_rows"].double().sum(0), legacy_db=2e-2, path=path)
  if masked:
    dkv = r["dqkv"].view(n, L, 3, H, Dh)[:, :, 1:]
    for i, ln in enumerate(lens):
      assert (dkv[i, ln:] == 0).all(), "masked keys must get zero dK / dV"


def _attn_rows():
  for L in (5, 33, 197, 208, 209, 257, 441, 576):
    add("bv_attn_fwd", f"L{L}", attn_fwd_row, "bv_attn_fwd", 2, L, 2, 64, False)
    add("bv_attn_bwd", f"L{L}", attn_bwd_row, "bv_attn_bwd", 2, L, 2, 64, False)
    add("bv_attn_fwd_masked", f"L{L}", attn_fwd_row, "bv_attn_fwd_masked", 3, L, 2, 64, True)
    add("bv_attn_bwd_masked", f"L{L}", attn_bwd_row, "bv_attn_bwd_masked", 3, L, 2, 64, True)
  add("bv_attn_fwd", "cfg8-L197", attn_fwd_row, "bv_attn_fwd", 2, 197, 2, 64, False, 8)
  add("bv_attn_fwd_masked", "cfg8-L197", attn_fwd_row, "bv_attn_fwd_masked", 3, 197, 2, 64, True, 8)
  for bit, L in ((16, 257), (32, 257), (64, 257), (128, 33), (128, 197), (256, 33), (256, 197), (1024, 441)):
    add("bv_attn_bwd", f"cfg{bit}-L{L}", attn_bwd_row, "bv_attn_bwd", 2, L, 2, 64, False, bit)
  for bit, L in ((32, 441), (64, 576)):
    add("bv_attn_bwd_masked", f"cfg{bit}-L{L}", attn_bwd_row, "bv_attn_bwd_masked", 3, L, 2, 64, True, bit)
  # 21 (sample, head) pairs: the persistent workgroups of the one-launch backward end on a partial pair list
  add("bv_attn_bwd", "n7-H3-L33-partial-pair-list", attn_bwd_row, "bv_attn_bwd", 7, 33, 3, 64, False)
  # head dims other than 64; H = 1 puts the padded head at the end of the buffer
  for Dh, L in ((16, 16), (40, 70), (72, 300), (72, 16), (96, 70), (128, 300)):
    for H in (1, 2):
      for masked in (False, True):
        t = f"Dh{Dh}-H{H}-L{L}-{'masked' if masked else 'unmasked'}"
        add("bv_attn_fwd_dh", t, attn_fwd_row, "bv_attn_fwd_dh", 3, L, H, Dh, masked)
        add("bv_attn_bwd_dh", t, attn_bwd_row, "bv_attn_bwd_dh", 3, L, H, Dh, masked)


_attn_rows()


def map_row(dev, entry, n, L, H, Dh, masked):
  lens = [L, max(1, L // 2), 1, max(1, L - 1)][:n] if masked else None
  q = randn((n, H * Dh), 1, dtype=BF16)
  kv = randn((n * L, 2 * H * Dh), 2, dtype=BF16)
  d_o = randn((n, H * Dh), 3, dtype=BF16)
  band = L * 2 * H * Dh * 2
  bwd = "bwd" in entry
  p_ref = B.map_attn_fwd_bounds(q, kv, n, L, H, Dh, lens)[0] if bwd else None

  def make():
    o = [Op("q", BF16, (n, H * Dh), fill=q), Op("kv", BF16, (n * L, 2 * H * Dh), fill=kv, band=band)]
    if lens is not None and not bwd:
      o.append(Op("kv_len", I32, (n,), fill=torch.tensor(lens, dtype=I32)))
    if bwd:
      o += [Op("p", F32, (n, H, L), fill=p_ref), Op("d_o", BF16, (n, H * Dh), fill=d_o),
            Op("dq", BF16, (n, H * Dh), "out"), Op("dkv", BF16, (n * L, 2 * H * Dh), "out", band=band)]
    else:
      o += [Op("o", BF16, (n, H * Dh), "out"), Op("p", F32, (n, H, L), "out")]
    return o

  def launch(ar):
    if bwd:
      a = [ar.ptr("q"), ar.ptr("kv"), ar.ptr("p"), ar.ptr("d_o"), ar.ptr("dq"), ar.ptr("dkv"), n, L, H]
      call(entry, *a, *([Dh] if entry.endswith("_dh") else []), stream())
    else:
      a = [ar.ptr("q"), ar.ptr("kv"), ar.ptr("o"), ar.ptr("p")]
      if entry == "bv_map_attn_fwd":
        call(entry, *a, n, L, H, stream())
      elif entry == "bv_map_attn_fwd_masked":
        call(entry, *a, ar.ptr("kv_len"), n, L, H, stream())
      else:
        call(entry, *a, ar.ptr("kv_len") if masked else None, n, L, H, Dh, stream())

  r = F.run(entry, f"n{n} L{L} H{H} Dh{Dh} lens {lens}", make, launch, dev)
  if bwd:
    B.check_map_attn_bwd(r["dq"], r["dkv"], q, kv, d_o, n, L, H, Dh, lens, legacy=2e-2)
  else:
    B.check_map_attn_fwd(r["o"], r["p"], q, kv, n, L, H, Dh, lens, legacy_p=(1e-3, 1e-5), legacy_o=(1e-2, 1e-2))


def _map_rows():
  for L in (16, 70):
    add("bv_map_attn_fwd", f"L{L}", map_row, "bv_map_attn_fwd", 3, L, 2, 64, False)
    add("bv_map_attn_fwd_masked", f"L{L}", map_row, "bv_map_attn_fwd_masked", 3, L, 2, 64, True)
    for masked in (False, True):
      add("bv_map_attn_bwd", f"L{L}-{'masked' if masked else 'unmasked'}-p", map_row, "bv_map_attn_bwd", 3, L, 2, 64, masked)
      for Dh, H in ((72, 1), (16, 2)):
        t = f"Dh{Dh}-H{H}-L{L}-{'masked' if masked else 'unmasked'}"
        add("bv_map_attn_fwd_dh", t, map_row, "bv_map_attn_fwd_dh", 3, L, H, Dh, masked)
        add("bv_map_attn_bwd_dh", t, map_row, "bv_map_attn_bwd_dh", 3, L, H, Dh, masked)
  add("bv_map_attn_fwd_dh", "2x3000x1x64", map_row, "bv_map_attn_fwd_dh", 2, 3000, 1, 64, True)
  add("bv_map_attn_bwd_dh", "2x3000x1x64", map_row, "bv_map_attn_bwd_dh", 2, 3000, 1, 64, True)


_map_rows()


# --------------------------------------------------------- elementwise ------
def simple(entry, case, make, launch, check):
  """A row from three closures: make() -> operands, launch(arena), check(result)."""
  def fn(dev):
    check(F.run(entry, case, make, launch, dev))
  ROWS.append(((entry,), case, fn))


def _patchify_rows():
  import bv_oracle as O
  for P, res in ((14, 28), (16, 64)):
    n, K = 3, P * P * 3
    h = res // P
    img = torch.rand((n, res, res, 3), generator=gen(5)) * 2 - 1
    for entry, ldo in (("bv_patchify", K), ("bv_patchify_ld", (K + 7) // 8 * 8 + 8)):
      def make(ldo=ldo, img=img, K=K, h=h, n=n):
        return [Op("image", F32, img.shape, fill=img), mat("patches", BF16, n * h * h, ldo, ldo, role="out")]

      def launch(ar, entry=entry, ldo=ldo, res=res, P=P, n=n):
        if entry == "bv_patchify":
          call(entry, ar.ptr("image"), ar.ptr("patches"), n, res, res, P, stream())
        else:
          call(entry, ar.ptr("image"), ar.ptr("patches"), n, res, res, P, ldo, stream())

      def check(r, img=img, K=K, P=P):
        ref, _ = O.extract_patches(img, (P, P))
        assert torch.equal(r["patches"][:, :K], ref.reshape(-1, K).to(BF16))
        assert (r["patches"][:, K:] == 0).all()     # columns [P*P*3, ldo) are written as zeros (include/bvhip.h)

      simple(entry, f"P{P}-res{res}-ldo{ldo}", make, launch, check)


_patchify_rows()


def _embed_rows():
  n, L, D, V = 5, 16, 136, 50
  ids = torch.randint(0, V, (n, L), generator=gen(0), dtype=I32)
  ids[:, 10:] = 1
  ids[0, 0], ids[0, 1], ids[4, 15] = 0, V - 1, V - 1

  def make_f():
    return [Op("ids", I32, (n, L), fill=ids), Op("table", F32, (V, D)), Op("pos", F32, (L, D)), Op("x", F32, (n * L, D), "out")]

  def check_f(r):
    assert torch.equal(r["x"], r["table"][ids.long().view(-1)] + r["pos"].repeat(n, 1))

  simple("bv_embed_fwd", "ids-0-and-vocab-1-repeated", make_f,
         lambda ar: call("bv_embed_fwd", ar.ptr("ids"), ar.ptr("table"), ar.ptr("pos"), ar.ptr("x"), n, L, D, V, stream()), check_f)

  def make_b():
    return [Op("ids", I32, (n * L,), fill=ids.view(-1)), Op("dx", F32, (n * L, D)), Op("dtable", F32, (V, D), "inout")]

  def check_b(r):
    ref = torch.full((V, D), 0.5, dtype=F64).index_add_(0, ids.long().view(-1), r["dx"].double())
    assert_close(r["dtable"], ref, 1e-5, 1e-5, "embed bwd")

  simple("bv_embed_bwd", "ids-0-and-vocab-1-repeated", make_b,
         lambda ar: call("bv_embed_bwd", ar.ptr("ids"), ar.ptr("dx"), ar.ptr("dtable"), n * L, D, V, stream()), check_b)


_embed_rows()


def _reduction_rows():
  rows, cols = 37, 136
  for dt in (BF16, F32):
    simple("bv_colsum", f"37x136-pitched-{'f32' if dt == F32 else 'bf16'}",
           lambda dt=dt: [mat("x", dt, rows, cols, cols + PAD), Op("out", F32, (cols,), "inout")],
           lambda ar, dt=dt: call("bv_colsum", ar.ptr("x"), int(dt == F32), cols + PAD, ar.ptr("out"), rows, cols, stream()),
           lambda r: assert_close(r["out"], 0.5 + r["x"].double().sum(0), 1e-5, 1e-3, "colsum"))
  n, L, D = 5, 7, 36
  simple("bv_batchsum", "5x7x36", lambda: [Op("x", F32, (n, L, D)), Op("out", F32, (L, D), "inout")],
         lambda ar: call("bv_batchsum", ar.ptr("x"), ar.ptr("out"), n, L, D, stream()),
         lambda r: assert_close(r["out"], 0.5 + r["x"].double().sum(0), 1e-5, 1e-4, "batchsum"))
  for count in (8, 24):
    simple("bv_cast_bf16", f"count{count}", lambda c=count: [Op("x", F32, (c,)), Op("y", BF16, (c,), "out")],
           lambda ar, c=count: call("bv_cast_bf16", ar.ptr("x"), ar.ptr("y"), c, stream()),
           lambda r: _eq(r["y"], r["x"].to(BF16), "cast_bf16"))
    simple("bv_cast_f32", f"count{count}", lambda c=count: [Op("x", BF16, (c,)), Op("y", F32, (c,), "out")],
           lambda ar, c=count: call("bv_cast_f32", ar.ptr("x"), ar.ptr("y"), c, stream()),
           lambda r: _eq(r["y"], r["x"].float(), "cast_f32"))
  R, C = 70, 130
  simple("bv_transpose_bf16", "70x130-pitched",
         lambda: [mat("src", BF16, R, C, C + PAD, tile_rows=64), mat("dst", BF16, C, R, R + 2 + PAD, role="out", tile_rows=64)],
         lambda ar: call("bv_transpose_bf16", ar.ptr("src"), ar.ptr("dst"), R, C, C + PAD, R + 2 + PAD, stream()),
         lambda r: _eq(r["dst"], r["src"].T, "transpose"))
  shapes = [(70, 130), (1, 8), (64, 64)]

  def make_t():
    o = []
    for i, (rr, cc) in enumerate(shapes):
      o += [mat(f"src{i}", BF16, rr, cc, cc + PAD * (i % 2), tile_rows=64),
            mat(f"dst{i}", BF16, cc, rr, (rr + 7) // 8 * 8 + PAD, role="out", tile_rows=64)]
    return o + [Op("leaves", U8, (len(shapes) * 48,), fill=torch.zeros(len(shapes) * 48))]

  def tiles_of():
    return sum(((cc + 63) // 64) * ((rr + 63) // 64) for rr, cc in shapes)

  def prepare_t(ar):
    """The leaf table holds this arena's addresses: written before the snapshot, an input like any other after it."""
    from big_vision_amd import ops
    tab = np.zeros(len(shapes), ops.TR_LEAF)
    assert tab.itemsize == 48   # struct bv_tr_leaf
    tiles = 0
    for i, (rr, cc) in enumerate(shapes):
      tx = (cc + 63) // 64
      tab[i] = (ar.ptr(f"src{i}"), ar.ptr(f"dst{i}"), cc + PAD * (i % 2), (rr + 7) // 8 * 8 + PAD, rr, cc, tiles, tx)
      tiles += tx * ((rr + 63) // 64)
    ar.view("leaves").copy_(torch.from_numpy(tab.view(np.uint8).copy()))

  def row_t(dev):
    r = F.run("bv_transpose_bf16_batched", "three-leaves", make_t,
              lambda ar: call("bv_transpose_bf16_batched", ar.ptr("leaves"), len(shapes), tiles_of(), stream()), dev,
              prepare=prepare_t)
    for i in range(len(shapes)):
      _eq(r[f"dst{i}"], r[f"src{i}"].T, f"batched transpose leaf {i}")

  ROWS.append((("bv_transpose_bf16_batched",), "three-leaves", row_t))
  simple("bv_concat_cls", "5x7x36", lambda: [Op("cls", F32, (D,)), Op("x", F32, (n, L, D)), Op("y", F32, (n, L + 1, D), "out")],
         lambda ar: call("bv_concat_cls", ar.ptr("cls"), ar.ptr("x"), ar.ptr("y"), n, L, D, stream()),
         lambda r: _eq(r["y"], torch.cat([r["cls"].expand(n, 1, D), r["x"]], 1), "concat_cls"))


def _eq(a, b, name):
  assert torch.equal(a, b), f"{name}: not bit-identical"


_reduction_rows()


def _pool_rows():
  n, L, D = 5, 7, 36
  lens = torch.tensor([1, L, 3, L - 1, 2], dtype=I32)
  x = randn((n, L, D), 71)
  dy = randn((n, D), 72)
  mask = (torch.arange(L)[None, :] < lens[:, None].long())
  simple("bv_pool_gap_fwd", "5x7x36", lambda: [Op("x", F32, (n, L, D), fill=x), Op("y", F32, (n, D), "out")],
         lambda ar: call("bv_pool_gap_fwd", ar.ptr("x"), ar.ptr("y"), n, L, D, stream()),
         lambda r: assert_close(r["y"], x.double().mean(1), 1e-5, 1e-6, "gap"))
  simple("bv_pool_gap_bwd", "5x7x36", lambda: [Op("dy", F32, (n, D), fill=dy), Op("dx", F32, (n, L, D), "out")],
         lambda ar: call("bv_pool_gap_bwd", ar.ptr("dy"), ar.ptr("dx"), n, L, D, stream()),
         lambda r: assert_close(r["dx"], (dy.double() / L)[:, None, :].expand(n, L, D), 1e-6, 1e-7, "gap bwd"))
  lo = lambda: Op("len", I32, (n,), fill=lens)
  ref_m = (x.double() * mask[:, :, None]).sum(1) / lens.double()[:, None]
  simple("bv_pool_gap_masked_fwd", "5x7x36-len-1-and-L", lambda: [Op("x", F32, (n, L, D), fill=x), lo(), Op("y", F32, (n, D), "out")],
         lambda ar: call("bv_pool_gap_masked_fwd", ar.ptr("x"), ar.ptr("y"), ar.ptr("len"), n, L, D, stream()),
         lambda r: assert_close(r["y"], ref_m, 1e-5, 1e-6, "masked gap"))
  ref_mb = (dy.double() / lens.double()[:, None])[:, None, :] * mask[:, :, None]
  simple("bv_pool_gap_masked_bwd", "5x7x36-len-1-and-L", lambda: [Op("dy", F32, (n, D), fill=dy), lo(), Op("dx", F32, (n, L, D), "out")],
         lambda ar: call("bv_pool_gap_masked_bwd", ar.ptr("dy"), ar.ptr("dx"), ar.ptr("len"), n, L, D, stream()),
         lambda r: assert_close(r["dx"], ref_mb, 1e-6, 1e-7, "masked gap bwd"))
  ymax, amax = x.max(dim=1)

  def check_max(r, y=ymax, a=amax):
    _eq(r["y"], y, "pool max")
    _eq(r["argmax"].long(), a, "pool argmax")

  simple("bv_pool_max_fwd", "5x7x36-argmax",
         lambda: [Op("x", F32, (n, L, D), fill=x), Op("y", F32, (n, D), "out"), Op("argmax", I32, (n, D), "out")],
         lambda ar: call("bv_pool_max_fwd", ar.ptr("x"), ar.ptr("y"), ar.ptr("argmax"), n, L, D, stream()), check_max)
  ym, am = x.masked_fill(~mask[:, :, None], float("-inf")).max(dim=1)
  simple("bv_pool_max_masked_fwd", "5x7x36-argmax-len-1-and-L",
         lambda: [Op("x", F32, (n, L, D), fill=x), Op("y", F32, (n, D), "out"), Op("argmax", I32, (n, D), "out"), lo()],
         lambda ar: call("bv_pool_max_masked_fwd", ar.ptr("x"), ar.ptr("y"), ar.ptr("argmax"), ar.ptr("len"), n, L, D, stream()),
         lambda r: check_max(r, ym, am))
  ref_xb = torch.zeros((n, L, D)).scatter_(1, amax[:, None, :], dy[:, None, :])
  simple("bv_pool_max_bwd", "5x7x36-argmax",
         lambda: [Op("dy", F32, (n, D), fill=dy), Op("argmax", I32, (n, D), fill=amax.to(I32)), Op("dx", F32, (n, L, D), "out")],
         lambda ar: call("bv_pool_max_bwd", ar.ptr("dy"), ar.ptr("argmax"), ar.ptr("dx"), n, L, D, stream()),
         lambda r: _eq(r["dx"], ref_xb, "pool max bwd"))


_pool_rows()


def _misc_rows():
  import bv_oracle as O
  P, grids = 16, [(8, 12), (16, 16), (3, 1)]
  n, N = len(grids), max(h * w for h, w in grids) + 3
  yabs = torch.zeros((n, N), dtype=I32); xabs = torch.zeros((n, N), dtype=I32)
  for e, (h, w) in enumerate(grids):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    yabs[e, :h * w] = yy.flatten(); xabs[e, :h * w] = xx.flatten()

  def check_w(r):
    ref = []
    for e, (h, w) in enumerate(grids):
      wy = O.scale_and_translate_weights(P, 64, h / P)[:, yabs[e].long()]
      wx = O.scale_and_translate_weights(P, 64, w / P)[:, xabs[e].long()]
      ref.append((wy[:, None, :] * wx[None, :, :]).reshape(P * P, N).T)
    assert_close(r["W"], torch.cat(ref), 1e-2, 1e-3, "naflex position-embedding weights")

  simple("bv_naflex_posemb_weights", "P16-three-grids",
         lambda: [Op("yabs", I32, (n, N), fill=yabs), Op("xabs", I32, (n, N), fill=xabs), Op("W", BF16, (n * N, P * P), "out")],
         lambda ar: call("bv_naflex_posemb_weights", ar.ptr("yabs"), ar.ptr("xabs"), ar.ptr("W"), n, N, P, stream()), check_w)
  rows, D = 7, 136
  z = randn((rows, D), 1, 3.0)
  dzn = randn((rows, D), 2)
  zr = z.double().requires_grad_(True)
  nr = torch.linalg.norm(zr, dim=1, keepdim=True)
  ref = zr / (nr + 1e-8)
  ref.backward(dzn.double())

  def check_l2(r):
    assert_close(r["zn"], ref.detach(), 1e-5, 1e-6, "l2norm")
    assert_close(r["norm"], nr.detach()[:, 0], 1e-5, 1e-6, "norm")

  simple("bv_l2norm_fwd", "7x136", lambda: [Op("z", F32, (rows, D), fill=z), Op("zn", F32, (rows, D), "out"), Op("norm", F32, (rows,), "out")],
         lambda ar: call("bv_l2norm_fwd", ar.ptr("z"), ar.ptr("zn"), ar.ptr("norm"), rows, D, 1e-8, stream()), check_l2)
  simple("bv_l2norm_bwd", "7x136",
         lambda: [Op("z", F32, (rows, D), fill=z), Op("norm", F32, (rows,), fill=nr.detach()[:, 0]), Op("dzn", F32, (rows, D), fill=dzn),
                  Op("dz", F32, (rows, D), "out")],
         lambda ar: call("bv_l2norm_bwd", ar.ptr("z"), ar.ptr("norm"), ar.ptr("dzn"), ar.ptr("dz"), rows, D, 1e-8, stream()),
         lambda r: assert_close(r["dz"], zr.grad, 1e-4, 1e-6, "l2norm bwd"))
  cnt = 7 * 384 + 3
  xt = randn((cnt,), 5, 2.0)
  simple("bv_tanh_fwd", f"count{cnt}", lambda: [Op("x", F32, (cnt,), fill=xt), Op("y", F32, (cnt,), "out")],
         lambda ar: call("bv_tanh_fwd", ar.ptr("x"), ar.ptr("y"), cnt, stream()),
         lambda r: assert_close(r["y"], torch.tanh(xt.double()), 1e-6, 1e-6, "tanh"))
  yt = torch.tanh(xt.double()).float()
  simple("bv_tanh_bwd", f"count{cnt}", lambda: [Op("y", F32, (cnt,), fill=yt), Op("dy", F32, (cnt,)), Op("dx", F32, (cnt,), "out")],
         lambda ar: call("bv_tanh_bwd", ar.ptr("y"), ar.ptr("dy"), ar.ptr("dx"), cnt, stream()),
         lambda r: assert_close(r["dx"], r["dy"].double() * (1 - torch.tanh(xt.double()) ** 2), 1e-5, 1e-6, "tanh bwd"))
  nm, re_ = 5, 8 * 8 * 3 + 1
  simple("bv_mixup", f"5x{re_}-odd-row", lambda: [Op("x", F32, (nm, re_)), Op("out", F32, (nm, re_), "out")],
         lambda ar: call("bv_mixup", ar.ptr("x"), ar.ptr("out"), 0.7, nm, re_, stream()),
         lambda r: assert_close(r["out"], 0.7 * r["x"].double() + 0.3 * torch.roll(r["x"].double(), 1, 0), 1e-6, 1e-6, "mixup"))


_misc_rows()


# ------------------------------------------------- loss and reductions ------
def _loss_rows():
  import bv_oracle as O
  for n, Bn, off in ((7, 21, 14), (48, 192, 96)):
    zi = torch.nn.functional.normalize(randn((n, 32), 1), dim=1)
    zt = torch.nn.functional.normalize(randn((Bn, 32), 2), dim=1)
    zt[off:off + n] = 0.7 * zt[off:off + n] + 0.3 * zi
    raw = (zi @ zt.T).contiguous()
    tp, bp = torch.tensor([math.log(10.0)]), torch.tensor([-2.71])

    def check_s(r, raw=raw, n=n, Bn=Bn, off=off):
      lg = (raw.double() * torch.exp(tp.double()) + bp.double()).requires_grad_(True)
      tpd = tp.double().requires_grad_(True); bpd = bp.double().requires_grad_(True)
      logits = raw.double() * torch.exp(tpd) + bpd
      m = -torch.ones_like(logits); m[torch.arange(n), off + torch.arange(n)] = 1.0
      loss = (-O.log_sigmoid(m * logits).sum(-1)).sum() / Bn
      loss.backward()
      (-O.log_sigmoid(m * lg).sum(-1)).sum().div(Bn).backward()
      st = r["stats"]
      assert_close(st[0], 0.5 + loss.detach(), 1e-5, 1e-6, "loss")
      assert_close(st[1], 0.5 + tpd.grad[0], 1e-4, 1e-6, "dt'")
      assert_close(st[2], 0.5 + bpd.grad[0], 1e-4, 1e-6, "db")
      B.check(r["raw"], lg.grad, None, legacy=(1e-4, 1e-7), name="siglip G")

    simple("bv_siglip_loss", f"n{n}-B{Bn}-off{off}",
           lambda raw=raw, n=n, Bn=Bn: [Op("raw", F32, (n, Bn), "inout", fill=raw), Op("t", F32, (1,), fill=tp), Op("b", F32, (1,), fill=bp),
                                        Op("stats", F64, (3,), "inout")],
           lambda ar, n=n, Bn=Bn, off=off: call("bv_siglip_loss", ar.ptr("raw"), ar.ptr("t"), ar.ptr("b"), ar.ptr("stats"), n, Bn, off, Bn, stream()),
           check_s)
  n, Bn, off = 7, 21, 14
  raw = randn((n, Bn), 51)
  t7, b7 = torch.tensor([math.log(7.0)]), torch.tensor([-1.5])

  def check_ls(r):
    lg = 7.0 * raw.double() - 1.5
    rows = torch.arange(n)
    pos = torch.zeros((n, Bn), dtype=torch.bool); pos[rows, off + rows] = True
    loc = torch.zeros_like(pos); loc[:, off:off + n] = True
    ref = torch.stack([f(s) for s in (lg[pos], lg[loc & ~pos], lg[~pos]) for f in (torch.min, torch.max, torch.mean)])
    assert_close(r["out9"], ref, 1e-5, 1e-5, "logit stats")

  simple("bv_logit_stats", "n7-B21-off14",
         lambda: [Op("raw", F32, (n, Bn), fill=raw), Op("t", F32, (1,), fill=t7), Op("b", F32, (1,), fill=b7),
                  Op("part", F32, (512 * 9,), "scratch"), Op("out9", F32, (9,), "out")],
         lambda ar: call("bv_logit_stats", ar.ptr("raw"), ar.ptr("t"), ar.ptr("b"), ar.ptr("part"), ar.ptr("out9"), n, Bn, off, stream()),
         check_ls)
  for count in (1, 1023, 4096 + 5):
    simple("bv_dot_f32", f"count{count}",
           lambda c=count: [Op("a", F32, (c,)), Op("b", F32, (c,)), Op("out", F64, (1,), "inout")],
           lambda ar, c=count: call("bv_dot_f32", ar.ptr("a"), ar.ptr("b"), c, ar.ptr("out"), stream()),
           lambda r, c=count: assert_close(r["out"], 0.5 + (r["a"].double() * r["b"].double()).sum().reshape(1), 1e-6, 1e-6 * c ** 0.5, "dot"))
    simple("bv_sqnorm", f"count{count}",
           lambda c=count: [Op("x", F32, (c,)), Op("out", F64, (1,), "inout", fill=torch.zeros(1))],
           lambda ar, c=count: call("bv_sqnorm", ar.ptr("x"), c, ar.ptr("out"), stream()),
           lambda r: assert_close(r["out"], (r["x"].double() ** 2).sum().reshape(1), 1e-6, 0, "sqnorm"))
  for entry, fn in (("bv_softmax_xent", O.softmax_xent), ("bv_sigmoid_xent", O.sigmoid_xent)):
    for C in (10, 1001):
      for grad in (True, False):
        logits = randn((6, C), 71, 3.0)
        labels = torch.softmax(randn((6, C), 72, 2.0), -1)

        def check_x(r, logits=logits, labels=labels, fn=fn, grad=grad):
          lr = logits.double().requires_grad_(True)
          ref = fn(lr, labels.double())
          ref.backward()
          assert_close(r["loss"], 0.5 + ref.detach().reshape(1), 1e-5, 1e-5 if fn is O.sigmoid_xent else 1e-6, "xent")
          if grad:
            assert_close(r["dlogits"], lr.grad, 1e-4, 1e-7, "dlogits")

        simple(entry, f"C{C}-{'with' if grad else 'without'}-dlogits",
               lambda logits=logits, labels=labels, grad=grad, C=C: (
                   [Op("logits", F32, (6, C), fill=logits), Op("labels", F32, (6, C), fill=labels), Op("loss", F64, (1,), "inout")]
                   + ([Op("dlogits", F32, (6, C), "out")] if grad else [])),
               lambda ar, entry=entry, grad=grad, C=C: call(entry, ar.ptr("logits"), ar.ptr("labels"), ar.ptr("loss"),
                                                            ar.ptr("dlogits") if grad else None, 6, C, 6, stream()),
               check_x)


_loss_rows()


# ----------------------------------------------------------- optimizers -----
def opt_row(dev, entry, mom_bf16, shadow):
  """Five 1024-element chunks in three segments (2 + 1 + 2), clip active, two schedule values."""
  count, chunk_seg = 5 * 1024, [0, 0, 1, 2, 2]
  segv = [(1e-2, 1e-2, 0), (5e-3, 0.0, 1), (2e-2, 1e-3, 0)]
  sched = [0.7, 0.3]
  seg_t = np.zeros(3, np.dtype([("lr", np.float32), ("wd", np.float32), ("si", np.int32), ("pad", np.int32)]))
  for i, s in enumerate(segv):
    seg_t[i] = s + (0,)
  adam = entry == "bv_adam_step"
  mdt = BF16 if mom_bf16 else F32
  p0, g0 = randn((count,), 1), randn((count,), 2, 3.0)
  m0, v0 = randn((count,), 3, 0.1, mdt), randn((count,), 4, 0.1).abs()
  gsq0 = (g0.double() ** 2).sum().reshape(1)
  arr = (ctypes.c_float * len(sched))(*sched)
  b1, b2, eps, k, clipn, beta = 0.9, 0.999, 1e-8, 3, 1.0, 0.9

  def make():
    o = [Op("params", F32, (count,), "inout", fill=p0), Op("grads", F32, (count,), fill=g0), Op("mu", mdt, (count,), "inout", fill=m0),
         Op("segs", U8, (48,), fill=torch.from_numpy(seg_t.view(np.uint8).copy())), Op("chunk_seg", I32, (5,), fill=torch.tensor(chunk_seg, dtype=I32)),
         Op("gsq", F64, (1,), fill=gsq0), Op("stats", F64, (2,), "inout")]
    if adam:
      o.append(Op("nu", F32, (count,), "inout", fill=v0))
    if shadow:
      o.append(Op("shadow", BF16, (count,), "out"))
    return o

  def launch(ar):
    sh = ar.ptr("shadow") if shadow else None
    sp = ctypes.cast(arr, ctypes.c_void_p)
    if adam:
      call(entry, ar.ptr("params"), ar.ptr("grads"), ar.ptr("mu"), int(mom_bf16), ar.ptr("nu"), sh, ar.ptr("segs"), ar.ptr("chunk_seg"),
           count, sp, len(sched), ar.ptr("gsq"), clipn, b1, b2, eps, 1 - b1 ** k, 1 - b2 ** k, ar.ptr("stats"), stream())
    else:
      call(entry, ar.ptr("params"), ar.ptr("grads"), ar.ptr("mu"), int(mom_bf16), sh, ar.ptr("segs"), ar.ptr("chunk_seg"), count, sp,
           len(sched), ar.ptr("gsq"), clipn, beta, 0, ar.ptr("stats"), stream())

  r = F.run(entry, f"mu {'bf16' if mom_bf16 else 'f32'} shadow {shadow}", make, launch, dev)
  seg = torch.tensor(chunk_seg).repeat_interleave(1024)
  lr = torch.tensor([s[0] for s in segv], dtype=F64)[seg]
  wd = torch.tensor([s[1] for s in segv], dtype=F64)[seg]
  sc = torch.tensor(sched, dtype=F64)[torch.tensor([s[2] for s in segv])[seg]]
  g = g0.double() * min(1.0, clipn / math.sqrt(gsq0.item()))
  if adam:
    m = b1 * m0.double() + (1 - b1) * g
    v = b2 * v0.double() + (1 - b2) * g * g
    u = (m / (1 - b1 ** k)) / (torch.sqrt(v / (1 - b2 ** k)) + eps)
    assert_close(r["nu"], v, 1e-5, 1e-6, "nu")
  else:
    m = g + beta * m0.double()
    u = m
  upd = sc * (lr * u + wd * p0.double())
  pn = p0.double() - upd
  # tolerances of test_sqnorm_and_adam_vs_oracle; a bf16 moment is one rounding (2^-8) of the fp32 value
  assert_close(r["params"], pn, 1e-5, 1e-6, "params")
  assert_close(r["mu"], m, 2.0 ** -8 if mom_bf16 else 1e-5, 1e-6, "mu")
  if shadow:
    _eq(r["shadow"], r["params"].to(BF16), "bf16 shadow")
  assert_close(r["stats"][0], 0.5 + (pn ** 2).sum(), 1e-5, 0, "l2_params^2")
  assert_close(r["stats"][1], 0.5 + (upd ** 2).sum(), 1e-4, 1e-12, "l2_updates^2")
  for name in ("segs", "chunk_seg", "gsq"):
    _eq(r.arena.get(name), r.inp[name], name)


for _e in ("bv_adam_step", "bv_trace_step"):
  for _mb in (1, 0):
    for _sh in (True, False):
      add(_e, f"mu-{'bf16' if _mb else 'f32'}-{'with' if _sh else 'without'}-shadow", opt_row, _e, _mb, _sh)


AF_LEAF = np.dtype([("off", np.int64), ("sB1", np.int64), ("sB2", np.int64), ("sR", np.int64), ("sC", np.int64),
                    ("soff", np.int64), ("B1", np.int32), ("B2", np.int32), ("R", np.int32), ("C", np.int32),
                    ("factored", np.int32), ("sched_idx", np.int32), ("r_fast", np.int32), ("pad_", np.int32),
                    ("lr_eff", np.float32), ("wd", np.float32)], align=True)   # struct bv_af_leaf (include/bvhip.h)
AF = dict(decay=0.8, eps=1e-30, mom=0.9, clip=1.0)
AF_SCHED = [0.7, 0.3]
AF_TOTAL = 6400 + 131 + 61     # elements of the params / grads / momentum / shadow buffers the leaves live in


def _af_leaves(which):
  """Leaves at offsets inside larger buffers: factored (37, 130), factored (40, 33), unfactored 131 elements.  Their
  statistics sit at soff in one state buffer, each padded to a multiple of 4 floats as the optimizer lays them out."""
  leaves = [dict(off=64, R=37, C=130, f=1, lr=1e-2, wd=1e-2, si=0), dict(off=5000, R=40, C=33, f=1, lr=5e-3, wd=0.0, si=1),
            dict(off=6400, R=1, C=131, f=0, lr=2e-2, wd=1e-3, si=0)]
  soff = 0
  for lf in leaves:
    lf["n"] = lf["R"] * lf["C"]
    lf["ns"] = lf["R"] + lf["C"] + 1 if lf["f"] else lf["n"]
    lf["soff"] = soff
    lf["sR"] = lf["C"] if lf["f"] else 0
    soff += (lf["ns"] + 3) // 4 * 4
  return [leaves[i] for i in which], soff


def _af_ref(p, g, m, st, lf, clipf, block_clip=0.0):
  """fp64 statement of one leaf (big_vision/optax.py:187-216 as restated by bv_oracle._adafactor, with
  optax.clip_by_block_rms when block_clip > 0): (p_new, m_new (unrounded), state_new, update)."""
  R, C = lf["R"], lf["C"]
  g = g.double() * clipf
  g2 = g * g + AF["eps"]
  d = AF["decay"]
  if lf["f"]:
    g2 = g2.view(R, C)
    vr = d * st[:R].double() + (1 - d) * g2.mean(1)
    vc = d * st[R:R + C].double() + (1 - d) * g2.mean(0)
    rcm = vr.mean()
    u = (g.view(R, C) * ((vr / rcm) ** -0.5)[:, None] * (vc ** -0.5)[None, :]).reshape(-1)
    stn = torch.cat([vr, vc, rcm.reshape(1)])
  else:
    stn = d * st.double() + (1 - d) * g2
    u = g * stn ** -0.5
  if block_clip > 0:
    u = u / max(1.0, math.sqrt((u ** 2).mean().item()) / block_clip)
  mn = AF["mom"] * m.double() + (1 - AF["mom"]) * u
  upd = AF_SCHED[lf["si"]] * (lf["lr"] * mn + lf["wd"] * p.double())
  return p.double() - upd, mn, stn, upd


def _af_run(dev, entry, case, leaves, soff, mom_bf16, block_clip, launch):
  """The guarded call and its value check, shared by the two entry points.  The extents of params / momentum / shadow /
  grads are the leaves' runs and those of `state` the leaves' statistics: the elements between the leaves and the
  padding between the statistics belong to no extent and must not change.  Values: parameters within 2e-5 of the
  largest parameter and l2_updates within 2e-3 (test_adafactor_gpu.py); the fp32 momentum, the statistics and sum p^2
  at the fp32 optimizer tolerance of test_sqnorm_and_adam_vs_oracle (rtol 1e-5, atol 1e-6; 1e-5 on the sums); a bf16
  momentum is the fp32 value rounded once (2^-8: the update itself takes the unrounded value, adafactor.hip)."""
  mdt = BF16 if mom_bf16 else F32
  p0, g0, m0 = randn((AF_TOTAL,), 1), randn((AF_TOTAL,), 2, 3.0), randn((AF_TOTAL,), 3, 0.1, mdt)
  st0 = randn((soff,), 4).abs() + 0.1
  gsq0 = (g0.double() ** 2).sum().reshape(1)
  clipf = min(1.0, AF["clip"] / math.sqrt(gsq0.item()))
  runs = [(lf["off"], lf["n"]) for lf in leaves]
  sruns = [(lf["soff"], lf["ns"]) for lf in leaves]

  def make():
    buf = dict(runs=runs, alloc=AF_TOTAL)
    o = [Op("params", F32, role="inout", fill=p0, **buf), Op("grads", F32, fill=g0, **buf),
         Op("momentum", mdt, role="inout", fill=m0, **buf), Op("shadow", BF16, role="out", **buf),
         Op("state", F32, role="inout", fill=st0, runs=sruns, alloc=soff), Op("gsq", F64, (1,), fill=gsq0),
         Op("stats", F64, (2,), "inout")]
    if entry == "bv_adafactor_step":
      tab = np.zeros(len(leaves), AF_LEAF)
      for i, lf in enumerate(leaves):
        tab[i] = (lf["off"], 0, 0, lf["sR"], 1, lf["soff"], 1, 1, lf["R"], lf["C"], lf["f"], lf["si"], int(lf["sR"] < 1), 0,
                  lf["lr"], lf["wd"])
      o.append(Op("leaves", U8, (tab.nbytes,), fill=torch.from_numpy(tab.view(np.uint8).copy())))
    if block_clip > 0:
      o.append(Op("block_usq", F64, (len(leaves),), "scratch"))
    return o

  r = F.run(entry, case, make, launch, dev)
  at = sat = 0
  sp = su = 0.0
  pmax = p0.abs().max().item()
  for lf in leaves:
    sl, ssl = slice(lf["off"], lf["off"] + lf["n"]), slice(lf["soff"], lf["soff"] + lf["ns"])
    pn, mn, stn, upd = _af_ref(p0[sl], g0[sl], m0[sl], st0[ssl], lf, clipf, block_clip)
    a, b = at, at + lf["n"]
    tag = f"{case}: leaf {lf['R']}x{lf['C']}"
    assert_close(r["params"][a:b], pn, 0, 2e-5 * max(1.0, pmax), tag + " params")
    assert_close(r["momentum"][a:b], mn, 2.0 ** -8 if mom_bf16 else 1e-5, 1e-6, tag + " momentum")
    assert_close(r["state"][sat:sat + lf["ns"]], stn, 1e-5, 1e-6, tag + " statistics")
    _eq(r["shadow"][a:b], r["params"][a:b].to(BF16), tag + " shadow")
    sp += (pn ** 2).sum().item(); su += (upd ** 2).sum().item()
    at, sat = b, sat + lf["ns"]
  assert abs(r["stats"][0].item() - 0.5 - sp) <= 1e-5 * sp, f"{case}: sum p^2"
  assert abs(math.sqrt(r["stats"][1].item() - 0.5) - math.sqrt(su)) <= 2e-3 * math.sqrt(su), f"{case}: l2_updates"


def af_leaf_row(dev, which, mom_bf16):
  (lf,), soff = _af_leaves([which])
  view = (ctypes.c_long * 9)(lf["off"], 1, 1, lf["R"], lf["C"], 0, 0, lf["sR"], 1)

  def launch(ar):
    call("bv_adafactor_leaf", ar.ptr("params"), ar.ptr("grads"), ar.ptr("momentum"), int(mom_bf16), ar.ptr("shadow"),
         ctypes.cast(view, ctypes.c_void_p), ar.ptr("state") + 4 * lf["soff"], lf["f"], ar.ptr("gsq"), AF["clip"], AF["decay"],
         AF["eps"], AF["mom"], lf["lr"], lf["wd"], AF_SCHED[lf["si"]], ar.ptr("stats"), stream())

  _af_run(dev, "bv_adafactor_leaf", f"leaf {lf['R']}x{lf['C']} mom {'bf16' if mom_bf16 else 'f32'}", [lf], soff, mom_bf16, 0.0,
          launch)


def af_step_row(dev, mom_bf16, block_clip):
  """Three leaves, one of each kind, in one table; block_clip > 0 adds the block_usq scratch (nleaves doubles) and the
  launch that fills it (scale_by_adafactor(clipping_threshold=0.7), as test_adafactor_gpu.py)."""
  leaves, soff = _af_leaves([0, 1, 2])
  fl = [lf for lf in leaves if lf["f"]]
  sched = (ctypes.c_float * 2)(*AF_SCHED)

  def launch(ar):
    call("bv_adafactor_step", ar.ptr("params"), ar.ptr("grads"), ar.ptr("momentum"), int(mom_bf16), ar.ptr("shadow"),
         ar.ptr("leaves"), len(leaves), max(lf["R"] for lf in fl), max(lf["C"] for lf in fl), 1, max(lf["n"] for lf in leaves),
         ar.ptr("state"), ar.ptr("gsq"), AF["clip"], AF["decay"], AF["eps"], AF["mom"], ctypes.cast(sched, ctypes.c_void_p), 2,
         ar.ptr("stats"), block_clip, ar.ptr("block_usq") if block_clip > 0 else None, stream())

  _af_run(dev, "bv_adafactor_step", f"three leaves mom {'bf16' if mom_bf16 else 'f32'} block clip {block_clip}", leaves, soff,
          mom_bf16, block_clip, launch)


for _mb in (0, 1):
  _m = "bf16" if _mb else "f32"
  add("bv_adafactor_leaf", f"factored-37x130-mom-{_m}", af_leaf_row, 0, _mb)
  add("bv_adafactor_leaf", f"unfactored-131-mom-{_m}", af_leaf_row, 2, _mb)
  add("bv_adafactor_step", f"three-leaves-one-of-each-kind-mom-{_m}", af_step_row, _mb, 0.0)
  add("bv_adafactor_step", f"three-leaves-block_rms_clip0.7-block_usq-mom-{_m}", af_step_row, _mb, 0.7)


# -------------------------------------------------------------- dropout -----
def _dropout_rows():
  import bv_oracle as O
  key, rate = 0xDEADBEEF12345678, 0.2
  scale = 1.0 / (1.0 - rate)
  for count in (8, 1000):
    keep = torch.from_numpy(np.asarray(O.dropout_keep_mask(key, count, rate)).astype(bool))
    simple("bv_dropout_mask", f"count{count}", lambda c=count: [Op("keep", U8, (c,), "out")],
           lambda ar, c=count: call("bv_dropout_mask", ar.ptr("keep"), c, key, rate, stream()),
           lambda r, keep=keep: _eq(r["keep"].bool(), keep, "keep mask"))
    for addend in (True, False):
      for outs in (("f32", "bf16"), ("f32",), ("bf16",)):
        def make(c=count, addend=addend, outs=outs):
          o = [Op("x", F32, (c,))] + ([Op("addend", F32, (c,))] if addend else [])
          return o + [Op("out_" + t, F32 if t == "f32" else BF16, (c,), "out") for t in outs]

        def launch(ar, c=count, addend=addend, outs=outs):
          call("bv_dropout_f32", ar.ptr("x"), ar.ptr("addend") if addend else None, ar.ptr("out_f32") if "f32" in outs else None,
               ar.ptr("out_bf16") if "bf16" in outs else None, c, key, rate, stream())

        def check(r, keep=keep, addend=addend, outs=outs):
          want = torch.where(keep, r["x"] * scale, torch.zeros_like(r["x"]))
          if addend:
            want = r["addend"] + want
          if "f32" in outs:
            assert torch.allclose(r["out_f32"], want, rtol=1e-6, atol=1e-6)
          if "bf16" in outs and not addend:
            _eq(r["out_bf16"], want.to(BF16), "dropout bf16 output")
          elif "bf16" in outs:
            assert_close(r["out_bf16"], want, 2.0 ** -8, 1e-6, "dropout bf16 output")

        simple("bv_dropout_f32", f"count{count}-{'addend' if addend else 'noaddend'}-{'+'.join(outs)}", make, launch, check)
    for two in (False, True):
      def make2(c=count, two=two):
        return [Op("a", BF16, (c,), "inout", fill=randn((c,), 8))] + ([Op("b", BF16, (c,), "inout", fill=randn((c,), 9))] if two else [])

      def check2(r, keep=keep, two=two):
        for nme in ("a", "b")[:1 + two]:
          _eq(r[nme], torch.where(keep, r.inp[nme].float() * scale, torch.zeros(keep.shape)).to(BF16), "dropout_bf16 " + nme)

      simple("bv_dropout_bf16", f"count{count}-{'two' if two else 'one'}-tensor", make2,
             lambda ar, c=count, two=two: call("bv_dropout_bf16", ar.ptr("a"), ar.ptr("b") if two else None, c, key, rate, stream()), check2)


_dropout_rows()


# ------------------------------------------------------------ the table -----
@pytest.mark.parametrize("fn", [pytest.param(fn, id=f"{e[0]}-{c}") for e, c, fn in ROWS])
def test_footprint(dev, fn):
  fn(dev)
