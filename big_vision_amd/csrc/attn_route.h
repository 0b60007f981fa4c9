// Which kernel serves a self-attention call: the ONE place that decides it, a pure function of the shape and the
// caller's BV_OPT_ATTN_CFG bits.  attention3.hip / attention5.hip instantiate their kernels from the constexpr tables
// below and launch what attn_route() names; ops.py states attn_route_is_adh() for its choice of entry point;
// tests/test_attn_route_cpu.py compiles this header into a host program (plain C++, no HIP headers) and holds the
// tests' mirrors (_bounds.py::attn_bwd_path, the tables of test_kernel_buckets_gpu.py) to it.
#pragma once

// Compile-time A/B of the 28-fragment kernels' workgroup sizes (tools/attn_fwd_long_ab.py builds the other values).
#ifndef A3_FWD_LONG_NW
#define A3_FWD_LONG_NW 8   // waves of the 28-fragment forward's workgroup: 8 (2 per SIMD, K-row prefetch) or 12 (3 per SIMD, plain loops,
#endif                     // 166 VGPRs): 12 is bit-identical and 2 % faster (433 vs 442 us, r06_attn_long_prefetch_ab.txt) - inside the spread, off
#ifndef A3_DQ_LONG_NW
#define A3_DQ_LONG_NW 16   // waves of the UNMASKED 28-fragment one-sweep dQ kernel: 16 (4 per SIMD: its 126 VGPRs fit the 128 line) ships since
#endif                     // round 6 - bit-identical, backward at L = 441 1424-1430 -> 1384-1400 us (same file); 8 = the former 2 per SIMD

namespace bvattn {

// ATTN_ADH: attention_dh.hip (any head dim and length; its own (Dh + 15) / 16 dispatch).  ATTN_3: attention3.hip (Dh = 64,
// L <= 576: forward, and the backward as dQ + dK/dV launches).  ATTN_5: attention5.hip, that backward in one launch.
enum AttnFamily { ATTN_ADH, ATTN_3, ATTN_5 };
// attn3_bwd_dkv_kernel<KF, NW, WPS> (16-key fragments) / attn4_bwd_dkv_kernel<KF, 7> / <KF, 4> (32-key blocks; 7 waves x 1
// workgroup per CU, 4 waves x 2)
enum AttnDkv { DKV_16, DKV_32X7, DKV_32X4 };
struct AttnGeom { int NW, WPS; };   // waves per workgroup, waves per SIMD (the kernels' launch bound)

struct AttnRoute {
  AttnFamily family;   // of the backward; the forward of an ATTN_5 shape is ATTN_3's
  int KF;              // key fragments of the instantiation; forward and backward share it (the lse layout depends on it)
  AttnGeom fwd;        // attn3_fwd_kernel<KF, NW, WPS, TAIL>
  bool fwd8;           // fwd = attn3_fwd_geom(KF, true): the A/B geometry of the 13-fragment forward
  bool tail;           // TAIL of the forward and of the one-sweep dQ kernel: only the last key fragment is masked
  bool dq1;            // attn3_bwd_dq1_kernel<KF, NW, WPS, TAIL> (one sweep, reads O), else attn3_bwd_dq_kernel<KF, NW, WPS>
  AttnGeom dq, dkv;    // dkv: of DKV_16
  AttnDkv dkv_kind;
  int LW;              // attn5_bwd_kernel<KF, LW, BM>: loader waves (BM depends on the dbias pointer: launch_bwd5)
  bool bias_dpp;       // ATTN_5: DPP column sums of the bias gradients where the identities apply (A/B)
};

constexpr bool attn_route_is_adh(int L, int Dh) { return Dh != 64 || L > 576; }
// Key fragments = ceil(L / 16) for the common lengths (64 text tokens; 196 / 197 at 224 px; 256 / 257; 441 at 336 px;
// 576 at 384 px), the next instantiated size otherwise.
constexpr int attn3_kf(int L) { return L <= 64 ? 4 : L <= 208 ? 13 : L <= 272 ? 17 : L <= 448 ? 28 : 36; }
// Forward.  13 key fragments: 4 waves per workgroup and 3 workgroups per CU (the third one computes while another
// stages its K/V: 605-650 us instead of 670-730 at n = 2048); fwd8 (BV_OPT_ATTN_CFG = 8): 8 waves x 2 workgroups.
constexpr AttnGeom attn3_fwd_geom(int KF, bool fwd8) {
  return KF == 4 ? AttnGeom{4, 4} : KF == 13 ? (fwd8 ? AttnGeom{8, 4} : AttnGeom{4, 3}) : KF == 17 ? AttnGeom{8, 4}
       : KF == 28 ? AttnGeom{A3_FWD_LONG_NW, A3_FWD_LONG_NW == 12 ? 3 : 2} : AttnGeom{8, 2};
}
// Two-launch backward: the dK/dV kernel, the two-sweep dQ kernel and the one-sweep dQ kernel without TAIL ...
constexpr AttnGeom attn3_bwd_geom(int KF) { return KF == 4 ? AttnGeom{4, 4} : KF <= 17 ? AttnGeom{8, 4} : AttnGeom{8, 2}; }
// ... and the one-sweep dQ kernel with TAIL (see A3_DQ_LONG_NW)
constexpr AttnGeom attn3_dq1_tail_geom(int KF) {
  return KF == 28 && A3_DQ_LONG_NW == 16 ? AttnGeom{16, 4} : attn3_bwd_geom(KF);
}
// 32-key-block dK/dV kernels exist from 13 key fragments: the 4-fragment sequences always take the 16-key kernel
constexpr bool attn4_dkv_exists(int KF) { return KF >= 13; }
// One-launch backward: KF key-owning + LW loader waves (13 + 3 fill the four SIMDs' wave slots at <= 128 VGPRs); 0 = the
// length is not covered
constexpr int attn5_lw(int L) { return L <= 64 ? 1 : L > 192 && L <= 208 ? 3 : 0; }

// masked: the call carries key-padding lengths.  cfg: BV_OPT_ATTN_CFG (include/bvhip.h).  has_o: the backward was
// given the forward's output (the masked entry point has none).
constexpr AttnRoute attn_route(int L, int Dh, bool masked, long cfg, bool has_o) {
  AttnRoute r{};
  r.family = ATTN_ADH;
  if (attn_route_is_adh(L, Dh)) return r;
  r.KF = attn3_kf(L);
  r.tail = !masked && L > (r.KF - 1) * 16;   // no kv_len and L in the last fragment: Lk > (KF - 1) * 16 for every sample
  r.fwd8 = r.KF == 13 && (cfg & 15) == 8;    // bit 8: forward of the 13-fragment kernels as 8 waves x 2 workgroups
  r.fwd = attn3_fwd_geom(r.KF, r.fwd8);
  r.bias_dpp = (cfg & 256) != 0;             // bit 256
  r.LW = attn5_lw(L);
  r.family = !masked && !(cfg & 128) && r.LW ? ATTN_5 : ATTN_3;   // bit 128: two launches also where one applies
  if (r.family == ATTN_5) return r;
  r.dq1 = has_o && !(cfg & 16);              // bit 16: always the two-sweep dQ kernel
  r.dq = r.dq1 && r.tail ? attn3_dq1_tail_geom(r.KF) : attn3_bwd_geom(r.KF);
  r.dkv = attn3_bwd_geom(r.KF);
  // Bits 32 / 64 ask for the 32-key-block dK/dV kernel (4 waves x 2 / 7 waves x 1).  Long sequences (28+ key fragments:
  // L/16 at 336 px = 441 tokens, 576 at 384 px), unmasked: the 7-wave one is the default since round 6 - bit-identical
  // results, whole backward 1360 -> 1249 us at n = 256, L = 441, H = 16 and 716 -> 686 us at L = 576
  // (tools/attn_longseq_cfg_ab.py, profiles/r06_attn_longseq_cfg_ab.txt); at 13-17 fragments it loses (L = 256: 366 ->
  // 461 us) and stays opt-in; bit 1024 keeps the 16-key kernel for the long sequences too
  const bool x7 = (cfg & 64) || (!(cfg & 32) && r.KF >= 28 && !masked && !(cfg & 1024));
  r.dkv_kind = !attn4_dkv_exists(r.KF) || !(x7 || (cfg & 32)) ? DKV_16 : x7 ? DKV_32X7 : DKV_32X4;
  return r;
}

}  // namespace bvattn
