// Which kernel serves a bv_gemm_bf16[_colsum] call, on what grid and with how many K splits: the ONE place that decides
// it, a pure function of the call's shape / layout / alignment and of the caller's options.  gemm_bf16.hip asks
// gemm_route() once per call and hands the result to one launcher per family (its own 128 x 128 kernel, gemm256.hip's
// 256 x 256 kernels); bv_gemm_workspace_bytes() is the route's slab_bytes of the weight-gradient call;
// tests/test_gemm_route_cpu.py compiles this header into a host program (plain C++, no HIP headers) and holds the tests'
// beliefs about the dispatch to it.
#pragma once
#include "../../include/bvhip.h"

namespace bvgemm {

// GEMM_128: gemm_bf16_kernel (gemm_bf16.hip: any shape the entry point accepts).  GEMM_256: gemm256_kernel, GEMM_256R:
// gemm256r_kernel, the rolling-epilogue kernel (gemm256.hip).
enum GemmFamily { GEMM_128, GEMM_256, GEMM_256R };
// One enumerator per instantiation the library holds, and no others (tests/kernel_coverage.json).
enum GemmKernel {
  G128_A0B0, G128_A0B1, G128_A1B0, G128_A1B1,     // gemm_bf16_kernel<A_KM, B_KM>
  G256_KMINOR,                                    // gemm256_kernel<false>: dW, every epilogue the layout takes
  G256_NONE_BF16, G256_NONE_F32, G256_RESIDUAL_BF16, G256_RESIDUAL_F32, G256_POS, G256_GELU, G256_GELU_BWD,
  G256_GELU_BWD_EMIT, G256_GELU_GD, G256_MUL, G256_GELU_G,   // gemm256_kernel<true, 0, EPI, OUTF32>
  G256R_NONE, G256R_NONE_ST, G256R_RESIDUAL_F32, G256R_GELU, G256R_GELU_ST,   // gemm256r_kernel<EPI, OUTF32[, 1]>
};
// bit i of GemmCall::misaligned: one of the low four address bits of that operand is set (a NULL operand is aligned)
enum GemmOperand { OP_A = 1, OP_B = 2, OP_C = 4, OP_AUX = 8, OP_BIAS = 16, OP_C2 = 32 };

// The call, as bv_gemm_bf16_colsum validated it (M, N, K > 0).
struct GemmCall {
  bool a_kmajor, b_kmajor;
  int M, N, K;
  long lda, ldb, ldc, ldaux;
  unsigned misaligned;
  bool has_aux, has_bias, has_colsum;
  int epilogue;
  bool out_f32, alpha_is_one;
  int split_k;            // 0 = automatic
};
// The caller's context: BV_OPT_FAST_PATH, _GEMM_ROLL, _GEMM_RESERVE_CUS, _GEMM_SKEW_PCT, _GEMM_SKEW_MODE, _GEMM_GROUP_N,
// _GEMM_NT, _GEMM_PRE_ISSUE and its split-K workspace.
struct GemmOpts {
  bool fast_path;
  int roll, reserve, skew_pct, skew_mode, group_n, nt, pre_issue;
  long ws_bytes;
  bool has_ws;
};
constexpr GemmOpts gemm_default_opts() { return GemmOpts{true, 1, 0, 0, 1, 0, 0, 0, 0, false}; }   // include/bvhip.h

struct GemmGrid { unsigned x, y, z; };
struct GemmRoute {
  GemmFamily family;
  GemmKernel kernel;
  int splits;             // split-K factor after rounding: no split is empty
  int ktiles_per_split;   // the 256 families: 64-wide K-tiles per split
  int k_chunk;            // GEMM_128: K elements per split (a multiple of 64)
  GemmGrid grid;
  unsigned block;
  bool use_slab;          // split-K partials go to the workspace and gemm256_reduce_kernel combines them; else fp32 atomics
  long slab_bytes;        // what the slab path takes for this call (0: one split, or not the 256 x 256 dW kernel)
  int skew_cycles, skew_mode, group_n, nt, pre_issue;   // as the 256 x 256 kernels see them
  bool multi, fused;      // BV_STAT_GEMM256_MULTI / _FUSED increment (BV_STAT_GEMM256_CALLS: family != GEMM_128)
};

constexpr int CUS = 256;   // the persistent 256 x 256 grid: one workgroup per CU

// The 256 x 256 x 64 kernels take M, N % 256 == 0, K % 64 == 0, both operands in one layout, 16-byte operand chunks
// (pitches of 8 elements, 16-byte pointers) and the epilogues their layout implements: every one but ATOMIC k-major;
// ATOMIC, and the plain fp32 store without a bias, k-minor.
constexpr bool gemm256_takes(const GemmCall& c) {
  if (c.a_kmajor != c.b_kmajor) return false;
  if ((c.M & 255) || (c.N & 255) || (c.K & 63)) return false;
  if (c.a_kmajor && c.epilogue == BV_EPI_ATOMIC) return false;
  if (!c.a_kmajor && !(c.epilogue == BV_EPI_ATOMIC || (c.epilogue == BV_EPI_NONE && c.out_f32 && !c.has_bias))) return false;
  if ((c.lda & 7) || (c.ldb & 7) || (c.ldc & 7) || (c.misaligned & (OP_A | OP_B | OP_C))) return false;
  if (c.has_aux && ((c.ldaux & 7) || (c.misaligned & OP_AUX))) return false;
  return !(c.misaligned & (OP_BIAS | OP_C2));
}

// Full-epilogue k-major kernel of an epilogue.  POS writes fp32 and the GELU family bf16 whatever out_f32 says (the
// entry point rejects the other value).
constexpr GemmKernel gemm256_full_kernel(int epilogue, bool out_f32) {
  switch (epilogue) {
    case BV_EPI_RESIDUAL: return out_f32 ? G256_RESIDUAL_F32 : G256_RESIDUAL_BF16;
    case BV_EPI_POS: return G256_POS;
    case BV_EPI_GELU: return G256_GELU;
    case BV_EPI_GELU_G: return G256_GELU_G;
    case BV_EPI_GELU_BWD: return G256_GELU_BWD;
    case BV_EPI_GELU_BWD_EMIT: return G256_GELU_BWD_EMIT;
    case BV_EPI_GELU_GD: return G256_GELU_GD;
    case BV_EPI_MUL: return G256_MUL;
    default: return out_f32 ? G256_NONE_F32 : G256_NONE_BF16;
  }
}

// Rolling-epilogue kernel (BV_OPT_GEMM_ROLL: bit 1 = RESIDUAL fp32 with alpha = 1 - the residual is loaded straight into
// the accumulators -, 2 = NONE bf16, 4 = GELU, 8 = their stores inside the MFMA segments): k-major, at least two K-tiles
// per tile, no fused column sums.  Returns false where the full-epilogue kernel runs.
constexpr bool gemm256_rolls(const GemmCall& c, int roll, GemmKernel* k) {
  if (!c.a_kmajor || (c.K >> 6) < 2 || c.has_colsum) return false;
  if ((roll & 1) && c.epilogue == BV_EPI_RESIDUAL && c.out_f32 && c.alpha_is_one) *k = G256R_RESIDUAL_F32;
  else if ((roll & 4) && c.epilogue == BV_EPI_GELU && !c.out_f32) *k = (roll & 8) ? G256R_GELU_ST : G256R_GELU;
  else if ((roll & 2) && c.epilogue == BV_EPI_NONE && !c.out_f32) *k = (roll & 8) ? G256R_NONE_ST : G256R_NONE;
  else return false;
  return true;
}

constexpr GemmRoute gemm_route(const GemmCall& c, const GemmOpts& o) {
  GemmRoute r{};
  if (!o.fast_path || !gemm256_takes(c)) {
    r.family = GEMM_128;
    r.kernel = c.a_kmajor ? (c.b_kmajor ? G128_A1B1 : G128_A1B0) : (c.b_kmajor ? G128_A0B1 : G128_A0B0);
    const int tiles_m = (c.M + 127) / 128, tiles_n = (c.N + 127) / 128, ksteps = (c.K + 63) / 64;
    r.splits = 1;
    if (c.epilogue == BV_EPI_ATOMIC) {
      if (c.split_k > 0) {
        r.splits = c.split_k;
      } else {
        // aim for >= 1024 workgroups (256 CUs x 2 resident x 2 waves of work) while keeping >= 8 K-steps per split
        r.splits = (1024 + tiles_m * tiles_n - 1) / (tiles_m * tiles_n);
        const int max_splits = ksteps / 8 > 0 ? ksteps / 8 : 1;
        if (r.splits > max_splits) r.splits = max_splits;
      }
      if (r.splits < 1) r.splits = 1;
      if (r.splits > ksteps) r.splits = ksteps;
    }
    r.k_chunk = (ksteps + r.splits - 1) / r.splits * 64;
    r.splits = (c.K + r.k_chunk - 1) / r.k_chunk;
    r.grid = GemmGrid{(unsigned)tiles_n, (unsigned)tiles_m, (unsigned)r.splits};
    r.block = 256;
    return r;
  }
  const bool km = c.a_kmajor;
  const int ntiles = (c.M >> 8) * (c.N >> 8), nk = c.K >> 6, cus = CUS - o.reserve;
  r.splits = 1;
  if (c.epilogue == BV_EPI_ATOMIC) {
    // split-K so that tiles x splits ~ one workgroup per CU: the K loop is the whole cost, every extra split adds a
    // 256 KiB partial tile of output traffic
    if (c.split_k > 0) {
      r.splits = c.split_k;   // clamped to nk below, not to nk / 8
    } else {
      r.splits = cus / ntiles;   // work items <= CUs in use (4 reserved CUs keep B/16's choices: 252 = 36 x 7 = 9 x 28)
      const int max_splits = nk / 8 > 0 ? nk / 8 : 1;
      if (r.splits > max_splits) r.splits = max_splits;
    }
    if (r.splits < 1) r.splits = 1;
    if (r.splits > nk) r.splits = nk;
  }
  r.ktiles_per_split = (nk + r.splits - 1) / r.splits;
  r.splits = (nk + r.ktiles_per_split - 1) / r.ktiles_per_split;
  // one 256 x 256 fp32 partial tile per work item; the reduce kernel's float4 accesses of C need ldc % 4 == 0
  r.slab_bytes = c.epilogue == BV_EPI_ATOMIC && r.splits > 1 ? (long)ntiles * r.splits * 65536 * 4 : 0;
  r.use_slab = r.slab_bytes > 0 && o.has_ws && r.slab_bytes <= o.ws_bytes && (c.ldc & 3) == 0;
  const int nwork = ntiles * r.splits;
  r.grid = GemmGrid{(unsigned)(nwork < cus ? nwork : cus), 1, 1};   // persistent: one workgroup per CU
  r.block = 512;
  // start skew (see the kernel): a percentage of one tile period (~3600 cycles per K-tile + epilogue), only where a
  // k-major workgroup walks more than one tile of a full grid
  if (km && o.skew_pct > 0 && nwork > CUS) {
    r.skew_cycles = (int)((long)(nk * 3600 + 12000) * o.skew_pct / 100);
    r.skew_mode = o.skew_mode;
  }
  r.group_n = km ? o.group_n : 0;   // the k-minor kernel has one tile order
  r.nt = o.nt;
  r.pre_issue = o.pre_issue;
  r.multi = nwork > (int)r.grid.x;
  r.fused = r.multi && ((c.epilogue != BV_EPI_NONE && c.epilogue != BV_EPI_ATOMIC) || c.has_colsum);
  r.family = GEMM_256;
  r.kernel = km ? gemm256_full_kernel(c.epilogue, c.out_f32) : G256_KMINOR;
  if (gemm256_rolls(c, o.roll, &r.kernel)) r.family = GEMM_256R;
  return r;
}

}  // namespace bvgemm
