// What gemm_bf16.hip (the entry point and the 128 x 128 launcher) and gemm256.hip (the 256 x 256 launcher) share on the
// host: the arguments of one call, the route gemm_route.h gives it under a context, and the operand fields of the two
// kernel parameter structs.
#pragma once
#include "bvhip_internal.h"
#include "gemm_route.h"
#include <cstdint>

// The arguments of one bv_gemm_bf16_colsum call (include/bvhip.h), as the entry point received them.
struct bv_gemm_args {
  int a_kmajor, b_kmajor;
  const void* A; long lda;
  const void* B; long ldb;
  void* C; long ldc;
  int out_f32, M, N, K, epilogue;
  const float* bias;
  const void* aux; long ldaux; int aux_rows;
  void* C2;
  float alpha;
  int split_k;
  float* colsum;
  void* stream;
};
// What gemm_route.h decides for a call under a context's options and workspace (ctx: not NULL - bv_ctx_or_default).
inline bvgemm::GemmRoute bv_gemm_route(const bv_gemm_args& g, const bv_ctx* ctx) {
  using namespace bvgemm;
  const auto low4 = [](const void* p, unsigned bit) { return (uintptr_t)p & 15 ? bit : 0u; };
  bvgemm::GemmCall c{};
  c.a_kmajor = g.a_kmajor != 0; c.b_kmajor = g.b_kmajor != 0;
  c.M = g.M; c.N = g.N; c.K = g.K;
  c.lda = g.lda; c.ldb = g.ldb; c.ldc = g.ldc; c.ldaux = g.ldaux;
  c.misaligned = low4(g.A, OP_A) | low4(g.B, OP_B) | low4(g.C, OP_C) | low4(g.aux, OP_AUX) | low4(g.bias, OP_BIAS) | low4(g.C2, OP_C2);
  c.has_aux = g.aux != nullptr; c.has_bias = g.bias != nullptr; c.has_colsum = g.colsum != nullptr;
  c.epilogue = g.epilogue; c.out_f32 = g.out_f32 != 0; c.alpha_is_one = g.alpha == 1.0f; c.split_k = g.split_k;
  bvgemm::GemmOpts o{};
  o.fast_path = ctx->opt[BV_OPT_FAST_PATH] != 0;
  o.roll = (int)ctx->opt[BV_OPT_GEMM_ROLL]; o.reserve = (int)ctx->opt[BV_OPT_GEMM_RESERVE_CUS];
  o.skew_pct = (int)ctx->opt[BV_OPT_GEMM_SKEW_PCT]; o.skew_mode = (int)ctx->opt[BV_OPT_GEMM_SKEW_MODE];
  o.group_n = (int)ctx->opt[BV_OPT_GEMM_GROUP_N]; o.nt = (int)ctx->opt[BV_OPT_GEMM_NT];
  o.pre_issue = (int)ctx->opt[BV_OPT_GEMM_PRE_ISSUE];
  o.ws_bytes = ctx->ws_bytes; o.has_ws = ctx->ws != nullptr;
  return bvgemm::gemm_route(c, o);
}
// The operand fields G256Params (gemm256.hip) and GemmParams (gemm_bf16.hip) share
template <class P>
inline void bv_gemm_fill(P& p, const bv_gemm_args& g) {
  p.A = (decltype(p.A))g.A; p.B = (decltype(p.B))g.B; p.C = g.C; p.C2 = g.C2;
  p.bias = g.bias; p.aux = g.aux; p.colsum = g.colsum;
  p.lda = g.lda; p.ldb = g.ldb; p.ldc = g.ldc; p.ldaux = g.ldaux;
  p.M = g.M; p.N = g.N; p.K = g.K; p.aux_rows = g.aux_rows > 0 ? g.aux_rows : 1;
  p.epi = g.epilogue; p.out_f32 = g.out_f32; p.alpha = g.alpha;
}
// gemm256.hip: launches a route of the families GEMM_256 / GEMM_256R (the kernel route.kernel names, then the split-K
// combine where route.use_slab) and counts it in the context's BV_STAT_GEMM256_* (ctx: not NULL).  BV_ERR_INVALID_ARG,
// and nothing launched or counted, for a route that names no 256 x 256 kernel.
int bv_gemm256_launch(const bv_gemm_args& g, const bvgemm::GemmRoute& route, const bv_ctx* ctx);
