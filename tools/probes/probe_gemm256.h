// The 256x256 kernels as the GEMM probes call them, with the arguments of bv_gemm_bf16_colsum: route the call
// (csrc/gemm_route.h, under the probe context's options - BV_OPT_FAST_PATH included) and launch it if a 256x256 kernel
// takes it; 0 = none does.  Include after gemm256.hip and probe_ctx.h.
#pragma once
static inline int probe_gemm256(int a_kmajor, int b_kmajor, const void* A, long lda, const void* B, long ldb, void* C,
                                long ldc, int out_f32, int M, int N, int K, int epilogue, const float* bias,
                                const void* aux, long ldaux, int aux_rows, void* C2, float alpha, int split_k,
                                float* colsum, void* stream, const bv_ctx* ctx) {
  const bv_gemm_args g{a_kmajor, b_kmajor, A, lda, B, ldb, C, ldc, out_f32, M, N, K, epilogue, bias, aux, ldaux, aux_rows, C2,
                       alpha, split_k, colsum, stream};
  const bv_ctx* const cx = bv_ctx_or_default(ctx);
  const bvgemm::GemmRoute r = bv_gemm_route(g, cx);
  return r.family != bvgemm::GEMM_128 && bv_gemm256_launch(g, r, cx) == BV_OK;
}
