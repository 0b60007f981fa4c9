// libbveval: one batch of the classification evaluator (evaluators/classification.py:37-53 with the losses of
// utils.py:236-243 and :276-281) in ONE pass over the logit and label matrices, for gfx950.  Plain HIP C++, fp32
// arithmetic per row, fp64 sums over rows, one launch per call.  This translation unit is the whole library
// (include/bveval.h): it carries its own last-error string and links nothing of libbvhip or libbvdistill.
//
// One read of every element for any C.  A lane streams its columns in increasing order and keeps eight words:
//   m, z     running maximum of its logits and sum of exp(l - m), rescaled by exp(m_old - m_new) whenever m moves
//            (online log-sum-exp; softmax only)
//   syl, sy  sum y l and sum y (softmax), or the running sum of the sigmoid terms
//   my       max y
//   bv, bi, by   the best logit so far, its column and the label there (`beats` below is jnp.argmax's order)
// Nothing of the row is kept, so there is no register-resident row, no second pass and no limit on C.  The lanes of
// a row are merged with the same recurrences: 6 xor-shuffle levels inside a wave and, for a workgroup-wide row, the
// four wave results through 128 bytes of LDS.
//
// Row mapping: C <= 1024 takes a wave per row (four rows per workgroup: a 10- or 1000-class row has at most 4 KB, and
// a wave covers it with at most four 16-byte loads per lane and operand); longer rows take a workgroup per row.  The
// switch-over is a choice by reasoning (the longest row a lane covers in four vector loads), not a tuned threshold;
// what either side reaches is in profiles/eval_yardstick.jsonl.  The grid is capped at 2048 workgroups that stride
// over the rows; every workgroup sums its rows' three contributions in fp64 registers and issues three atomic adds.
#include <float.h>
#include <limits.h>

#define BV_STATUS_LINKAGE static   // the whole library is this file
#include "bv_common.h"
#include "../../include/bveval.h"

BV_DEFINE_STATUS(bv_eval_last_error, bv_eval_version, BVEVAL_VERSION)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGrid = 2048;

struct RowState {
  float m, z, syl, sy, my, bv, by;
  int bi;
};

// m starts at -FLT_MAX, not -inf: exp(m_old - m_new) is then never exp(-inf + inf), also for a row of -inf logits
__device__ __forceinline__ RowState row_init() { return RowState{-FLT_MAX, 0.f, 0.f, 0.f, -INFINITY, -INFINITY, 0.f, INT_MAX}; }

// jnp.argmax's order: (xv, xi) precedes (bv, bi).  A NaN is the maximum; among equals the lower index wins.  The
// start value (-inf, INT_MAX) loses against every element, so a row of -inf logits answers column 0.
__device__ __forceinline__ bool beats(float xv, int xi, float bv, int bi) {
  const bool xn = xv != xv, bn = bv != bv;
  return xn ? (!bn || xi < bi) : (!bn && (xv > bv || (xv == bv && xi < bi)));
}

// everything of one element but its exponential
template <int KIND>
__device__ __forceinline__ void take_rest(RowState& s, float x, float y, int c) {
  if (KIND == BVE_LOSS_SOFTMAX_XENT) {
    s.syl = fmaf(y, x, s.syl);
    s.sy += y;
  } else {
    const float t = log1pf(__expf(-fabsf(x)));
    const float lp = fminf(x, 0.f) - t, ln = fminf(-x, 0.f) - t;   // log_sigmoid(x), log_sigmoid(-x)
    s.syl += fmaf(1.f - y, ln, y * lp);
  }
  s.my = fmaxf(s.my, y);
  if (beats(x, c, s.bv, s.bi)) { s.bv = x; s.bi = c; s.by = y; }
}

template <int KIND>
__device__ __forceinline__ void take(RowState& s, float x, float y, int c) {
  if (KIND == BVE_LOSS_SOFTMAX_XENT) {
    const float nm = fmaxf(s.m, x);
    s.z = s.z * __expf(s.m - nm) + __expf(x - nm);     // a NaN logit is skipped by fmaxf and poisons z through x - nm
    s.m = nm;
  }
  take_rest<KIND>(s, x, y, c);
}

// four elements at columns c, c + step, c + 2 step, c + 3 step: one rescale of z for the four
template <int KIND>
__device__ __forceinline__ void take4(RowState& s, f32x4 x, f32x4 y, int c, int step) {
  if (KIND == BVE_LOSS_SOFTMAX_XENT) {
    const float nm = fmaxf(s.m, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    const float e = (__expf(x[0] - nm) + __expf(x[1] - nm)) + (__expf(x[2] - nm) + __expf(x[3] - nm));
    s.z = s.z * __expf(s.m - nm) + e;
    s.m = nm;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) take_rest<KIND>(s, x[k], y[k], c + k * step);
}

template <int KIND>
__device__ __forceinline__ RowState merge(RowState a, const RowState& b) {
  if (KIND == BVE_LOSS_SOFTMAX_XENT) {
    const float nm = fmaxf(a.m, b.m);
    a.z = a.z * __expf(a.m - nm) + b.z * __expf(b.m - nm);
    a.m = nm;
    a.sy += b.sy;
  }
  a.syl += b.syl;
  a.my = fmaxf(a.my, b.my);
  if (beats(b.bv, b.bi, a.bv, a.bi)) { a.bv = b.bv; a.bi = b.bi; a.by = b.by; }
  return a;
}

template <int KIND>
__device__ __forceinline__ RowState wave_merge(RowState s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowState t;
    t.m = __shfl_xor(s.m, o, 64); t.z = __shfl_xor(s.z, o, 64); t.syl = __shfl_xor(s.syl, o, 64);
    t.sy = __shfl_xor(s.sy, o, 64); t.my = __shfl_xor(s.my, o, 64); t.bv = __shfl_xor(s.bv, o, 64);
    t.by = __shfl_xor(s.by, o, 64); t.bi = __shfl_xor(s.bi, o, 64);
    s = merge<KIND>(s, t);
  }
  return s;
}

struct EvalArgs {
  const float* logits;
  const float* labels;
  const float* mask;
  double* acc;
  float* row_loss;
  int* row_top1;
  int n, C;
};

// VEC: 16-byte loads (C % 4 == 0, both matrices 16-byte aligned: every row then is).  WG: a workgroup per row.
template <int KIND, int VEC, int WG>
__global__ __launch_bounds__(kThreads) void eval_classify_kernel(EvalArgs p) {
  constexpr int L = WG ? kThreads : 64;                  // lanes that share a row
  __shared__ RowState sh[kWaves];
  __shared__ double shd[kWaves][3];
  const int C = p.C;
  const int lane = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const int wave = threadIdx.x >> 6;
  const long first = WG ? (long)blockIdx.x : (long)blockIdx.x * kWaves + wave;
  const long stride = WG ? (long)gridDim.x : (long)gridDim.x * kWaves;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;                   // this workgroup's (WG) / wave's share of acc
  for (long row = first; row < p.n; row += stride) {
    const float* __restrict__ xr = p.logits + row * C;
    const float* __restrict__ yr = p.labels + row * C;
    RowState s = row_init();
    if (VEC) {
#pragma unroll 2
      for (long c = 4L * lane; c < C; c += 4L * L)      // C % 4 == 0: a vector that starts below C ends below C
        take4<KIND>(s, *reinterpret_cast<const f32x4*>(xr + c), *reinterpret_cast<const f32x4*>(yr + c), (int)c, 1);
    } else {
      long c = lane;
#pragma unroll 2
      for (; c + 3L * L < C; c += 4L * L) {
        const f32x4 x = {xr[c], xr[c + L], xr[c + 2 * L], xr[c + 3 * L]};
        const f32x4 y = {yr[c], yr[c + L], yr[c + 2 * L], yr[c + 3 * L]};
        take4<KIND>(s, x, y, (int)c, L);
      }
      for (; c < C; c += L) take<KIND>(s, xr[c], yr[c], (int)c);
    }
    s = wave_merge<KIND>(s);
    bool owner = lane == 0;
    if (WG) {
      __syncthreads();                                   // the previous row's readers are done with sh
      if ((threadIdx.x & 63) == 0) sh[wave] = s;
      __syncthreads();
      if (owner) s = merge<KIND>(merge<KIND>(sh[0], sh[1]), merge<KIND>(sh[2], sh[3]));
    }
    if (owner) {
      const float loss = KIND == BVE_LOSS_SOFTMAX_XENT ? s.sy * (s.m + logf(s.z)) - s.syl : -s.syl;
      const double mi = (double)(p.mask ? p.mask[row] : 1.f) * (double)s.my;
      if (p.row_loss) p.row_loss[row] = loss;
      if (p.row_top1) p.row_top1[row] = s.bi;
      a0 += (double)s.by * mi;
      a1 += (double)loss * mi;
      a2 += mi;
    }
  }
  if (!p.acc) return;
  if (!WG) {
    if (lane == 0) { shd[wave][0] = a0; shd[wave][1] = a1; shd[wave][2] = a2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      a0 = (shd[0][0] + shd[1][0]) + (shd[2][0] + shd[3][0]);
      a1 = (shd[0][1] + shd[1][1]) + (shd[2][1] + shd[3][1]);
      a2 = (shd[0][2] + shd[1][2]) + (shd[2][2] + shd[3][2]);
    }
  }
  if (threadIdx.x == 0) {
    atomicAdd(p.acc + 0, a0);
    atomicAdd(p.acc + 1, a1);
    atomicAdd(p.acc + 2, a2);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int KIND>
void launch(bool vec, bool wg, const EvalArgs& a, hipStream_t s) {
  const long groups = wg ? (long)a.n : ((long)a.n + kWaves - 1) / kWaves;
  const dim3 grid((unsigned)(groups < kMaxGrid ? groups : kMaxGrid)), block(kThreads);
  if (vec && wg) hipLaunchKernelGGL((eval_classify_kernel<KIND, 1, 1>), grid, block, 0, s, a);
  else if (vec) hipLaunchKernelGGL((eval_classify_kernel<KIND, 1, 0>), grid, block, 0, s, a);
  else if (wg) hipLaunchKernelGGL((eval_classify_kernel<KIND, 0, 1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((eval_classify_kernel<KIND, 0, 0>), grid, block, 0, s, a);
}

}  // namespace

extern "C" int bv_eval_classify(int loss_kind, const float* logits, const float* labels, const float* mask, double* acc,
                                float* row_loss, int* row_top1, int n, int C, void* stream) {
  BV_REQUIRE(n > 0 && C > 0, "bv_eval_classify: bad shape n=%d C=%d", n, C);
  BV_REQUIRE(loss_kind >= 0 && loss_kind < BVE_LOSS_COUNT, "bv_eval_classify: unknown loss kind %d", loss_kind);
  BV_REQUIRE(logits && labels, "bv_eval_classify: NULL logits or labels");
  BV_REQUIRE(acc || row_loss || row_top1, "bv_eval_classify: acc, row_loss and row_top1 are all NULL (nothing to compute)");
  const EvalArgs a{logits, labels, mask, acc, row_loss, row_top1, n, C};
  const bool vec = C % 4 == 0 && aligned16(logits) && aligned16(labels);
  const bool wg = C > BVE_WAVE_ROW_MAX_C;
  if (loss_kind == BVE_LOSS_SOFTMAX_XENT) launch<BVE_LOSS_SOFTMAX_XENT>(vec, wg, a, (hipStream_t)stream);
  else launch<BVE_LOSS_SIGMOID_XENT>(vec, wg, a, (hipStream_t)stream);
  return bv_check_launch("bv_eval_classify");
}
