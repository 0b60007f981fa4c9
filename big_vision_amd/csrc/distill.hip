// libbvdistill: the distillation distances of evaluators/proj/distill/distance.py:35-67 with their derivatives, the
// entropy measurement and the teacher-ensemble softmax of trainers/proj/distill/distill.py, for gfx950.  Plain HIP
// C++, fp32 arithmetic, one launch per call.  This translation unit is the whole library (include/bvdistill.h): it
// carries its own last-error string and links nothing of libbvhip.
//
// Work decomposition: ONE 256-LANE WORKGROUP PER ROW, not one wave per row.  This is a choice by reasoning; no
// wave-per-row variant was built or timed against it.  The rows of a distillation step are the per-device batch
// (512 .. 4096) and a row is a class vector (C = 1000: 4 KB).  With a wave per row, 512 rows are 512 waves for the
// 1024 SIMDs of the chip and each row's loads are issued by a single wave.  A workgroup per row puts 4 waves on every
// row (2048 waves at n = 512), each lane issues one or two 16-byte loads per operand and the whole row is in flight
// at once; the price is a cross-wave reduction through 16 bytes of LDS per phase.  What the chosen kernel reaches is
// in profiles/distill_yardstick.md: 867 GB/s of algorithmic traffic at n = 4096, C = 1000 - well below HBM rate, so
// the dependent reductions, not the traffic, bound it today.
//
// Traffic contract: for C <= 4096 a lane keeps its <= 16 student and <= 16 teacher logits in registers from the one
// load to the last phase (max, sum of exponentials, value, gradient), so each logit is read from HBM once and each
// output element is written once.  The register arrays are only ever indexed by the induction variables of fully
// unrolled loops (compile-time constants): a run-time index would move them to scratch.  C > 4096 re-reads the row in
// every phase (MODE_STREAM) with the same arithmetic per element, always with 4-byte accesses (an untuned fallback).
#define BV_STATUS_LINKAGE static   // the whole library is this file
#include "bv_common.h"
#include "../../include/bvdistill.h"

BV_DEFINE_STATUS(bv_distill_last_error, bv_distill_version, BVDISTILL_VERSION)

namespace {

constexpr int kThreads = 256;
constexpr int kSlots = 16;                    // logits of one operand a lane holds: rows up to 16 * 256 = 4096
constexpr int kCachedMaxC = kSlots * kThreads;
constexpr float kLogClip = -18.420680743952367f;   // log(1e-8): log(max(y, 1e-8)) = max(log y, log 1e-8)

// how a lane walks its row: 16-byte loads of 4 consecutive columns, scalar loads 256 columns apart, or no cache
enum { MODE_VEC = 0, MODE_SCALAR = 1, MODE_STREAM = 2 };

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
// block reductions over the 4 waves; sh: 4 words of LDS shared by all of them (hence the leading barrier)
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ int block_sum_i(int v, float* sh) {
  int* si = reinterpret_cast<int*>(sh);
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = v;
  __syncthreads();
  return si[0] + si[1] + si[2] + si[3];
}
__device__ __forceinline__ int block_min_i(int v, float* sh) {
  int* si = reinterpret_cast<int*>(sh);
  v = wave_min_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = v;
  __syncthreads();
  return min(min(si[0], si[1]), min(si[2], si[3]));
}

// column of slot i of this lane
template <int MODE>
__device__ __forceinline__ int slot_col(int i) {
  return MODE == MODE_VEC ? (((i >> 2) * kThreads + (int)threadIdx.x) * 4 + (i & 3)) : (i * kThreads + (int)threadIdx.x);
}

// the one read of a row (MODE_STREAM: nothing is cached).  MODE_VEC requires C % 4 == 0 and a 16-byte aligned row:
// a vector that starts below C ends below C.
template <int MODE>
__device__ __forceinline__ void load_row(float (&v)[kSlots], const float* __restrict__ row, int C) {
  if (MODE == MODE_VEC) {
#pragma unroll
    for (int j = 0; j < kSlots / 4; ++j) {
      const int c = (j * kThreads + (int)threadIdx.x) * 4;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (c < C) x = *reinterpret_cast<const f32x4*>(row + c);
      v[4 * j + 0] = x[0]; v[4 * j + 1] = x[1]; v[4 * j + 2] = x[2]; v[4 * j + 3] = x[3];
    }
  } else if (MODE == MODE_SCALAR) {
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
      const int c = i * kThreads + (int)threadIdx.x;
      v[i] = c < C ? row[c] : 0.f;
    }
  }
}

// f(c, a_c, b_c) for every column c of this lane (rb may be NULL in MODE_STREAM: b_c = 0)
template <int MODE, class F>
__device__ __forceinline__ void each(const float (&a)[kSlots], const float (&b)[kSlots], const float* __restrict__ ra,
                                     const float* __restrict__ rb, int C, F f) {
  if (MODE == MODE_STREAM) {
    for (int c = threadIdx.x; c < C; c += kThreads) f(c, ra[c], rb ? rb[c] : 0.f);
  } else {
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
      const int c = slot_col<MODE>(i);
      if (c < C) f(c, a[i], b[i]);
    }
  }
}

// out[c] (+)= g(c, a_c, b_c) for every column of this lane; each element is stored once
template <int MODE, class G>
__device__ __forceinline__ void emit(float* __restrict__ out, int accumulate, const float (&a)[kSlots],
                                     const float (&b)[kSlots], const float* __restrict__ ra,
                                     const float* __restrict__ rb, int C, G g) {
  if (MODE == MODE_VEC) {
#pragma unroll
    for (int j = 0; j < kSlots / 4; ++j) {
      const int c = (j * kThreads + (int)threadIdx.x) * 4;
      if (c < C) {
        f32x4 o;
        o[0] = g(c + 0, a[4 * j + 0], b[4 * j + 0]);
        o[1] = g(c + 1, a[4 * j + 1], b[4 * j + 1]);
        o[2] = g(c + 2, a[4 * j + 2], b[4 * j + 2]);
        o[3] = g(c + 3, a[4 * j + 3], b[4 * j + 3]);
        f32x4* dst = reinterpret_cast<f32x4*>(out + c);
        if (accumulate) o += *dst;
        *dst = o;
      }
    }
  } else {
    each<MODE>(a, b, ra, rb, C, [&](int c, float x, float y) {
      const float o = g(c, x, y);
      out[c] = accumulate ? out[c] + o : o;
    });
  }
}

// max and sum of exp((x - max) inv_t) of one cached / streamed row
template <int MODE>
__device__ __forceinline__ void row_max_sumexp(const float (&v)[kSlots], const float* __restrict__ row, int C,
                                               float inv_t, float* sh, float& mx, float& z) {
  float m = -INFINITY;
  each<MODE>(v, v, row, nullptr, C, [&](int, float x, float) { m = fmaxf(m, x); });
  mx = block_max(m, sh);
  const float mm = mx;
  float acc = 0.f;
  each<MODE>(v, v, row, nullptr, C, [&](int, float x, float) { acc += __expf((x - mm) * inv_t); });
  z = block_sum(acc, sh);
}

// first index of the row's maximum (ties to the lower index, jnp.argmax / lax.top_k)
template <int MODE>
__device__ __forceinline__ int row_first_argmax(const float (&v)[kSlots], const float* __restrict__ row, int C,
                                                float mx, float* sh) {
  int a = 0x7fffffff;
  each<MODE>(v, v, row, nullptr, C, [&](int c, float x, float) { if (x == mx) a = min(a, c); });
  return block_min_i(a, sh);
}

struct DistArgs {
  const float* student;
  const float* teacher;
  float* per_row;
  double* loss_sum;
  float* dstudent;
  int accumulate, C, k, n_global;
  float inv_n, t, ls, eps;
};

template <int KIND, int MODE>
__global__ __launch_bounds__(kThreads) void distill_dist_kernel(DistArgs p) {
  __shared__ float sh[4];
  const int C = p.C;
  const long base = (long)blockIdx.x * C;
  const float* __restrict__ sr = p.student + base;
  const float* __restrict__ tr = p.teacher + base;
  float* __restrict__ gr = p.dstudent ? p.dstudent + base : nullptr;
  float s[kSlots], T[kSlots];
  load_row<MODE>(s, sr, C);
  load_row<MODE>(T, tr, C);
  const float inv_n = p.inv_n;
  float value = 0.f;

  if (KIND == BVD_KIND_L2 || KIND == BVD_KIND_EUCLIDEAN) {
    float acc = 0.f;
    each<MODE>(s, T, sr, tr, C, [&](int, float a, float b) { const float d = a - b; acc = fmaf(d, d, acc); });
    const float ss = block_sum(acc, sh);
    value = KIND == BVD_KIND_L2 ? ss : sqrtf(ss + p.eps);
    if (gr) {
      const float scale = KIND == BVD_KIND_L2 ? 2.f * inv_n : inv_n / value;
      emit<MODE>(gr, p.accumulate, s, T, sr, tr, C, [&](int, float a, float b) { return (a - b) * scale; });
    }
  } else if (KIND == BVD_KIND_KL || KIND == BVD_KIND_HARD) {
    const float t = KIND == BVD_KIND_KL ? p.t : 1.f;
    const float inv_t = 1.f / t;
    float ms, zs, mt, zt = 1.f;
    row_max_sumexp<MODE>(s, sr, C, inv_t, sh, ms, zs);
    const float lzs = logf(zs), inv_zs = 1.f / zs;
    // the labels y_c and the clipped log(max(y_c, 1e-8)) of either kind
    float lzt = 0.f, inv_zt = 1.f, on = 1.f, off = 0.f, lon = 0.f, loff = 0.f;
    int a = 0;
    if (KIND == BVD_KIND_KL) {
      row_max_sumexp<MODE>(T, tr, C, inv_t, sh, mt, zt);
      lzt = logf(zt); inv_zt = 1.f / zt;
    } else {
      float m = -INFINITY;
      each<MODE>(T, T, tr, nullptr, C, [&](int, float x, float) { m = fmaxf(m, x); });
      mt = block_max(m, sh);
      a = row_first_argmax<MODE>(T, tr, C, mt, sh);
      on = 1.f - p.ls;
      off = C > 1 ? p.ls / (float)(C - 1) : 0.f;
      lon = logf(fmaxf(on, 1e-8f));
      loff = logf(fmaxf(off, 1e-8f));
    }
    float acc = 0.f;
    each<MODE>(s, T, sr, tr, C, [&](int c, float x, float w) {
      const float lp = (x - ms) * inv_t - lzs;          // log_softmax(s / t)_c
      float y, ly;
      if (KIND == BVD_KIND_KL) {
        const float u = (w - mt) * inv_t;
        y = __expf(u) * inv_zt;
        ly = fmaxf(u - lzt, kLogClip);
      } else {
        y = c == a ? on : off;
        ly = c == a ? lon : loff;
      }
      acc = fmaf(y, ly - lp, acc);
    });
    value = t * t * block_sum(acc, sh);
    if (gr) {
      const float scale = t * inv_n;
      emit<MODE>(gr, p.accumulate, s, T, sr, tr, C, [&](int c, float x, float w) {
        const float ps = __expf((x - ms) * inv_t) * inv_zs;
        const float y = KIND == BVD_KIND_KL ? __expf((w - mt) * inv_t) * inv_zt : (c == a ? on : off);
        return (ps - y) * scale;
      });
    }
  } else if (KIND == BVD_KIND_LOGSOFTMAX_EUCLIDEAN) {
    float ms, zs, mt, zt;
    row_max_sumexp<MODE>(s, sr, C, 1.f, sh, ms, zs);
    row_max_sumexp<MODE>(T, tr, C, 1.f, sh, mt, zt);
    const float lzs = logf(zs), lzt = logf(zt), inv_zs = 1.f / zs;
    float acc = 0.f, acc1 = 0.f;
    each<MODE>(s, T, sr, tr, C, [&](int, float x, float w) {
      const float e = ((x - ms) - lzs) - ((w - mt) - lzt);
      acc = fmaf(e, e, acc);
      acc1 += e;
    });
    const float ss = block_sum(acc, sh);
    const float se = block_sum(acc1, sh);
    value = sqrtf(ss + p.eps);
    if (gr) {
      const float scale = inv_n / value;
      emit<MODE>(gr, p.accumulate, s, T, sr, tr, C, [&](int, float x, float w) {
        const float e = ((x - ms) - lzs) - ((w - mt) - lzt);
        const float ps = __expf(x - ms) * inv_zs;
        return (e - ps * se) * scale;
      });
    }
  } else {   // BVD_KIND_AGREE
    float m = -INFINITY;
    each<MODE>(T, T, tr, nullptr, C, [&](int, float x, float) { m = fmaxf(m, x); });
    const float mt = block_max(m, sh);
    const int a = row_first_argmax<MODE>(T, tr, C, mt, sh);
    float sa = -INFINITY;
    each<MODE>(s, s, sr, nullptr, C, [&](int c, float x, float) { if (c == a) sa = x; });
    sa = block_max(sa, sh);
    int ahead = 0;
    each<MODE>(s, s, sr, nullptr, C, [&](int c, float x, float) { ahead += (x > sa) || (x == sa && c < a); });
    ahead = block_sum_i(ahead, sh);
    value = ahead < p.k ? 1.f : 0.f;
  }

  if (threadIdx.x == 0) {
    if (p.per_row) p.per_row[blockIdx.x] = value;
    if (p.loss_sum) atomicAdd(p.loss_sum, (double)value / (double)p.n_global);   // the mean's share in fp64
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void distill_entropy_kernel(const float* __restrict__ logits,
                                                                   float* __restrict__ per_row,
                                                                   double* __restrict__ sum, int C, int n_global) {
  __shared__ float sh[4];
  const float* __restrict__ xr = logits + (long)blockIdx.x * C;
  float x[kSlots];
  load_row<MODE>(x, xr, C);
  float mx, z;
  row_max_sumexp<MODE>(x, xr, C, 1.f, sh, mx, z);
  const float lz = logf(z), inv_z = 1.f / z;
  float acc = 0.f;
  each<MODE>(x, x, xr, nullptr, C, [&](int, float v, float) {
    const float u = v - mx;
    acc = fmaf(__expf(u) * inv_z, lz - u, acc);        // -p log p, log p = u - lz
  });
  const float h = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    if (per_row) per_row[blockIdx.x] = h;
    if (sum) atomicAdd(sum, (double)h / (double)n_global);
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void distill_softmax_acc_kernel(const float* __restrict__ logits,
                                                                       float* __restrict__ probs, float weight,
                                                                       int accumulate, int C) {
  __shared__ float sh[4];
  const long base = (long)blockIdx.x * C;
  const float* __restrict__ xr = logits + base;
  float x[kSlots];
  load_row<MODE>(x, xr, C);
  float mx, z;
  row_max_sumexp<MODE>(x, xr, C, 1.f, sh, mx, z);
  const float scale = weight / z;
  emit<MODE>(probs + base, accumulate, x, x, xr, nullptr, C, [&](int, float v, float) { return __expf(v - mx) * scale; });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the walk of a row: cached in registers up to 4096 columns, 16-byte accesses when every row base is 16-byte aligned
int row_mode(int C, const void* a, const void* b, const void* c) {
  if (C > kCachedMaxC) return MODE_STREAM;
  return (C % 4 == 0 && aligned16(a) && (!b || aligned16(b)) && (!c || aligned16(c))) ? MODE_VEC : MODE_SCALAR;
}

template <int KIND>
void launch_dist(int mode, const DistArgs& a, int n, hipStream_t stream) {
  if (mode == MODE_VEC) hipLaunchKernelGGL((distill_dist_kernel<KIND, MODE_VEC>), dim3(n), dim3(kThreads), 0, stream, a);
  else if (mode == MODE_SCALAR) hipLaunchKernelGGL((distill_dist_kernel<KIND, MODE_SCALAR>), dim3(n), dim3(kThreads), 0, stream, a);
  else hipLaunchKernelGGL((distill_dist_kernel<KIND, MODE_STREAM>), dim3(n), dim3(kThreads), 0, stream, a);
}

}  // namespace

extern "C" int bv_distill_dist(int kind, const float* student, const float* teacher, float* per_row, double* loss_sum,
                               float* dstudent, int accumulate, int n, int C, int n_global, float t, float ls,
                               float eps, int k, void* stream) {
  BV_REQUIRE(n > 0 && C > 0 && n_global >= n, "bv_distill_dist: bad shape n=%d C=%d n_global=%d", n, C, n_global);
  BV_REQUIRE(kind >= 0 && kind < BVD_KIND_COUNT, "bv_distill_dist: unknown kind %d", kind);
  BV_REQUIRE(student && teacher, "bv_distill_dist: NULL student or teacher");
  BV_REQUIRE(kind != BVD_KIND_KL || t > 0.f, "bv_distill_dist: kl needs a temperature t > 0 (got %g)", (double)t);
  BV_REQUIRE(kind != BVD_KIND_HARD || C > 1 || ls == 0.f, "bv_distill_dist: label smoothing needs C > 1 (ls / (C - 1))");
  BV_REQUIRE(kind != BVD_KIND_AGREE || (k >= 1 && !dstudent), "bv_distill_dist: agree needs k >= 1 and has no derivative");
  BV_REQUIRE(eps >= 0.f, "bv_distill_dist: eps < 0");
  DistArgs a{student, teacher, per_row, loss_sum, dstudent, accumulate != 0, C, k, n_global, 1.f / (float)n_global, t, ls, eps};
  const int mode = row_mode(C, student, teacher, dstudent);
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case BVD_KIND_L2: launch_dist<BVD_KIND_L2>(mode, a, n, s); break;
    case BVD_KIND_EUCLIDEAN: launch_dist<BVD_KIND_EUCLIDEAN>(mode, a, n, s); break;
    case BVD_KIND_KL: launch_dist<BVD_KIND_KL>(mode, a, n, s); break;
    case BVD_KIND_HARD: launch_dist<BVD_KIND_HARD>(mode, a, n, s); break;
    case BVD_KIND_LOGSOFTMAX_EUCLIDEAN: launch_dist<BVD_KIND_LOGSOFTMAX_EUCLIDEAN>(mode, a, n, s); break;
    default: launch_dist<BVD_KIND_AGREE>(mode, a, n, s); break;
  }
  return bv_check_launch("bv_distill_dist");
}

extern "C" int bv_distill_entropy(const float* logits, float* per_row, double* sum, int n, int C, int n_global,
                                  void* stream) {
  BV_REQUIRE(n > 0 && C > 0 && n_global >= n, "bv_distill_entropy: bad shape n=%d C=%d n_global=%d", n, C, n_global);
  BV_REQUIRE(logits, "bv_distill_entropy: NULL logits");
  const int mode = row_mode(C, logits, nullptr, nullptr);
  hipStream_t s = (hipStream_t)stream;
  if (mode == MODE_VEC) hipLaunchKernelGGL(distill_entropy_kernel<MODE_VEC>, dim3(n), dim3(kThreads), 0, s, logits, per_row, sum, C, n_global);
  else if (mode == MODE_SCALAR) hipLaunchKernelGGL(distill_entropy_kernel<MODE_SCALAR>, dim3(n), dim3(kThreads), 0, s, logits, per_row, sum, C, n_global);
  else hipLaunchKernelGGL(distill_entropy_kernel<MODE_STREAM>, dim3(n), dim3(kThreads), 0, s, logits, per_row, sum, C, n_global);
  return bv_check_launch("bv_distill_entropy");
}

extern "C" int bv_distill_softmax_acc(const float* logits, float* probs, float weight, int accumulate, int n, int C,
                                      void* stream) {
  BV_REQUIRE(n > 0 && C > 0, "bv_distill_softmax_acc: bad shape n=%d C=%d", n, C);
  BV_REQUIRE(logits && probs, "bv_distill_softmax_acc: NULL logits or probs");
  const int mode = row_mode(C, logits, probs, nullptr);
  hipStream_t s = (hipStream_t)stream;
  if (mode == MODE_VEC) hipLaunchKernelGGL(distill_softmax_acc_kernel<MODE_VEC>, dim3(n), dim3(kThreads), 0, s, logits, probs, weight, accumulate != 0, C);
  else if (mode == MODE_SCALAR) hipLaunchKernelGGL(distill_softmax_acc_kernel<MODE_SCALAR>, dim3(n), dim3(kThreads), 0, s, logits, probs, weight, accumulate != 0, C);
  else hipLaunchKernelGGL(distill_softmax_acc_kernel<MODE_STREAM>, dim3(n), dim3(kThreads), 0, s, logits, probs, weight, accumulate != 0, C);
  return bv_check_launch("bv_distill_softmax_acc");
}
