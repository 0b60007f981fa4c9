// Prints what big_vision_amd/csrc/gemm_route.h decides, for tests/test_gemm_route_cpu.py: a host program, no HIP, no GPU.
//   gemm_route_dump routes  < cases     one line per case
//   gemm_route_dump kernels < cases     every case under BV_OPT_GEMM_ROLL 0 .. 15 x column sums off / on x alpha = 1 / != 1:
//                                       the distinct instantiations the route names, one per line
//   gemm_route_dump defaults            gemm_default_opts(), its 10 fields in declaration order on one line
// A case is one line of 27 integers: the fields of bvgemm::GemmCall, then those of bvgemm::GemmOpts, in declaration order.
// A `routes` line, tab-separated:
//   family  kernel  splits  ktiles_per_split  k_chunk  grid.x  grid.y  grid.z  block  use_slab  slab_bytes  skew_cycles
//   skew_mode  group_n  multi  fused
// with the kernel written as c++filt writes the instantiation (default template arguments spelled out).
#include <cstdio>
#include <set>
#include <string>

#include "../big_vision_amd/csrc/gemm_route.h"

using namespace bvgemm;

static const char* kernel_name(GemmKernel k) {
  switch (k) {
    case G128_A0B0: return "gemm_bf16_kernel<false, false>";
    case G128_A0B1: return "gemm_bf16_kernel<false, true>";
    case G128_A1B0: return "gemm_bf16_kernel<true, false>";
    case G128_A1B1: return "gemm_bf16_kernel<true, true>";
    case G256_KMINOR: return "gemm256_kernel<false, 0, 0, false>";
    case G256_NONE_BF16: return "gemm256_kernel<true, 0, 0, false>";
    case G256_NONE_F32: return "gemm256_kernel<true, 0, 0, true>";
    case G256_RESIDUAL_BF16: return "gemm256_kernel<true, 0, 1, false>";
    case G256_RESIDUAL_F32: return "gemm256_kernel<true, 0, 1, true>";
    case G256_POS: return "gemm256_kernel<true, 0, 2, true>";
    case G256_GELU: return "gemm256_kernel<true, 0, 3, false>";
    case G256_GELU_BWD: return "gemm256_kernel<true, 0, 4, false>";
    case G256_GELU_BWD_EMIT: return "gemm256_kernel<true, 0, 6, false>";
    case G256_GELU_GD: return "gemm256_kernel<true, 0, 7, false>";
    case G256_MUL: return "gemm256_kernel<true, 0, 8, false>";
    case G256_GELU_G: return "gemm256_kernel<true, 0, 9, false>";
    case G256R_NONE: return "gemm256r_kernel<0, false, 0>";
    case G256R_NONE_ST: return "gemm256r_kernel<0, false, 1>";
    case G256R_RESIDUAL_F32: return "gemm256r_kernel<1, true, 0>";
    case G256R_GELU: return "gemm256r_kernel<3, false, 0>";
    case G256R_GELU_ST: return "gemm256r_kernel<3, false, 1>";
  }
  return "?";
}

// The family a kernel belongs to must be the family the route states.
static bool family_holds(const GemmRoute& r) {
  const std::string k = kernel_name(r.kernel);
  const char* want = r.family == GEMM_128 ? "gemm_bf16_kernel<" : r.family == GEMM_256 ? "gemm256_kernel<" : "gemm256r_kernel<";
  return k.rfind(want, 0) == 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc == 2 ? argv[1] : "";
  if (mode == "defaults") {
    constexpr GemmOpts d = gemm_default_opts();
    std::printf("%d %d %d %d %d %d %d %d %ld %d\n", (int)d.fast_path, d.roll, d.reserve, d.skew_pct, d.skew_mode, d.group_n, d.nt,
                d.pre_issue, d.ws_bytes, (int)d.has_ws);
    return 0;
  }
  if (mode != "routes" && mode != "kernels") {
    std::fprintf(stderr, "usage: %s routes|kernels < cases, or %s defaults\n", argv[0], argv[0]);
    return 2;
  }
  std::set<std::string> seen;
  long v[27];
  for (;;) {
    int n = 0;
    while (n < 27 && std::scanf("%ld", &v[n]) == 1) ++n;
    if (n == 0) break;
    if (n != 27) {
      std::fprintf(stderr, "a case needs 27 integers\n");
      return 2;
    }
    GemmCall c{v[0] != 0, v[1] != 0, (int)v[2], (int)v[3], (int)v[4], v[5], v[6], v[7], v[8], (unsigned)v[9], v[10] != 0,
               v[11] != 0, v[12] != 0, (int)v[13], v[14] != 0, v[15] != 0, (int)v[16]};
    GemmOpts o{v[17] != 0, (int)v[18], (int)v[19], (int)v[20], (int)v[21], (int)v[22], (int)v[23], (int)v[24], v[25], v[26] != 0};
    if (c.M <= 0 || c.N <= 0 || c.K <= 0) {
      std::fprintf(stderr, "M, N, K must be positive\n");
      return 2;
    }
    if (mode == "kernels") {
      for (o.roll = 0; o.roll < 16; ++o.roll)
        for (int cs = 0; cs < 2; ++cs)
          for (int a1 = 0; a1 < 2; ++a1) {
            c.has_colsum = cs != 0;
            c.alpha_is_one = a1 != 0;
            const GemmRoute r = gemm_route(c, o);
            if (!family_holds(r)) return 3;
            seen.insert(kernel_name(r.kernel));
          }
      continue;
    }
    const GemmRoute r = gemm_route(c, o);
    if (!family_holds(r)) return 3;
    std::printf("%d\t%s\t%d\t%d\t%d\t%u\t%u\t%u\t%u\t%d\t%ld\t%d\t%d\t%d\t%d\t%d\n", (int)r.family, kernel_name(r.kernel), r.splits,
                r.ktiles_per_split, r.k_chunk, r.grid.x, r.grid.y, r.grid.z, r.block, (int)r.use_slab, r.slab_bytes,
                r.skew_cycles, r.skew_mode, r.group_n, (int)r.multi, (int)r.fused);
  }
  for (const std::string& k : seen) std::printf("%s\n", k.c_str());
  return 0;
}
