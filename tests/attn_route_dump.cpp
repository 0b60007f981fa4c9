// Prints what big_vision_amd/csrc/attn_route.h decides, for tests/test_attn_route_cpu.py: a host program, no HIP, no GPU.
//   attn_route_dump LMAX CFG...
// One line per (cfg, masked, Dh in 8, 16 .. 128, L in 1 .. LMAX), tab-separated:
//   L Dh masked cfg  forward KF  forward kernel  backward family  backward KF  backward kernels  bias_dpp
// with the kernels written as tests/test_kernel_buckets_gpu.py writes them (fwd<KF,NW,WPS,TAIL>, attn5<KF,LW>,
// dq1<KF,NW,WPS,TAIL> or dq<KF,NW,WPS> + dkv<KF,NW,WPS> or dkv32<KF,NW>) and "adh" for attention_dh.hip.  The calls are
// those of bv_attn3_fwd / bv_attn3_bwd: the forward has its output, the masked backward has none.
#include <cstdio>
#include <cstdlib>

#include "../big_vision_amd/csrc/attn_route.h"

using namespace bvattn;

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s LMAX CFG...\n", argv[0]);
    return 2;
  }
  const int lmax = std::atoi(argv[1]);
  for (int a = 2; a < argc; ++a) {
    const long cfg = std::atol(argv[a]);
    for (int masked = 0; masked < 2; ++masked)
      for (int Dh = 8; Dh <= 128; Dh += 8)
        for (int L = 1; L <= lmax; ++L) {
          const AttnRoute f = attn_route(L, Dh, masked != 0, cfg, true), b = attn_route(L, Dh, masked != 0, cfg, !masked);
          std::printf("%d\t%d\t%d\t%ld\t%d\t", L, Dh, masked, cfg, f.KF);
          if (f.family == ATTN_ADH) std::printf("adh");
          else std::printf("fwd<%d,%d,%d,%d>", f.KF, f.fwd.NW, f.fwd.WPS, (int)f.tail);
          std::printf("\t%s\t%d\t", b.family == ATTN_ADH ? "adh" : b.family == ATTN_5 ? "attn5" : "attn3", b.KF);
          if (b.family == ATTN_ADH) std::printf("adh");
          else if (b.family == ATTN_5) std::printf("attn5<%d,%d>", b.KF, b.LW);
          else {
            if (b.dq1) std::printf("dq1<%d,%d,%d,%d>", b.KF, b.dq.NW, b.dq.WPS, (int)b.tail);
            else std::printf("dq<%d,%d,%d>", b.KF, b.dq.NW, b.dq.WPS);
            if (b.dkv_kind == DKV_16) std::printf("+dkv<%d,%d,%d>", b.KF, b.dkv.NW, b.dkv.WPS);
            else std::printf("+dkv32<%d,%d>", b.KF, b.dkv_kind == DKV_32X7 ? 7 : 4);
          }
          std::printf("\t%d\n", (int)b.bias_dpp);
        }
  }
  return 0;
}
