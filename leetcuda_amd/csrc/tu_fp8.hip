// tu_fp8.hip — translation unit of the fp8 GEMM kernels (gemm_fp8.hip) — see lc_launch.h
#include "lc_plan.h"
#include "gemm_fp8.hip"

namespace lc {
// one workgroup per 256 x 256 tile of the plan; extra: the kernel's arguments behind the panel width
template <typename KernelT, typename... Extra>
static int launch_tiles(KernelT kern, int threads, int lds, const GemmFp8Plan& p, const GemmFp8Ptrs& a, Extra... extra) {
  if (int rc = set_dyn_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(threads), lds, a.st, a.A, a.B, a.C, p.call.M, p.call.N, p.call.K, a.alpha, p.tiles_m,
                     p.tiles_n, p.panel_w, extra...);
  return check_launch();
}

int launch_gemm_fp8_plan(const GemmFp8Plan& p, const GemmFp8Ptrs& a) {
  switch (p.kern) {
    case Fp8Kern::W4: return launch_tiles(gemm_fp8_w4_kernel, 256, W4B_LDS, p, a, stagger_arg(p.call.K / BK8));   // K-loop stagger as hgemm_w4y (lc_launch.h)
    case Fp8Kern::PINGPONG2_MX: return launch_tiles(gemm_fp8_pingpong2_kernel<true>, 512, HGEMM256_LDS, p, a);
    case Fp8Kern::PINGPONG2: return launch_tiles(gemm_fp8_pingpong2_kernel<false>, 512, HGEMM256_LDS, p, a);
    default: return launch_gemm_fp8_w4k_plan(p, a);   // tu_fp8k.hip
  }
}
}  // namespace lc
