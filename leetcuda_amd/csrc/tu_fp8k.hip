// tu_fp8k.hip — translation unit of the K = 128 MX fp8 GEMM kernel (gemm_fp8_w4k.hip) — see lc_launch.h
#include "lc_plan.h"
#include "gemm_fp8_w4k.hip"

namespace lc {
template <bool MX>
static int launch_w4k(const GemmFp8Plan& p, const GemmFp8Ptrs& a) {
  auto kern = gemm_fp8_w4k_kernel<MX>;
  if (int rc = set_dyn_lds(kern, W4B_LDS)) return rc;
  const PersistWalk w = persist_walk(p.tiles_m * p.tiles_n);   // persistent workgroups under hgemm_w4y's rule (lc_launch.h)
  hipLaunchKernelGGL(kern, dim3(w.grid), dim3(256), W4B_LDS, a.st, a.A, a.B, a.C, p.call.M, p.call.N, p.call.K, a.alpha, p.tiles_m, p.tiles_n,
                     p.panel_w, stagger_arg(p.call.K / BK8K), w.nblk, a.PA, a.PB);
  return check_launch();
}

int launch_gemm_fp8_w4k_plan(const GemmFp8Plan& p, const GemmFp8Ptrs& a) {
  if (p.kern == Fp8Kern::W4K) return launch_w4k<false>(p, a);
  return p.kern == Fp8Kern::W4K_MX ? launch_w4k<true>(p, a) : LC_ERR_ARG;
}

int launch_mx_pack_scales(const uint8_t* S, uint32_t* P, int rows, int K, hipStream_t st) {
  const size_t total = (size_t)(rows / 128) * (K / BK8K) * 128;
  hipLaunchKernelGGL(mx_pack_scales_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, S, P, rows, K);
  return check_launch();
}
}  // namespace lc
