// tu_w4.hip — translation unit of the 4-wave HGEMM kernel (hgemm_w4.hip) — see lc_launch.h
#include "lc_launch.h"
#include "hgemm_w4y.hip"

namespace lc {
namespace {
template <bool B_KN, bool BUF, int DG>
int launch_w4_one(const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int tiles_m, int tiles_n, int pw,
                  hipStream_t st) {
  auto kern = hgemm_w4b_kernel<B_KN, BUF, DG>;
  if (int rc = set_dyn_lds(kern, W4B_LDS)) return rc;
  hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(256), W4B_LDS, st, A, B, C, M, N, K, tiles_m, tiles_n, pw);
  return check_launch();
}

// nblk_arg: blocks to launch (< tiles_m * tiles_n when the ragged last wave goes to the 128-tile kernel), <= 0 = all; an explicit
// argument of every launcher below — no per-call state lives at file scope, so concurrent host threads cannot see each other's grid
template <bool B_KN, int Y>   // Y: -1 = hgemm_w4x_kernel, 0.. = hgemm_w4y_kernel<.., Y>
int launch_w4x_one(const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int tiles_m, int tiles_n, int pw,
                   int nblk_arg, hipStream_t st) {
  auto kern = [] {
    if constexpr (Y < 0) return hgemm_w4x_kernel<B_KN>;
    else return hgemm_w4y_kernel<B_KN, Y>;
  }();
  if (int rc = set_dyn_lds(kern, W4B_LDS)) return rc;
  const int nblk = nblk_arg > 0 ? nblk_arg : tiles_m * tiles_n;
  if constexpr (Y < 0) {
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), W4B_LDS, st, A, B, C, M, N, K, tiles_m, tiles_n, pw);
  } else {
    const PersistWalk w = persist_walk(nblk);   // one workgroup per CU walks the block ids (hgemm_w4y.hip), or one per block (lc_launch.h)
    hipLaunchKernelGGL(kern, dim3(w.grid), dim3(256), W4B_LDS, st, A, B, C, M, N, K, tiles_m, tiles_n, pw, stagger_arg(K / BK), w.nblk);
  }
  return check_launch();
}

template <bool B_KN>
int launch_w4_t(const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int variant, int sched, int stamps, int abl, int tiles_m,
                int tiles_n, int pw, int nblk, hipStream_t st) {
#ifdef LC_DIAG
  if (variant == LC_HGEMM_MFMA256W4C && stamps)
    return launch_w4_one<B_KN, true, 1>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
  if (variant == LC_HGEMM_MFMA256W4C && abl) {
    switch (abl) {   // bits: 2 no DMA, 4 no wait + barrier, 8 no fragment reads
      case 2: return launch_w4_one<B_KN, true, 2>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
      case 4: return launch_w4_one<B_KN, true, 4>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
      case 6: return launch_w4_one<B_KN, true, 6>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
      case 8: return launch_w4_one<B_KN, true, 8>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
      case 14: return launch_w4_one<B_KN, true, 14>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
      default: return LC_ERR_ARG;
    }
  }
#endif
  if constexpr (!B_KN) {
    if (variant == LC_HGEMM_MFMA256W4X) return launch_w4x_one<B_KN, -1>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
    if (variant == LC_HGEMM_MFMA256W4Y) {
      if (sched == 0) return launch_w4x_one<B_KN, 0>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
      if (sched == 1) return launch_w4x_one<B_KN, 1>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
#ifdef LC_DIAG
      if (sched == 3) return launch_w4x_one<B_KN, 3>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
      if (sched == 4) return launch_w4x_one<B_KN, 4>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
      if (sched == 5) return launch_w4x_one<B_KN, 5>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
      if (sched == 6) return launch_w4x_one<B_KN, 6>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);   // k-step-outer twin of the pair loop (correct results)
#endif
      return launch_w4x_one<B_KN, 2>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);
    }
  } else {
    if (variant == LC_HGEMM_MFMA256W4Y) return launch_w4x_one<B_KN, 1>(A, B, C, M, N, K, tiles_m, tiles_n, pw, nblk, st);   // one NN schedule
  }
  if (variant == LC_HGEMM_MFMA256W4C || variant == LC_HGEMM_MFMA256W4X || variant == LC_HGEMM_MFMA256W4Y)
    return launch_w4_one<B_KN, true, 0>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
  return launch_w4_one<B_KN, false, 0>(A, B, C, M, N, K, tiles_m, tiles_n, pw, st);
}
}  // namespace

int launch_w4_family(const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int variant, int sched, int stamps, int abl, bool b_kn,
                     int tiles_m, int tiles_n, int panel_w, int nblk, hipStream_t st) {
  return b_kn ? launch_w4_t<true>(A, B, C, M, N, K, variant, sched, stamps, abl, tiles_m, tiles_n, panel_w, nblk, st)
              : launch_w4_t<false>(A, B, C, M, N, K, variant, sched, stamps, abl, tiles_m, tiles_n, panel_w, nblk, st);
}
}  // namespace lc
