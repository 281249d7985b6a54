// tu_core.hip — translation unit of the builtin-MFMA kernels (attn_fwd.hip, hgemm_generic / edge / mfma128 / mfma256 / pingpong.hip) and of the
// launchers that run a plan (lc_plan.h): launch_hgemm, launch_attn_plan — see lc_launch.h
#include <limits.h>
#include <math.h>

#include "lc_plan.h"
#include "attn_fwd.hip"
#include "hgemm_generic.hip"
#include "hgemm_edge.hip"
#include "hgemm_mfma128.hip"
#include "hgemm_mfma256.hip"
#include "hgemm_pingpong.hip"

extern "C" __global__ void lc_clock_probe_kernel(unsigned long long* out) {
  if (threadIdx.x == 0) {
    out[0] = __builtin_readcyclecounter();        // s_memtime: shader cycles
    out[1] = __builtin_amdgcn_s_memrealtime();    // constant 100 MHz
  }
}

namespace lc {
namespace {

// ------------------------------------------------------------------------------------------------
// HGEMM launchers
template <bool B_KN>
int launch_mfma128_blocks(int ksw, int nblocks, const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int tiles_m, int tiles_n,
                          int pw, int rem_base, int rem_blocks, int nright, int ks, float* ws, hipStream_t st) {
  const bool eight = ksw == 2 && ks == 1;   // (ks == 1: no workspace, ws == nullptr)
  auto kern = eight ? hgemm_mfma128_kernel<B_KN, 2> : hgemm_mfma128_kernel<B_KN, 1>;
  if (int rc = set_dyn_lds(kern, HGEMM128_LDS)) return rc;
  hipLaunchKernelGGL(kern, dim3(nblocks * ks), dim3(eight ? 512 : 256), HGEMM128_LDS, st, A, B, C, M, N, K, tiles_m, tiles_n, pw, rem_base, rem_blocks,
                     nright, ks, ws);
  return check_launch();
}

// hgemm_w4y_kernel (or its 4-wave siblings) on the plan's 256 x 256 tiles, then the ragged last round on the mid-size kernel when the plan says so
int launch_w4_tail(const HgemmPlan& p, const half_t* A, const half_t* B, half_t* C, int M, int N, int K, bool b_kn, int pw, hipStream_t st) {
  if (int rc = launch_w4_family(A, B, C, M, N, K, p.w4, p.sched, p.k.hgemm_stamps, p.k.w4_abl, b_kn, p.tiles_m, p.tiles_n, pw, p.tail.nblk, st))
    return rc;
  if (!p.tail.tmw) return LC_OK;
  return launch_hgemm_mid_rem(A, B, C, M, N, K, b_kn, p.tail.tmw, p.tail.ns, p.tiles_m, p.tiles_n, pw, p.tail.nblk, p.tail.R, st);
}

template <bool B_KN>
int launch_mfma256(const HgemmPlan& p, const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int swizzle_stride, hipStream_t st) {
  const int pw = panel_tiles(p.k.hgemm_raster, swizzle_stride, p.tiles_n, BN, ((size_t)M + N) * K * 2);
  if (p.w4) {
    if (int rc = launch_w4_tail(p, A, B, C, M, N, K, B_KN, pw, st)) return rc;
    if (p.nb128 == 0) return LC_OK;
    // the border strips and / or the tail quadrants on the 128-tile kernel; split-K partials in this stream's cached workspace — not while the
    // stream is being captured (no allocation, no pool pointer inside a graph): one block per tile then
    const bool split = p.tail.nblk >= 0;
    int ks = p.ks;
    WorkspaceLease lease;
    if (ks > 1 && !stream_is_capturing(st)) lease = stream_workspace(st, (size_t)p.nb128 * ks * (128 * 128 * sizeof(float)));
    if (!lease.ptr) ks = 1;
    if (int rc = launch_mfma128_blocks<B_KN>(p.ksw, p.nb128, A, B, C, M, N, K, p.tiles_m, p.tiles_n, pw, split ? p.tail.nblk : -2,
                                             split ? 4 * p.tail.R : 0, p.nright, ks, static_cast<float*>(lease.ptr), st))
      return rc;
    if (ks > 1) {
      hipLaunchKernelGGL(hgemm_splitk_reduce_kernel, dim3(p.nb128), dim3(256), 0, st, static_cast<const float*>(lease.ptr), C, M, N, p.tiles_m,
                         p.tiles_n, pw, split ? p.tail.nblk : -2, split ? 4 * p.tail.R : 0, p.nright, ks);
      return check_launch();
    }
    return LC_OK;
  }
  auto launch = [&](auto kern) {   // the 8-wave cross-check kernels
    if (int rc = set_dyn_lds(kern, HGEMM256_LDS)) return rc;
    hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(512), HGEMM256_LDS, st, A, B, C, M, N, K, p.tiles_m, p.tiles_n, pw);
    return check_launch();
  };
#ifdef LC_DIAG
  if (p.variant == LC_HGEMM_MFMA256P2 && p.k.hgemm_stamps) return launch(hgemm_pingpong2_kernel<B_KN, true>);
#endif
  if (p.variant == LC_HGEMM_MFMA256P2) return launch(hgemm_pingpong2_kernel<B_KN>);
  return launch(hgemm_mfma256_kernel<B_KN>);
}

int launch_mid(const HgemmPlan& p, const half_t* A, const half_t* B, half_t* C, int M, int N, int K, bool b_kn, int swizzle_stride, hipStream_t st) {
  const MidTile t = p.mid;
  const int pw = panel_tiles(p.k.hgemm_raster, swizzle_stride, N / (64 * t.tnw), 64 * t.tnw, ((size_t)M + N) * K * 2);
  if (t.ks > 1 && !stream_is_capturing(st)) {
    WorkspaceLease lease = stream_workspace(st, (size_t)t.ks * M * N * sizeof(float));
    if (lease.ptr) return launch_hgemm_mid(A, B, C, M, N, K, b_kn, t.tmw, t.tnw, 3, pw, st, static_cast<float*>(lease.ptr), t.ks);
  }
  return launch_hgemm_mid(A, B, C, M, N, K, b_kn, t.tmw, t.tnw, t.ns, pw, st);   // (no workspace — graph capture, allocation failure: one K range)
}

// hgemm_edge_kernel over the right strip (all rows, columns Ni .. N) and the bottom strip (rows Mi .. M, columns 0 .. Ni) of C; Mi = Ni = 0:
// the whole matrix.  Ni % 128 == 0.
template <bool B_KN>
int launch_edge(const half_t* A, const half_t* B, half_t* C, int M, int N, int K, int Mi, int Ni, hipStream_t st) {
  const long nrc = (N - Ni + EN - 1) / EN, nright = nrc * ((M + EM - 1) / EM);
  const long nbottom = (long)((M - Mi + EM - 1) / EM) * (Ni / EN);
  if (nright + nbottom <= 0) return LC_OK;
  if (nright + nbottom > INT_MAX) return LC_ERR_SHAPE;
  auto kern = hgemm_edge_kernel<B_KN>;
  if (int rc = set_dyn_lds(kern, EDGE_LDS)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nright + nbottom)), dim3(256), EDGE_LDS, st, A, B, C, M, N, K, Mi, Ni, (int)nright, (int)(nrc > 0 ? nrc : 1));
  return check_launch();
}
template <bool B_KN>
int launch_generic(const half_t* A, const half_t* B, half_t* C, int M, int N, int K, hipStream_t st) {
  const dim3 grid((N + GN - 1) / GN, (M + GM - 1) / GM), block(256);
  hipLaunchKernelGGL(hgemm_generic_kernel<B_KN>, grid, block, 0, st, A, B, C, M, N, K);
  return check_launch();
}

// The border launch beside the interior (HgemmPlan::fork): one side stream per device, forked from the caller's stream
// by an event and joined back by another, so that the edge blocks (one 72 KiB workgroup per CU at best, a latency-bound K walk) fill the CUs
// the interior's last round leaves idle instead of holding the whole GPU for a round of their own.  The device's mutex (the one the workspace
// leases hold) covers the enqueue sequence: two host threads cannot interleave their fork / join events.  Not while the caller's stream is being
// captured, not when the side stream cannot be created: both launches on the caller's stream then.
struct ForkLane { hipStream_t side = nullptr; hipEvent_t fork = nullptr, join = nullptr; bool tried = false; };
ForkLane* fork_lane(int dev) {   // (call with the device's mutex held)
  static ForkLane lanes[64];
  if (dev < 0 || dev >= 64) return nullptr;
  ForkLane& l = lanes[dev];
  if (!l.tried) {
    l.tried = true;
    RelaxedCaptureMode relaxed;
    int least = 0, greatest = 0;   // (the lowest priority, for what it is worth)
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    if (hipStreamCreateWithPriority(&l.side, hipStreamNonBlocking, least) != hipSuccess || hipEventCreateWithFlags(&l.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&l.join, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      l.side = nullptr;
    }
  }
  return l.side ? &l : nullptr;
}

int launch_ragged(const HgemmPlan& p, const half_t* A, const half_t* B, half_t* C, int M, int N, int K, bool b_kn, int swizzle_stride, hipStream_t st) {
  const RaggedPlan& r = p.rag;
  if (r.kind == 2) {
    if (r.ks > 1 && !stream_is_capturing(st)) {
      WorkspaceLease lease = stream_workspace(st, launch_hgemm_mid_edge_sk_floats(M, N, r.tmw, r.ks) * sizeof(float));
      if (lease.ptr) return launch_hgemm_mid_edge_sk(A, B, C, M, N, K, b_kn, r.tmw, r.ks, static_cast<float*>(lease.ptr), st);
    }
    return launch_hgemm_mid_edge(A, B, C, M, N, K, b_kn, r.tmw, r.tnw, r.ns, 0, 0, st);   // (no workspace — graph capture, allocation failure: one K range)
  }
  // kind 1: the interior as a problem of its own (+ its last round), the border on hgemm_mid_edge_kernel
  const int pw = panel_tiles(p.k.hgemm_raster, swizzle_stride, p.tiles_n, BN, ((size_t)p.tiles_m * BM + (size_t)p.tiles_n * BN) * K * 2);
  int dev = 0;
  if (p.fork && !workspace_held_by_this_thread() && !stream_is_capturing(st) && hipGetDevice(&dev) == hipSuccess) {
    std::unique_lock<std::mutex> lock(workspace_pool(dev).mu);
    ForkLane* l = fork_lane(dev);
    if (l && hipEventRecord(l->fork, st) == hipSuccess && hipStreamWaitEvent(l->side, l->fork, 0) == hipSuccess) {
      // (the order of the two launches and the side stream's priority change nothing measurable)
      int rc = launch_w4_tail(p, A, B, C, M, N, K, b_kn, pw, st);
      if (rc == LC_OK) rc = launch_hgemm_mid_edge(A, B, C, M, N, K, b_kn, 2, 2, r.ns, r.Mi, r.Ni, l->side);
      const bool joined = hipEventRecord(l->join, l->side) == hipSuccess;
      if (!joined || hipStreamWaitEvent(st, l->join, 0) != hipSuccess) {   // (cannot order the caller's stream behind the border: wait for it here)
        (void)hipGetLastError();
        (void)hipStreamSynchronize(l->side);
      }
      return rc;
    }
    (void)hipGetLastError();
  }
  if (int rc = launch_w4_tail(p, A, B, C, M, N, K, b_kn, pw, st)) return rc;
  return launch_hgemm_mid_edge(A, B, C, M, N, K, b_kn, 2, 2, r.ns, r.Mi, r.Ni, st);
}

}  // namespace

int launch_hgemm(const HgemmPlan& p, const half_t* A, const half_t* B, half_t* C, int M, int N, int K, bool b_kn, int swizzle_stride, hipStream_t st) {
  switch (p.fam) {
    case HFam::VALU: return launch_valu_rung(A, B, C, M, N, K, p.variant, st);
    case HFam::TILE256:
      return b_kn ? launch_mfma256<true>(p, A, B, C, M, N, K, swizzle_stride, st) : launch_mfma256<false>(p, A, B, C, M, N, K, swizzle_stride, st);
    case HFam::MFMA128: {
      const int tiles_m = M / BM1, tiles_n = N / BN1;
      const int pw = panel_tiles(p.k.hgemm_raster, swizzle_stride, tiles_n, BN1, ((size_t)M + N) * K * 2);
      return b_kn ? launch_mfma128_blocks<true>(p.ksw, tiles_m * tiles_n, A, B, C, M, N, K, tiles_m, tiles_n, pw, -1, 0, 0, 1, nullptr, st)
                  : launch_mfma128_blocks<false>(p.ksw, tiles_m * tiles_n, A, B, C, M, N, K, tiles_m, tiles_n, pw, -1, 0, 0, 1, nullptr, st);
    }
    case HFam::MID: return launch_mid(p, A, B, C, M, N, K, b_kn, swizzle_stride, st);
    case HFam::RAGGED: return launch_ragged(p, A, B, C, M, N, K, b_kn, swizzle_stride, st);
    case HFam::KPAD: {
      const int Kp = p.Kp;   // (A and B with K padded to Kp by zeros, in the workspace)
      if (!workspace_held_by_this_thread() && !stream_is_capturing(st)) {
        WorkspaceLease lease = stream_workspace(st, ((size_t)M + N) * Kp * 2);
        if (lease.ptr) {
          half_t* ap = static_cast<half_t*>(lease.ptr);
          half_t* bp = ap + (size_t)M * Kp;
          // A [M][K] -> [M][Kp]; B as [N][K] -> [N][Kp], as [K][N] -> [Kp][N] (zero rows behind the last k)
          const size_t ca = (size_t)M * (Kp / 8), cb = b_kn ? (size_t)Kp * (N / 8) : (size_t)N * (Kp / 8);
          hipLaunchKernelGGL(hgemm_pad_copy_kernel, dim3((unsigned)((ca + 255) / 256)), dim3(256), 0, st, A, ap, M, K, M, Kp);
          if (b_kn) hipLaunchKernelGGL(hgemm_pad_copy_kernel, dim3((unsigned)((cb + 255) / 256)), dim3(256), 0, st, B, bp, K, N, Kp, N);
          else hipLaunchKernelGGL(hgemm_pad_copy_kernel, dim3((unsigned)((cb + 255) / 256)), dim3(256), 0, st, B, bp, N, K, N, Kp);
          if (int rc = check_launch()) return rc;
          HgemmPlan inner;
          plan_hgemm(p.k, M, N, Kp, b_kn, LC_HGEMM_AUTO, true, &inner);   // (LC_HGEMM_AUTO always has a plan)
          workspace_held_by_this_thread() = true;   // the padded problem's launch: workspace-free forms, no fork
          const int rc = launch_hgemm(inner, ap, bp, C, M, N, Kp, b_kn, swizzle_stride, st);
          workspace_held_by_this_thread() = false;
          return rc;
        }
      }
      break;   // (graph capture, no workspace: every LC_HGEMM_KPAD shape is an edge-kernel shape)
    }
    case HFam::EDGE: break;
    case HFam::GENERIC: return b_kn ? launch_generic<true>(A, B, C, M, N, K, st) : launch_generic<false>(A, B, C, M, N, K, st);
  }
  return b_kn ? launch_edge<true>(A, B, C, M, N, K, 0, 0, st) : launch_edge<false>(A, B, C, M, N, K, 0, 0, st);
}

// ------------------------------------------------------------------------------------------------
// attention launchers
namespace {
template <int D, int NW, bool VT, int ABL = 0>
int launch_attn(const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N,
                hipStream_t st) {
  auto kern = attn_fwd_kernel<D, NW, VT, ABL>;
  constexpr int lds = attn_lds_bytes<D, VT>();
  if (int rc = set_dyn_lds(kern, lds)) return rc;
  const int nqb = N / (NW * 32);
  const dim3 grid((unsigned)((size_t)nqb * B * H)), block(NW * 64);
  const float sl2 = (1.0f / sqrtf((float)D)) * 1.4426950408889634f;
  hipLaunchKernelGGL(kern, grid, block, lds, st, Q, K, V, O, N, nqb, sl2);
  return check_launch();
}
template <int D, bool VT>
int launch_lockstep(const AttnPlan& p, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, hipStream_t st) {
#ifdef LC_DIAG
  if constexpr (D == 128 && !VT) {   // perf-diagnosis instantiations (lc_tune_set "attn_ablate")
    switch (p.abl) {
      case 1: return launch_attn<D, 8, VT, 1>(Q, K, V, O, B, H, N, st);
      case 2: return launch_attn<D, 8, VT, 2>(Q, K, V, O, B, H, N, st);
      case 3: return launch_attn<D, 8, VT, 3>(Q, K, V, O, B, H, N, st);
      case 4: return launch_attn<D, 8, VT, 4>(Q, K, V, O, B, H, N, st);
      case 6: return launch_attn<D, 8, VT, 6>(Q, K, V, O, B, H, N, st);
      case 7: return launch_attn<D, 8, VT, 7>(Q, K, V, O, B, H, N, st);
      case 8: return launch_attn<D, 8, VT, 8>(Q, K, V, O, B, H, N, st);
      case 16: return launch_attn<D, 8, VT, 16>(Q, K, V, O, B, H, N, st);
      case 24: return launch_attn<D, 8, VT, 24>(Q, K, V, O, B, H, N, st);
      case 30: return launch_attn<D, 8, VT, 30>(Q, K, V, O, B, H, N, st);
      case 31: return launch_attn<D, 8, VT, 31>(Q, K, V, O, B, H, N, st);
      case 32: return launch_attn<D, 8, VT, 32>(Q, K, V, O, B, H, N, st);
      default: break;
    }
  }
#endif
  if (p.nw == 8) return launch_attn<D, 8, VT>(Q, K, V, O, B, H, N, st);
  if (p.nw == 4) return launch_attn<D, 4, VT>(Q, K, V, O, B, H, N, st);
  return launch_attn<D, 2, VT>(Q, K, V, O, B, H, N, st);
}
template <int D, int NW, bool VT>
int launch_attn_causal(const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, hipStream_t st) {
  auto kern = attn_fwd_causal_kernel<D, NW, VT>;
  constexpr int lds = attn_lds_bytes<D, VT>();
  if (int rc = set_dyn_lds(kern, lds)) return rc;
  const int nqb = N / (NW * 32);
  const float sl2 = (1.0f / sqrtf((float)D)) * 1.4426950408889634f;
  hipLaunchKernelGGL(kern, dim3((unsigned)((size_t)nqb * B * H)), dim3(NW * 64), lds, st, Q, K, V, O, N, nqb, sl2);
  return check_launch();
}
template <int D, bool VT>
int launch_lockstep_causal(const AttnPlan& p, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, hipStream_t st) {
  if (p.nw == 8) return launch_attn_causal<D, 8, VT>(Q, K, V, O, B, H, N, st);
  if (p.nw == 4) return launch_attn_causal<D, 4, VT>(Q, K, V, O, B, H, N, st);
  return launch_attn_causal<D, 2, VT>(Q, K, V, O, B, H, N, st);
}

template <int D, int NW, bool VT, bool BF16 = false>
int launch_attn_bigd(const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N,
                     hipStream_t st) {
  constexpr int DO = D > 256 ? 256 : D;   // output columns per workgroup (D = 512: two column halves)
  auto kern = attn_fwd_bigd_kernel<D, DO, NW, VT, BF16>;
  constexpr int lds = attn_bigd_lds_bytes<NW>();
  if (int rc = set_dyn_lds(kern, lds)) return rc;
  const int nqb = N / (NW * 32);
  const dim3 grid((unsigned)((size_t)nqb * B * H * (D / DO))), block(NW * 64);
  const float sl2 = (1.0f / sqrtf((float)D)) * 1.4426950408889634f;
  hipLaunchKernelGGL(kern, grid, block, lds, st, Q, K, V, O, N, nqb, sl2);
  return check_launch();
}
template <int D, bool VT>   // the column-split kernel (bf16: D = 256 / 512, V as [B,H,N,D])
int launch_colsplit(const AttnPlan& p, bool bf16, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, hipStream_t st) {
  if constexpr (!VT && D != 1024) {
    if (bf16) return p.nw == 4 ? launch_attn_bigd<D, 4, false, true>(Q, K, V, O, B, H, N, st) : launch_attn_bigd<D, 2, false, true>(Q, K, V, O, B, H, N, st);
  }
  return p.nw == 4 ? launch_attn_bigd<D, 4, VT>(Q, K, V, O, B, H, N, st) : launch_attn_bigd<D, 2, VT>(Q, K, V, O, B, H, N, st);
}

template <bool VT>
int launch_attn_plan_vt(const AttnPlan& p, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, int D, bool bf16,
                        hipStream_t st) {
  switch (p.kern) {
    case AKern::W4U:
      if (D == 128) return VT ? launch_attn_w4u_d128t(Q, K, V, O, B, H, N, p.walk, p.nsplit, st) : launch_attn_w4u_d128(Q, K, V, O, B, H, N, p.walk, p.nsplit, st);
      return VT ? launch_attn_w4u_d64t(Q, K, V, O, B, H, N, p.walk, p.nsplit, st) : launch_attn_w4u_d64(Q, K, V, O, B, H, N, p.walk, p.nsplit, st);
    case AKern::W4I: return launch_attn_w4i(Q, K, V, O, B, H, N, D, p.sched, st);
    case AKern::LOCKSTEP:
      return D == 32   ? launch_lockstep<32, VT>(p, Q, K, V, O, B, H, N, st)
             : D == 64 ? launch_lockstep<64, VT>(p, Q, K, V, O, B, H, N, st)
             : D == 96 ? launch_lockstep<96, VT>(p, Q, K, V, O, B, H, N, st)
                       : launch_lockstep<128, VT>(p, Q, K, V, O, B, H, N, st);
    case AKern::BIGD4: return launch_attn_bigd4(Q, K, V, O, B, H, N, p.span8, st);
    case AKern::BIGD6: return launch_attn_bigd6(Q, K, V, O, B, H, N, bf16, st);
    case AKern::BIGD7: return VT ? launch_attn_bigd7_vt(Q, K, V, O, B, H, N, st) : launch_attn_bigd7(Q, K, V, O, B, H, N, bf16, st);
    case AKern::BIGD2:
    case AKern::BIGD3:
      return VT ? launch_attn_bigd2_vt(Q, K, V, O, B, H, N, D, st) : launch_attn_bigd2(Q, K, V, O, B, H, N, D, bf16, p.kern == AKern::BIGD3, st);
    case AKern::COLSPLIT:
      return D == 256   ? launch_colsplit<256, VT>(p, bf16, Q, K, V, O, B, H, N, st)
             : D == 512 ? launch_colsplit<512, VT>(p, bf16, Q, K, V, O, B, H, N, st)
                        : launch_colsplit<1024, VT>(p, bf16, Q, K, V, O, B, H, N, st);
    case AKern::W4U_CAUSAL:
      if (D == 128) return VT ? launch_attn_w4u_causal_d128t(Q, K, V, O, B, H, N, p.order, st) : launch_attn_w4u_causal_d128(Q, K, V, O, B, H, N, p.order, st);
      return VT ? launch_attn_w4u_causal_d64t(Q, K, V, O, B, H, N, p.order, st) : launch_attn_w4u_causal_d64(Q, K, V, O, B, H, N, p.order, st);
    case AKern::LOCKSTEP_CAUSAL:
      return D == 32   ? launch_lockstep_causal<32, VT>(p, Q, K, V, O, B, H, N, st)
             : D == 64 ? launch_lockstep_causal<64, VT>(p, Q, K, V, O, B, H, N, st)
             : D == 96 ? launch_lockstep_causal<96, VT>(p, Q, K, V, O, B, H, N, st)
                       : launch_lockstep_causal<128, VT>(p, Q, K, V, O, B, H, N, st);
  }
  return LC_ERR_HEADDIM;
}
}  // namespace

int launch_attn_plan(const AttnPlan& p, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, int D, bool vt, bool bf16,
                     hipStream_t st) {
  if (p.gqa > 1) return bf16 ? LC_ERR_HEADDIM : launch_attn_plan_gqa(p, Q, K, V, O, B, H, N, D, vt, st);   // (K / V hold H / p.gqa heads)
  return vt ? launch_attn_plan_vt<true>(p, Q, K, V, O, B, H, N, D, bf16, st) : launch_attn_plan_vt<false>(p, Q, K, V, O, B, H, N, D, bf16, st);
}

int launch_clock_probe(unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(lc_clock_probe_kernel, dim3(1), dim3(64), 0, st, out);
  return check_launch();
}

}  // namespace lc
