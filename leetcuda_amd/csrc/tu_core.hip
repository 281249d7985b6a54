// tu_core.hip — translation unit of the builtin-MFMA kernels (attn_fwd.hip, hgemm_generic / edge / mfma128 / mfma256 / pingpong.hip) and of the
// launchers that run a plan (lc_plan.h): launch_hgemm, launch_attn_plan — see lc_launch.h
#include <limits.h>
#include <math.h>

#include "lc_plan.h"
#include "tu_attn_lockstep_impl.h"
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
template <int D, int NW, bool VT, bool BF16 = false>
int launch_attn_bigd(const AttnPtrs& a, int BH, int N) {
  constexpr int DO = D > 256 ? 256 : D;   // output columns per workgroup (D = 512: two column halves)
  const int nqb = N / (NW * 32);
  return launch_attn_kernel(attn_fwd_bigd_kernel<D, DO, NW, VT, BF16>, dim3((unsigned)((size_t)nqb * BH * (D / DO))), dim3(NW * 64), attn_bigd_lds_bytes<NW>(),
                            a.st, a.Q, a.K, a.V, a.O, N, nqb, attn_scale_log2e(D));
}
template <int D, bool VT>   // the column-split kernel (bf16: D = 256 / 512, V as [B,H,N,D])
int launch_colsplit(int nw, bool bf16, const AttnPtrs& a, int BH, int N) {
  if constexpr (!VT && D != 1024) {
    if (bf16) return nw == 4 ? launch_attn_bigd<D, 4, false, true>(a, BH, N) : launch_attn_bigd<D, 2, false, true>(a, BH, N);
  }
  return nw == 4 ? launch_attn_bigd<D, 4, VT>(a, BH, N) : launch_attn_bigd<D, 2, VT>(a, BH, N);
}
template <bool VT>
int launch_colsplit_d(int D, int nw, bool bf16, const AttnPtrs& a, int BH, int N) {
  return D == 256   ? launch_colsplit<256, VT>(nw, bf16, a, BH, N)
         : D == 512 ? launch_colsplit<512, VT>(nw, bf16, a, BH, N)
                    : launch_colsplit<1024, VT>(nw, bf16, a, BH, N);
}
}  // namespace

// ONE dispatch for every attention plan.  c.gqa > 1 (K / V hold H / c.gqa heads): the `_gqa` twin of the plan's kernel — fp16 and D <= 128 only;
// the merged-phase units by lookup (lc_launch.h), the lock-step twins in tu_attn_gqa.hip.  A plan without a kernel is LC_ERR_HEADDIM, never another kernel.
int launch_attn_plan(const AttnPlan& p, const AttnPtrs& a) {
  const AttnCall& c = p.call;
  const int BH = (int)c.bh, N = c.N, D = c.D;   // (B H < 2^31: the entry points bound the grid)
  const bool vt = c.vt, bf16 = c.bf16, g = c.gqa > 1;
  if (g && (bf16 || !is_small_headdim(D))) return LC_ERR_HEADDIM;
  switch (p.kern) {
    case AKern::W4U:
    case AKern::W4U_CAUSAL:
      if (const AttnW4uUnit* u = find_attn_w4u(D, vt, g))
        return p.kern == AKern::W4U ? u->launch(a, BH, N, p.walk, p.nsplit, c.gqa) : u->launch_causal(a, BH, N, p.order, c.gqa);
      break;
    case AKern::W4I:
      if (!vt) return kAttnW4iUnits[g]->launch(a, BH, N, D, p.sched, c.gqa);
      break;
    case AKern::LOCKSTEP:
    case AKern::LOCKSTEP_CAUSAL:
      if (g) return launch_attn_lockstep_gqa(a, BH, N, D, vt, p.kern == AKern::LOCKSTEP_CAUSAL, p.nw, c.gqa);
#ifdef LC_DIAG
      if (p.kern == AKern::LOCKSTEP && D == 128 && !vt) {   // perf-diagnosis instantiations (lc_tune_set "attn_ablate")
        switch (p.abl) {
          case 1: return launch_lockstep_t<128, 8, false, false, 1>(a, BH, N, 1);
          case 2: return launch_lockstep_t<128, 8, false, false, 2>(a, BH, N, 1);
          case 3: return launch_lockstep_t<128, 8, false, false, 3>(a, BH, N, 1);
          case 4: return launch_lockstep_t<128, 8, false, false, 4>(a, BH, N, 1);
          case 6: return launch_lockstep_t<128, 8, false, false, 6>(a, BH, N, 1);
          case 7: return launch_lockstep_t<128, 8, false, false, 7>(a, BH, N, 1);
          case 8: return launch_lockstep_t<128, 8, false, false, 8>(a, BH, N, 1);
          case 16: return launch_lockstep_t<128, 8, false, false, 16>(a, BH, N, 1);
          case 24: return launch_lockstep_t<128, 8, false, false, 24>(a, BH, N, 1);
          case 30: return launch_lockstep_t<128, 8, false, false, 30>(a, BH, N, 1);
          case 31: return launch_lockstep_t<128, 8, false, false, 31>(a, BH, N, 1);
          case 32: return launch_lockstep_t<128, 8, false, false, 32>(a, BH, N, 1);
          default: break;
        }
      }
#endif
      return launch_lockstep(a, BH, N, D, vt, p.kern == AKern::LOCKSTEP_CAUSAL, p.nw, 1);
    case AKern::BIGD4: return launch_attn_bigd4(a, BH, N, p.span8);
    case AKern::BIGD6: return launch_attn_bigd6(a, BH, N, bf16);
    case AKern::BIGD7: return vt ? launch_attn_bigd7_vt(a, BH, N) : launch_attn_bigd7(a, BH, N, bf16);
    case AKern::BIGD2:
    case AKern::BIGD3: return vt ? launch_attn_bigd2_vt(a, BH, N, D) : launch_attn_bigd2(a, BH, N, D, bf16, p.kern == AKern::BIGD3);
    case AKern::COLSPLIT: return vt ? launch_colsplit_d<true>(D, p.nw, bf16, a, BH, N) : launch_colsplit_d<false>(D, p.nw, bf16, a, BH, N);
  }
  return LC_ERR_HEADDIM;
}

int launch_clock_probe(unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(lc_clock_probe_kernel, dim3(1), dim3(64), 0, st, out);
  return check_launch();
}

}  // namespace lc
