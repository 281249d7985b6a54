// tu_attn_w4u_impl.h — body of the four translation units tu_attn_w4u_{d128,d128t,d64,d64t}.hip: the merged-phase attention kernel
// (attn_w4u.hip) for ONE (head dim, V layout) and its three block walks.  The includer defines W4U_D, W4U_VT and W4U_TAG.
// With W4U_GQA defined (tu_attn_w4u_gqa_{d128,d128t,d64,d64t}.hip; W4U_TAG gqa_d128 ...) the unit holds the grouped-query forms instead
// (attn_w4u_gqa.hip): the same launchers, whose group size kvg = H / Hkv is handed to the kernels (the MHA kernels have no such argument and
// the MHA units are only ever handed 1); grids, walks, split-KV partials and the combine kernel are per query head and do not change.
// The unit exports one record, g_attn_w4u_<W4U_TAG> (lc_launch.h AttnW4uUnit).
#include <limits.h>

#include <atomic>

#include "lc_launch.h"
#define W4U_CAT2(a, b) a##b
#define W4U_CAT(a, b) W4U_CAT2(a, b)
#define LC_AN_SLOWPATH_SYM W4U_CAT(g_au_slowpath_, W4U_TAG)
#ifdef W4U_GQA
#include "attn_w4u_gqa.hip"
#define W4U_KERNEL attn_fwd_w4u_gqa_kernel
#define W4U_CAUSAL_KERNEL attn_fwd_w4u_causal_gqa_kernel
#define W4U_IS_GQA true
#else
#include "attn_w4u.hip"
#define W4U_KERNEL attn_fwd_w4u_kernel
#define W4U_CAUSAL_KERNEL attn_fwd_w4u_causal_kernel
#define W4U_IS_GQA false
#endif

namespace lc {
namespace {
template <int WALK>
int launch_w4u_walk(const AttnPtrs& a, half_t* O, int N, int grid_wgs, size_t nblk, int kvg, int nsplit = 1, float* lse = nullptr) {
  constexpr int D = W4U_D;
  static std::atomic<unsigned> ticket{0};     // rotating claim-counter slot of the dynamic walk (attn_w4u.hip g_w4u_queue)
  const int qslot = WALK == 2 ? (int)(ticket.fetch_add(1, std::memory_order_relaxed) % (unsigned)W4U_QSLOTS) : 0;
  return launch_attn_kernel_kvg<W4U_IS_GQA>(W4U_KERNEL<D, W4U_VT, WALK>, dim3((unsigned)grid_wgs), dim3(256), W4U<D>::LDS, a.st, kvg, a.Q, a.K, a.V, O, N,
                                            (N + 255) / 256, attn_scale_log2e(D), (int)nblk, grid_wgs, qslot, nsplit, lse);
}

// Split-KV (WALK 3): nsplit workgroups per query block write [nsplit][B H][N][D] fp16 partials + [nsplit][B H][N] fp32 log-sum-exps
// into this stream's cached workspace (lc_launch.h stream_workspace), then the combine kernel.  Returns LC_ERR_ARG when the split
// cannot run here (the stream is being captured into a graph — no allocation may happen, and a graph must not keep a pointer into a
// pool that can be regrown — or the allocator refuses): the caller then launches the one-block walk instead, never an error.
int launch_w4u_split(const AttnPtrs& a, int BH, int N, int nsplit, int kvg) {
  constexpr int D = W4U_D;
  if (stream_is_capturing(a.st)) return LC_ERR_ARG;
  const size_t rows = (size_t)BH * N;
  const size_t obytes = (size_t)nsplit * rows * D * sizeof(half_t), lbytes = (size_t)nsplit * rows * sizeof(float);
  WorkspaceLease ws = stream_workspace(a.st, obytes + lbytes);   // (held until both kernels are enqueued)
  if (!ws.ptr) return LC_ERR_ARG;
  half_t* op = static_cast<half_t*>(ws.ptr);
  float* lse = reinterpret_cast<float*>(static_cast<char*>(ws.ptr) + obytes);
  const size_t nblk = (size_t)(N / 256) * BH * nsplit;
  if (nblk > (size_t)INT_MAX) return LC_ERR_ARG;   // (the grid and the kernel's block count are ints: the caller runs the unsplit walk)
  if (int rc = launch_w4u_walk<3>(a, op, N, (int)nblk, nblk, kvg, nsplit, lse)) return rc;
  const size_t threads = rows * (D / 8);
  return launch_attn_kernel(attn_split_combine_kernel<D>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, a.st, op, lse, a.O, nsplit, rows);
}

// N % 256 == 0 (walk 0: also N % 256 == 128); walk: 0 one block per workgroup, 1 persistent static walk, 2 persistent dynamic queue.  A persistent walk with no
// more blocks than CUs IS the one-block launch; the dynamic queue needs a grid that is a multiple of the 8 XCDs.
// walk 3 = split-KV with `nsplit` (>= 2, N / 64 % nsplit == 0, >= 2 tiles per split: attn_split_auto, tu_plan.hip) workgroups per query
// block; when the split cannot run on this stream (graph capture, allocator) the one-block walk runs instead.
int launch_w4u(const AttnPtrs& a, int BH, int N, int walk, int nsplit, int kvg) {
  const size_t nblk = (size_t)((N + 255) / 256) * BH;  // (N % 256 != 0: the head's last block is partly real; one block per workgroup only)
  if (nblk > (size_t)INT_MAX) return LC_ERR_SHAPE;           // (int grid / block-count arguments; 2^31 query blocks = 2^39 query rows)
  const int ncu = device_cu_count();   // one workgroup per CU: each takes a CU's whole register file and > half its LDS
  if (N % 256 != 0) walk = 0;          // the persistent walks stage the NEXT block's tiles into ring slots T % 4 == 0 expects; split-KV needs whole blocks
  if (walk == 3) {
    if (nsplit >= 2 && (N / 64) % nsplit == 0 && (N / 64) / nsplit >= 2) {
      const int rc = launch_w4u_split(a, BH, N, nsplit, kvg);
      if (rc != LC_ERR_ARG) return rc;
    }
    walk = 0;
  }
  if (walk != 0 && nblk <= (size_t)ncu) walk = 0;
  if (walk == 2 && ncu % 8 != 0) walk = 1;
  if (walk == 2) {
    // the dynamic queue's claim-counter slot is picked by a host-side ticket AT LAUNCH TIME: captured into a graph it would be baked
    // in, and concurrent replays would share counters (round-4 advisor) -> the static walk while the stream is capturing
    if (stream_is_capturing(a.st)) walk = 1;
  }
  if (walk == 0) return launch_w4u_walk<0>(a, a.O, N, (int)nblk, nblk, kvg);
  if (walk == 1) return launch_w4u_walk<1>(a, a.O, N, ncu, nblk, kvg);
  return launch_w4u_walk<2>(a, a.O, N, ncu, nblk, kvg);
}
// causal (N % 256 == 0): one 256-row query block per workgroup, walking KV tiles 0 .. 4 b + 3; order 0 = longest block first, 1 = head-major
int launch_w4u_causal(const AttnPtrs& a, int BH, int N, int order, int kvg) {
  constexpr int D = W4U_D;
  const size_t nblk = (size_t)(N / 256) * BH;
  if (nblk > (size_t)INT_MAX) return LC_ERR_SHAPE;
  return launch_attn_kernel_kvg<W4U_IS_GQA>(W4U_CAUSAL_KERNEL<D, W4U_VT>, dim3((unsigned)nblk), dim3(256), W4U<D>::LDS, a.st, kvg, a.Q, a.K, a.V, a.O, N,
                                            N / 256, attn_scale_log2e(D), (int)nblk, order);
}
int slowpath_w4u(unsigned* out4, int reset) { return attn_slowpath_read(LC_AN_SLOWPATH_SYM, out4, reset); }
}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (a host object: the device pass would emit the constant and ask for device forms of the launchers)
const AttnW4uUnit W4U_CAT(g_attn_w4u_, W4U_TAG) = {W4U_D, W4U_VT, W4U_IS_GQA, launch_w4u, launch_w4u_causal, slowpath_w4u};
#endif
}  // namespace lc
