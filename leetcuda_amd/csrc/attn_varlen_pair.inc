// attn_varlen_pair.inc — the two range kernels of ONE variant of the ragged family, included by attn_varlen.hip once per variant behind
//   #define LC_VARLEN_PAIR  <the <D, RT> kernel>, <the <D> chunk kernel>, KV8, BF16, LSE, TREE
// (a file and not a macro: each kernel is the shared body, attn_decode_body.inc, included textually).  The pair has one argument list and one
// set of flags by construction; VarlenKernels<KV8, BF16, LSE, TREE> hands both kernels to the launcher.
template <int D, int RT>
__global__ __launch_bounds__(256) void LC_VARLEN_APPLY(LC_VARLEN_RANGES_, LC_VARLEN_PAIR)(LC_VARLEN_APPLY(LC_VARLEN_SIGNATURE_, LC_VARLEN_PAIR)) {
  constexpr bool CHUNK = false;
  LC_VARLEN_APPLY(LC_VARLEN_COMMON_, LC_VARLEN_PAIR)
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void LC_VARLEN_APPLY(LC_VARLEN_CHUNK_, LC_VARLEN_PAIR)(LC_VARLEN_APPLY(LC_VARLEN_SIGNATURE_, LC_VARLEN_PAIR)) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  LC_VARLEN_APPLY(LC_VARLEN_COMMON_, LC_VARLEN_PAIR)
#include "attn_decode_body.inc"
}

template <>
struct VarlenKernels<LC_VARLEN_APPLY(LC_VARLEN_FLAGS_, LC_VARLEN_PAIR)> {
  template <int D, int RT>
  static auto ranges() { return LC_VARLEN_APPLY(LC_VARLEN_RANGES_, LC_VARLEN_PAIR)<D, RT>; }
  template <int D>
  static auto chunk() { return LC_VARLEN_APPLY(LC_VARLEN_CHUNK_, LC_VARLEN_PAIR)<D>; }
};
#undef LC_VARLEN_PAIR
