// tu_rope_append_varlen_bf16.hip — the bfloat16 ragged rotary-embedding + append kernels (rope_append_varlen_bf16_kernel<D, INTERLEAVED>,
// rope_append_varlen_kv8_bf16_kernel<D, INTERLEAVED>)
#include "tu_rope_append_varlen_impl.h"

namespace lc {
template int launch_rope_append_varlen<RopeVarlenUnit::BF16>(const RopeAppendCall&, const RopeAppendPtrs&);
}  // namespace lc
