// tu_rope_append_varlen_pos.hip — the ragged rotary-embedding + append kernels with per-token rotary positions, fp16 and bfloat16
// (rope_append_varlen_pos_kernel<D, INTERLEAVED>, _pos_kv8_kernel, _pos_bf16_kernel, _pos_kv8_bf16_kernel)
#include "tu_rope_append_varlen_impl.h"

namespace lc {
template int launch_rope_append_varlen<RopeVarlenUnit::POS>(const RopeAppendCall&, const RopeAppendPtrs&);
}  // namespace lc
