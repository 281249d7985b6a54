// tu_rope_append_varlen.hip — the fp16 ragged rotary-embedding + append kernels (rope_append_varlen_kernel<D, INTERLEAVED>,
// rope_append_varlen_kv8_kernel<D, INTERLEAVED>)
#include "tu_rope_append_varlen_impl.h"

namespace lc {
template int launch_rope_append_varlen<RopeVarlenUnit::F16>(const RopeAppendCall&, const RopeAppendPtrs&);
}  // namespace lc
