// tu_attn_varlen_paged_kv8_tree.hip — the fp16 ragged-batch kernels over the fp8 paged cache with a look-back visibility mask per query token
// (attn_varlen_paged_kv8_tree_kernel<D, RT>, attn_varlen_chunk_paged_kv8_tree_kernel<D>).  The combine kernel is
// tu_attn_varlen_paged_lse.hip's
#define VARLEN_CACHE DecodeCache::PAGED_KV8
#define VARLEN_BF16 false
#define VARLEN_OUT VarlenOut::TREE
#include "tu_attn_varlen_impl.h"
