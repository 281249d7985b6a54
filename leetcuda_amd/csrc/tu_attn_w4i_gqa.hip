// tu_attn_w4i_gqa.hip — translation unit of the grouped-query forms of the generated merged-phase attention kernel (attn_w4i.hip with
// W4I_GQA: attn_fwd_w4i_gqa_kernel<D, SCHED>) — see lc_launch.h
#define LC_AN_SLOWPATH_SYM g_ag_slowpath_gqa
#define W4I_GQA 1
#include "tu_attn_w4i_impl.h"
