// tu_attn_w4i.hip — translation unit of the generated merged-phase attention kernel (attn_w4i.hip: one generated hand-ordered asm
// statement per phase) — see lc_launch.h
#define LC_AN_SLOWPATH_SYM g_ag_slowpath
#include "tu_attn_w4i_impl.h"
