// tu_attn_w4u_gqa_d64t.hip — translation unit of the grouped-query merged-phase attention kernels (attn_w4u_gqa.hip), D = 64, V as [B,Hkv,D,N] — see lc_launch.h
#define W4U_D 64
#define W4U_VT true
#define W4U_TAG gqa_d64t
#define W4U_GQA 1
#include "tu_attn_w4u_impl.h"
