// tu_attn_w4u_gqa_d64.hip — translation unit of the grouped-query merged-phase attention kernels (attn_w4u_gqa.hip), D = 64, V as [B,Hkv,N,D] — see lc_launch.h
#define W4U_D 64
#define W4U_VT false
#define W4U_TAG gqa_d64
#define W4U_GQA 1
#include "tu_attn_w4u_impl.h"
