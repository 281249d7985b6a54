// tu_attn_w4u_gqa_d128.hip — translation unit of the grouped-query merged-phase attention kernels (attn_w4u_gqa.hip), D = 128, V as [B,Hkv,N,D] — see lc_launch.h
#define W4U_D 128
#define W4U_VT false
#define W4U_TAG gqa_d128
#define W4U_GQA 1
#include "tu_attn_w4u_impl.h"
