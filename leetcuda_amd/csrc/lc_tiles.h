// lc_tiles.h — the tile sizes that both the kernels and the host-side launch rules (lc_plan.h) reason with, defined once.
#pragma once

namespace lc {

constexpr int BM = 256, BN = 256, BK = 64;   // hgemm_mfma256.hip and the 4-wave 256-tile kernels
constexpr int BM1 = 128, BN1 = 128;          // hgemm_mfma128.hip
constexpr int KVB = 64;  // kv rows per tile (attn_fwd.hip and the merged-phase kernels)

}  // namespace lc
