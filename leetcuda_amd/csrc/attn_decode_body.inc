// attn_decode_body.inc — the body of attn_decode_kernel<D, RT> (attn_decode.hip), of attn_decode_paged_kernel<D, RT> (attn_decode_paged.hip) and of
// attn_decode_paged_kv8_kernel<D, RT> (attn_decode_paged_kv8.hip), included textually by all three: the first two differ in how a key row becomes
// an address and in nothing else; the third (KV8, always PAGED) loads e4m3 bytes instead of halves, converts them to fp16 in registers in front of
// the two consumers and applies the per-head scales in fp32.  The including kernel has the template parameters D, RT, the parameters Q, K, V, O,
// kv_len, part_o, part_lse, H, Hkv, Nq, Ncap, causal, S, sl2, total_rows, a `constexpr bool PAGED` with a `const DecodePaging pg` (PAGED = false:
// unused) and a `constexpr bool KV8` with a `const DecodeKv8 kv8` (KV8 = false: unused) in scope.  See attn_decode.hip for the design.
// A `constexpr bool CHUNK` is in scope too.  CHUNK = false: the workgroup holds all R <= 64 rows of its (batch, K / V head).  CHUNK = true (the
// attn_chunk_*_kernel<D> of attn_chunk.hip, RT = 4; DESIGN.md §4.3i): R is unbounded, the grid has RB = ceil(R / 64) row blocks per (batch, K / V
// head), ((b Hkv + kvh) RB + rb) S + s, and this workgroup owns rows 64 rb ... of the [R, D] matrix; causal, it walks only the keys below L_blk,
// the largest limit of its rows.  With CHUNK = false the block offset `rbase` is the constant 0 and the walked length `Lw` is L_b: the nine
// decode kernels' code does not depend on the parameter (DESIGN.md §4.3i compares their assembly).
// A `constexpr bool LOCAL` with a `const DecodeLocal lc` (LOCAL = false: unused) is in scope as well.  LOCAL = true (the attn_local_*_kernel of
// attn_local.hip; DESIGN.md §4.3k): a sliding window of lc.window keys (0: none) — a lower limit next to the upper one lim[rt], and a first tile
// `tile_lo` next to the last one T: the workgroup walks tiles [tile_lo, T) and THOSE are cut into the S ranges — and an attention sink per query
// head (lc.sinks, nullptr: none): a logit that joins the row's softmax denominator and carries no value, the start of (m, l) in range 0, wave 0.
// With LOCAL = false tile_lo is the constant 0: the twelve decode and chunk kernels' code does not depend on the parameter (§4.3k compares it).
// A `constexpr bool VARLEN` with a `const DecodeVarlen vl` (VARLEN = false: unused) is the last one.  VARLEN = true (the attn_varlen_*_kernel of
// attn_varlen.hip; DESIGN.md §4.3l): Q and O are token-major [T, H, D] and sequence b owns the tokens q0 = clamp(cu_q[b], 0, T) ... q0 + Nq_b - 1,
// Nq_b = clamp(cu_q[b + 1] - q0, 0, min(Nq, T - q0)).  The argument Nq is then max_nq, the host's bound, and sizes the grid's RB only; every
// other use is the workgroup-uniform `Nqb` = Nq_b.  The row order inside a (sequence, K / V head) stays r = g Nq_b + i: only the ADDRESS of a row
// changes, global row (q0 + r % Nq_b) H + kvh G + r / Nq_b in place of row0 + r.  A workgroup whose row block starts at or past R_b returns in
// front of the first LDS access and barrier.  With VARLEN = false Nqb IS Nq: the 36 other kernels' code does not depend on the parameter.
// A `constexpr bool BF16` closes the list.  BF16 = true (the attn_varlen_*_bf16_kernel of attn_varlen.hip; DESIGN.md §4.3m): the 16-bit lanes
// of Q, O and a 16-bit cache are bfloat16.  Four places read them as numbers and only those change: the two MFMA sites (mfma16_16<BF16>), the
// rounding of P and of O (cvt16<BF16>, RNE), and the e4m3 -> 16-bit conversion of an fp8 cache (kv8_16x8<BF16>).  Loads, LDS images, transposed
// reads, masks, (m, l) and the partials do not know the element type.  With BF16 = false the three helpers ARE mfma16, (half_t)x and kv8_half8:
// every fp16 kernel's code is what it was without the parameter (§4.3m compares it).
// A `constexpr bool LSE` with a `const DecodeLse ls` (LSE = false: unused) is the newest.  LSE = true (the attn_varlen_*_lse*_kernel of
// attn_varlen.hip; DESIGN.md §4.3n): where wave 0 stores a row's O (S == 1) its h == 0 lanes also store the row's log-sum-exp in NATURAL
// units, ls.lse[row] with the global row of O and O's row guard.  The S > 1 path is untouched: part_lse always carried it, and the combine
// kernel of an LSE plan stores it.  With LSE = false nothing changes: every other kernel's code does not depend on the parameter (§4.3n compares it).
// A `constexpr bool TREE` with a `const DecodeTree tr` (TREE = false: unused) follows it.  TREE = true (the attn_varlen_*_tree*_kernel of
// attn_varlen.hip; DESIGN.md §4.3o): every query token carries a 64-bit look-back word, and key j of the row at slot p = lim - 1 is visible
// only if the compare below holds AND, for d = p - j < 64, bit d of the word is set; keys 64 or more slots back are not governed.  The mask only
// REMOVES keys: Lw, tile_lo, the range partition, the page ids and the source clamps do not know it.  A row's word sits in the padding of its
// Q row in LDS (no more LDS, no register across the loop), and a step whose every key lies 64 or more slots below the workgroup's lowest row
// slot takes the unmasked select through ONE wave-uniform branch per step: the scores and the softmax of a step are a text of their own
// (attn_decode_scores.inc) that a TREE kernel includes twice, with the bit test and without, so that either side of the branch stays one
// straight run of code (a branch per row tile cost the four-row-tile kernels 24 % on EVERY tile: hipcc no longer ran a row tile's MFMAs
// under the softmax of the one before).  With TREE = false the text is included once, where it stood: every other kernel's code does not
// depend on the parameter (§4.3o compares it).
  using L = DecodeLds<D, RT>;
  constexpr int KS = D / 32;    // k-steps of Sᵀ = K Qᵀ
  constexpr int DB = D / 16;    // 16-wide blocks of d
  constexpr int CH = D / 8;     // 16-byte chunks per row
  // keys per pipeline step: a wave walks its 64-key tiles in steps of 64 keys — of 32 where the accumulators of four row tiles at D = 128 leave
  // no room for a whole tile's K and V in flight (hipcc spilled; the audit's rule R2)
  constexpr int STEP = (D == 128 && RT == 4) ? 32 : 64;
  constexpr int SPT = DEC_KVB / STEP;     // steps per tile
  constexpr int NKB = STEP / 16;          // 16-key blocks of Sᵀ per step
  constexpr int NPS = STEP / 32;          // 32-key k-steps of Oᵀ += Vᵀ Pᵀ per step
  constexpr int VL = STEP * CH / 64;      // V chunks per lane and step
  // KV8: a cache element is one byte.  A lane's D / 4 contiguous elements of a key row are KR = D / 64 dwordx4, a 16-byte V chunk holds 16
  // elements of one key row (CHV per row, VLR per lane and step): half the registers in flight
  constexpr int ROWB = KV8 ? D : D * 2;   // bytes of a cache row
  constexpr int KR = KV8 ? KS / 2 : KS;
  constexpr int CHV = KV8 ? CH / 2 : CH;
  constexpr int VLR = KV8 ? VL / 2 : VL;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;
  // (integer division runs on the vector ALU: readfirstlane tells hipcc that the quotients are wave-uniform — scalar addressing, a scalar tile loop)
  const int bks = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)S)), s_idx = (int)blockIdx.x - bks * S;
  int bk = bks, rbase = 0;   // rbase: the first row of this workgroup's row block (CHUNK = false: 0, the only block)
  if constexpr (CHUNK) {
    const int RB = __builtin_amdgcn_readfirstlane(((H / Hkv) * Nq + 63) / 64);
    bk = __builtin_amdgcn_readfirstlane(bks / RB);
    rbase = 64 * (bks - bk * RB);
  }
  const int b = __builtin_amdgcn_readfirstlane(bk / Hkv), kvh = bk - b * Hkv;
  const int G = __builtin_amdgcn_readfirstlane(H / Hkv);
  int Nqb = Nq, q0 = 0;   // VARLEN: this sequence's tokens, clamped into the T rows whatever cu_q holds
  if constexpr (VARLEN) {
    const int c0 = __builtin_amdgcn_readfirstlane(vl.cu_q[b]), c1 = __builtin_amdgcn_readfirstlane(vl.cu_q[b + 1]);
    q0 = c0 < 0 ? 0 : (c0 > vl.T ? vl.T : c0);
    const int cap = Nq < vl.T - q0 ? Nq : vl.T - q0;
    Nqb = c1 <= q0 ? 0 : (c1 - q0 > cap ? cap : c1 - q0);   // (c1 > q0 >= 0: the difference does not wrap)
    if (rbase >= G * Nqb) return;   // no row of this sequence in the block (Nq_b = 0 included): nothing touched
  }
  const int R = G * Nqb;
  int Lb = kv_len ? kv_len[b] : Ncap;
  Lb = __builtin_amdgcn_readfirstlane(Lb);   // (a vector load of a uniform address: tell hipcc that the tile loop is wave-uniform)
  Lb = Lb < 0 ? 0 : (Lb > Ncap ? Ncap : Lb);
  // the keys this workgroup walks: all L_b — CHUNK and causal: those below L_blk = the limit of the row block's last token i_max (Nq - 1 where
  // the block straddles a head boundary); the tiles, the range partition and the source clamp follow it, the mask keeps using L_b
  int Lw = Lb;
  if constexpr (CHUNK) {
    if (causal) {
      const int span = (R - rbase < 64 ? R - rbase : 64) - 1;   // last row of the block - first
      const int i0 = __builtin_amdgcn_readfirstlane(rbase % Nqb);
      const int imax = i0 + span >= Nqb ? Nqb - 1 : i0 + span;
      const int v = Lb - Nqb + imax + 1;
      Lw = v < 0 ? 0 : (v > Lb ? Lb : v);
    }
  }
  const int T = (Lw + DEC_KVB - 1) / DEC_KVB;
  // LOCAL: the tile of the lowest key a row of this workgroup can see, Llo = max(0, L_b - Nq + i_min + 1 - W) with i_min the workgroup's lowest
  // token (0 unless a row block lies inside one head: then its first row's); nothing below tile_lo 64 is loaded, no table entry below it is read.
  // (Llo > 0 implies Llo < Lw: tile_lo < T)
  int tile_lo = 0;
  if constexpr (LOCAL) {
    if (lc.window > 0) {
      int imin = 0;
      if constexpr (CHUNK) {
        const int span = (R - rbase < 64 ? R - rbase : 64) - 1;
        const int i0 = __builtin_amdgcn_readfirstlane(rbase % Nqb);
        imin = i0 + span >= Nqb ? 0 : i0;
      }
      const long v = (long)Lb - Nqb + imin + 1 - lc.window;
      tile_lo = v > 0 ? (int)(v / DEC_KVB) : 0;
    }
  }
  const int Tw = T - tile_lo;   // tiles this workgroup walks (LOCAL = false: T)
  // (T < 2^24 tiles — one head's cache is below 2 GiB — and S <= 64: the products fit 32 bits)
  const int t0 = tile_lo + __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * Tw) / (unsigned)S));
  const int t1 = tile_lo + __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * Tw) / (unsigned)S));

  const long row0 = ((long)b * H + (long)kvh * G) * Nq;   // the R rows of this (batch, K / V head): one contiguous [R, D] matrix
  const half_t* Qg = Q + row0 * D;
  // VARLEN: the global row of row r of this (sequence, K / V head) in the token-major [T, H, D] buffers (q0 + i < T: the clamps above)
  auto vrow = [&](int r) {
    const int g = r / Nqb;
    return (long)(q0 + (r - g * Nqb)) * H + kvh * G + g;
  };
  // (PAGED: K / V are the pools; the base of a load group is that of its page, below)
  const half_t* Kg = PAGED ? K : K + ((long)b * Hkv + kvh) * (long)Ncap * D;
  const half_t* Vg = PAGED ? V : V + ((long)b * Hkv + kvh) * (long)Ncap * D;

  // ---- Q -> LDS (rows >= R: row R - 1)
  for (int c = tid; c < 16 * RT * CH; c += 256) {
    const int r = c / CH, ch = c % CH;
    const int rs = rbase + r < R ? rbase + r : R - 1;
    if constexpr (VARLEN)
      *reinterpret_cast<u32x4_t*>(lds + r * L::kQStride + ch * 16) = *reinterpret_cast<const u32x4_t*>(Q + vrow(rs) * D + ch * 8);
    else
      *reinterpret_cast<u32x4_t*>(lds + r * L::kQStride + ch * 16) = *reinterpret_cast<const u32x4_t*>(Qg + (long)rs * D + ch * 8);
    // TREE: the row's look-back word travels with its Q row, in the first 8 of the row's 16 padding bytes (token q0 + rs % Nqb < T: the clamps
    // above; padding rows take row R - 1's, as they take its Q).  No register holds a word across the steps that do not test it
    if constexpr (TREE) {
      if (ch == 0) *reinterpret_cast<uint64_t*>(lds + r * L::kQStride + D * 2) = tr.mask[q0 + rs % Nqb];
    }
  }
  __syncthreads();

  // visible keys of this lane's query row in each row tile: keys j < lim
  int lim[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    int r = rbase + 16 * rt + i16;
    r = r < R ? r : R - 1;
    int v = causal ? Lb - Nqb + (r % Nqb) + 1 : Lb;
    lim[rt] = v < 0 ? 0 : v;
  }
  // LOCAL: key j is visible to a row iff lim - W <= j < lim, one unsigned compare of j - lim + W against W; no window is the widest one
  // (j - lim >= -(2^31 - 1): the sum does not wrap below 0)
  const unsigned wlo = LOCAL && lc.window > 0 ? (unsigned)lc.window : 0x7fffffffu;
  // TREE: the lowest key ANY row of the workgroup has a bit for: tree_lo = p_min - 63 with p_min the slot of the workgroup's lowest token (i_min
  // as for LOCAL: 0 unless a row block lies inside one head).  A step below it does not look at the words
  int tree_lo = 0;
  if constexpr (TREE) {
    int imin = 0;
    if constexpr (CHUNK) {
      const int span = (R - rbase < 64 ? R - rbase : 64) - 1;
      const int i0 = __builtin_amdgcn_readfirstlane(rbase % Nqb);
      imin = i0 + span >= Nqb ? 0 : i0;
    }
    tree_lo = Lb - Nqb + imin - 63;
  }

  float m[RT], l[RT];
  f32x4_t o[RT][DB];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    m[rt] = DEC_NEG_INF;
    l[rt] = 0.f;
#pragma unroll
    for (int db = 0; db < DB; ++db) o[rt][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // LOCAL: the sink of the row's query head is one more score of the row, without a value: the running maximum starts at it (natural units,
  // not scaled by 1 / sqrt(D): x log2 e only) and the running sum at exp2(0) = 1, in ONE lane group of ONE wave of ONE range; the wave merge,
  // the partial's log-sum-exp and the combine kernel then see a wave that has met one key.  (-inf: l = 1 meets exp2(-inf) = 0 wherever it is
  // used.)  Padding rows take row R - 1's head, as they take its Q.
  if constexpr (LOCAL) {
    if (lc.sinks && s_idx == 0 && w == 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        int r = rbase + 16 * rt + i16;
        r = r < R ? r : R - 1;
        m[rt] = lc.sinks[kvh * G + r / Nqb] * 1.4426950408889634f;
        l[rt] = h == 0 ? 1.f : 0.f;
      }
    }
  }

  char* vimg = lds + L::kVOff + w * L::kVBytes;
  // transposed-read address of this lane inside a 32-key k-step: row 4 h + q (+ 16 for the second half), d = 16 db + 4 p
  const int q4 = i16 >> 2, p4 = i16 & 3;
  int tr_off[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) tr_off[db] = dec_v_off<D>(4 * h + q4, 2 * db + (p4 >> 1)) + 8 * (p4 & 1);

  u32x4_t kf[NKB][KR], vf[VLR];
  const int last = Lw - 1;   // (>= 0 whenever a tile exists)
  // step u of this wave: keys key0(u) ... key0(u) + STEP - 1 of tile t0 + w + 4 (u / SPT)
  auto key0 = [&](int u) { return (t0 + w + DEC_WAVES * (u / SPT)) * DEC_KVB + (u % SPT) * STEP; };
  // PAGED: the pool page of each 16-key block of a step.  A block's keys share a page (page_size % 16 == 0), and so do the 4 or 8 key rows of a
  // V chunk group with their block; the clamp to `last` keeps that true (keys past it collapse onto one row, inside last's own block), and it
  // keeps the table index below ceil(L_b / page_size).  Ids are clamped to the pool: a garbage entry reads a wrong page, never outside the pool.
  // readfirstlane: table reads are scalar loads, page bases live in SGPRs (per-lane 64-bit addresses would not fit <128,4>'s register file)
  int pid[PAGED ? NKB : 1];
  auto page_ids = [&](int u) {
    const int k0 = key0(u);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      int first = k0 + 16 * kb;
      first = first < last ? first : last;
      int id = __builtin_amdgcn_readfirstlane(pg.table[(long)b * pg.max_pages + (first >> pg.lps)]);
      id = id < 0 ? 0 : id;
      pid[kb] = id < pg.num_pages ? id : pg.num_pages - 1;
    }
  };
  // byte base of (page id, this K / V head): 64-bit, scalar; the offset inside the run is 32-bit (one run is below 2 GiB: checked by the host)
  auto page_base = [&](const half_t* pool, int id) {
    return reinterpret_cast<const char*>(pool) + ((((long)id * Hkv + kvh) << pg.lps) * ROWB);
  };
  const int pmask = PAGED ? (1 << pg.lps) - 1 : -1;
  auto load_k = [&](int u) {
    const int k0 = key0(u);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      int key = k0 + 16 * kb + i16;
      key = key < last ? key : last;
      if constexpr (KV8) {   // bytes h D / 4 ... of the row; k-step s is bytes 8 s ... 8 s + 7 of them (k_frag)
        const char* base = page_base(Kg, pid[kb]);
        const unsigned off = (unsigned)(key & pmask) * ROWB + h * (D / 4);
#pragma unroll
        for (int s = 0; s < KR; ++s) kf[kb][s] = *reinterpret_cast<const u32x4_t*>(base + (off + 16 * s));
      } else if constexpr (PAGED) {
        const char* base = page_base(Kg, pid[kb]);
        const unsigned off = (unsigned)(key & pmask) * (D * 2) + h * (D / 2);
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[kb][s] = *reinterpret_cast<const u32x4_t*>(base + (off + 16 * s));
      } else {
        const unsigned off = (unsigned)key * (D * 2) + h * (D / 2);   // bytes inside the head: < 2 GiB (checked by the host), base in SGPRs
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[kb][s] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(Kg) + (off + 16 * s));
      }
    }
  };
  auto load_v = [&](int u) {
    const int k0 = key0(u);
#pragma unroll
    for (int n = 0; n < VLR; ++n) {
      const int c = n * 64 + lane;
      int key = k0 + c / CHV;
      key = key < last ? key : last;
      if constexpr (KV8)   // (chunk group n: the 64 / CHV = 8 or 16 key rows from k0 + n 64 / CHV on, inside 16-key block n 4 / CHV)
        vf[n] = *reinterpret_cast<const u32x4_t*>(page_base(Vg, pid[n * 4 / CHV]) + ((unsigned)(key & pmask) * ROWB + (c % CHV) * 16));
      else if constexpr (PAGED)   // (chunk group n: the 64 / CH key rows from k0 + n 64 / CH on, inside 16-key block n 4 / CH)
        vf[n] = *reinterpret_cast<const u32x4_t*>(page_base(Vg, pid[n * 4 / CH]) + ((unsigned)(key & pmask) * (D * 2) + (c % CH) * 16));
      else
        vf[n] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(Vg) + ((unsigned)key * (D * 2) + (c % CH) * 16));
    }
  };
  auto store_v = [&]() {
#pragma unroll
    for (int n = 0; n < VLR; ++n) {
      const int c = n * 64 + lane;
      if constexpr (KV8) {   // one e4m3 chunk is the two adjacent fp16 chunks 2 (c % CHV), + 1 of its row: the image is the fp16 kernels'
        *reinterpret_cast<u32x4_t*>(vimg + dec_v_off<D>(c / CHV, 2 * (c % CHV))) = kv8_16x8<BF16>(vf[n][0], vf[n][1]);
        *reinterpret_cast<u32x4_t*>(vimg + dec_v_off<D>(c / CHV, 2 * (c % CHV) + 1)) = kv8_16x8<BF16>(vf[n][2], vf[n][3]);
      } else {
        *reinterpret_cast<u32x4_t*>(vimg + dec_v_off<D>(c / CH, c % CH)) = vf[n];
      }
    }
  };
  // the A operand of k-step s of 16-key block kb
  auto k_frag = [&](int kb, int s) {
    if constexpr (KV8) return __builtin_bit_cast(half8_t, kv8_16x8<BF16>(kf[kb][s >> 1][2 * (s & 1)], kf[kb][s >> 1][2 * (s & 1) + 1]));
    else return __builtin_bit_cast(half8_t, kf[kb][s]);
  };
  // KV8: the scales of this K / V head, fp32 only: k_scale goes once into the score scale, v_scale into the normalisation of O
  float sc2 = sl2, vsc = 1.f;
  if constexpr (KV8) {
    if (kv8.k_scale) sc2 *= __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, kv8.k_scale[kvh])));
    if (kv8.v_scale) vsc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, kv8.v_scale[kvh])));
  }

  const int my_tiles = t1 - t0 - w > 0 ? (t1 - t0 - w + DEC_WAVES - 1) / DEC_WAVES : 0;
  const int steps = my_tiles * SPT;
  if (steps > 0) {
    if constexpr (PAGED) page_ids(0);
    load_k(0);
    load_v(0);
    if constexpr (PAGED) page_ids(1);   // (a step past the last one names the page of key L_b - 1: always a valid table position)
    store_v();
  }
  for (int u = 0; u < steps; ++u) {
    // ---- Sᵀ = K Qᵀ for this tile (the K registers are free behind it)
    // and the online softmax (log2 domain) of each row tile right behind its scores: Sᵀ -> P in fp16 (BF16: bf16), register for register the B operand of
    // Oᵀ += Vᵀ Pᵀ (16 score registers per lane alive at a time, not 16 RT)
    const int k0 = key0(u) + 4 * h;
    half8_t pf[RT][NPS];
    float alpha[RT];
    // (the scores and the softmax of the step: attn_decode_scores.inc, included with a `constexpr bool MASKED` in scope.  TREE: ONE wave-uniform
    // branch per step picks the text with the bit test or the text without it, each one straight run of code; every other kernel includes
    // the text without it once, where the loop always stood)
    if constexpr (TREE) {
      if (key0(u) + STEP - 1 >= tree_lo) {   // some row of the workgroup has a bit for a key of the step
        constexpr bool MASKED = true;
#include "attn_decode_scores.inc"
      } else {
        constexpr bool MASKED = false;
#include "attn_decode_scores.inc"
      }
    } else {
      constexpr bool MASKED = false;
#include "attn_decode_scores.inc"
    }
    // ---- the next tile's K and V loads into the registers that are free now: a whole tile in flight under the rest of the arithmetic (the
    // scheduling barrier keeps hipcc from hoisting them over the scores: that is what keeps the four-row-tile kernel inside the register file)
    __builtin_amdgcn_sched_barrier(0);
    const bool more = u + 1 < steps;
    if (more) load_k(u + 1);
    if (more) load_v(u + 1);
    // PAGED: the table entries of step u + 2, read one iteration before the loads that need them: no K / V load waits for a table load
    if constexpr (PAGED) page_ids(u + 2);
    // ---- rescale O only when some row's maximum moved (a multiplication by exactly 1 otherwise: same bits).  A block of its own, so that the
    // accumulators stay where the MFMAs below want them instead of travelling through the vector ALU on every tile
    bool moved = false;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) moved |= alpha[rt] != 1.f;
    if (__builtin_amdgcn_ballot_w64(moved) != 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int db = 0; db < DB; ++db) o[rt][db] *= alpha[rt];
    }
    // ---- Oᵀ += Vᵀ Pᵀ: the Vᵀ fragments of a 16-wide block of d out of the image serve every row tile
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      half8_t va[NPS];
#pragma unroll
      for (int s = 0; s < NPS; ++s) va[s] = cat4(lds_tr16(vimg + (D * 2) * (32 * s) + tr_off[db]), lds_tr16(vimg + (D * 2) * (32 * s + 16) + tr_off[db]));
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int s = 0; s < NPS; ++s) o[rt][db] = mfma16_16<BF16>(va[s], pf[rt][s], o[rt][db]);
    }
    if (more) store_v();   // (LDS operations of one wave execute in order: the transposed reads above are behind us)
  }

  // ---- merge the four waves' (m, l, O)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    l[rt] += __shfl_xor(l[rt], 16);
    l[rt] += __shfl_xor(l[rt], 32);
  }
  float* ml = reinterpret_cast<float*>(lds + L::kMlOff);
  if (h == 0) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      ml[w * 16 * RT + 16 * rt + i16] = m[rt];
      ml[(DEC_WAVES + w) * 16 * RT + 16 * rt + i16] = l[rt];
    }
  }
  __syncthreads();   // every wave is out of its key loop: the V images are free
  float lt[RT], mt[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float mm = DEC_NEG_INF;
#pragma unroll
    for (int x = 0; x < DEC_WAVES; ++x) mm = fmaxf(mm, ml[x * 16 * RT + 16 * rt + i16]);
    const float mu = (mm == DEC_NEG_INF) ? 0.f : mm;
    float ls = 0.f;
#pragma unroll
    for (int x = 0; x < DEC_WAVES; ++x) ls += ml[(DEC_WAVES + x) * 16 * RT + 16 * rt + i16] * __builtin_amdgcn_exp2f(ml[x * 16 * RT + 16 * rt + i16] - mu);
    const float mine = __builtin_amdgcn_exp2f(m[rt] - mu);
#pragma unroll
    for (int db = 0; db < DB; ++db) o[rt][db] *= mine;
    lt[rt] = ls;
    mt[rt] = mm;
  }
  f32x4_t* slot = reinterpret_cast<f32x4_t*>(lds + L::kVOff);
  constexpr int SLOT = L::kOBytes / 16;   // f32x4 per slot
  auto put = [&](int sl) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int db = 0; db < DB; ++db) slot[sl * SLOT + (rt * DB + db) * 64 + lane] = o[rt][db];
  };
  auto add = [&](int sl) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int db = 0; db < DB; ++db) o[rt][db] += slot[sl * SLOT + (rt * DB + db) * 64 + lane];
  };
  if (w >= 2) put(w - 2);
  __syncthreads();
  if (w < 2) add(w);
  __syncthreads();
  if (w == 1) put(0);
  __syncthreads();
  if (w != 0) return;
  add(0);

  // ---- wave 0 writes: fp16 (BF16: bf16) O (S == 1) or the normalised fp32 partial + the row's log2-domain log-sum-exp
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = rbase + 16 * rt + i16;
    if (r >= R) continue;   // padding rows store nothing
    float inv = lt[rt] > 0.f ? 1.f / lt[rt] : 0.f;
    if constexpr (KV8) inv *= vsc;
    long row = row0 + r;
    if constexpr (VARLEN) row = vrow(r);
    if (S == 1) {
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const f32x4_t x = o[rt][db] * inv;
        half4_t y = {cvt16<BF16>(x[0]), cvt16<BF16>(x[1]), cvt16<BF16>(x[2]), cvt16<BF16>(x[3])};
        *reinterpret_cast<half4_t*>(O + row * D + 16 * db + 4 * h) = y;
      }
      if constexpr (LSE) {   // (m in the log2 domain -> natural log: what a caller's merge of two results wants)
        if (h == 0) ls.lse[row] = lt[rt] > 0.f ? (mt[rt] + log2f(lt[rt])) * 0.6931471805599453f : DEC_NEG_INF;
      }
    } else {
      float* po = part_o + ((long)s_idx * total_rows + row) * D;
#pragma unroll
      for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4_t*>(po + 16 * db + 4 * h) = o[rt][db] * inv;
      if (h == 0) part_lse[(long)s_idx * total_rows + row] = lt[rt] > 0.f ? mt[rt] + log2f(lt[rt]) : DEC_NEG_INF;
    }
  }
