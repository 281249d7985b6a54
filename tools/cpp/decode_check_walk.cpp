// decode_check_walk.cpp — walks check_attn_decode (tu_plan.hip), the one check-and-plan function of the three decode-attention families, through
// their bad-argument cases with null and odd pointers, and asserts the status of each.  It launches nothing and needs no GPU, so it is the
// program to build with the host sanitizers (never load sanitized code into Python):
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/cpp/decode_check_walk.cpp leetcuda_amd/csrc/tu_plan.hip -o decode_check_walk && ./decode_check_walk
#include <stdio.h>

#include "../../leetcuda_amd/csrc/lc_plan.h"

namespace lc {   // what tu_plan.hip's HGEMM planner names in the kernel units; the decode path never reaches them
void valu_rung_tile(int, int*, int*, int*) {}
const char* valu_rung_kernel_name(int) { return ""; }
size_t launch_hgemm_mid_edge_sk_floats(int, int, int, int) { return 0; }
}  // namespace lc
using namespace lc;

static int g_bad = 0, g_seen = 0;
static void expect(int want, const DecodeCall& c, const DecodePtrs* a, const char* what) {
  DecodePlan p;
  const int got = check_attn_decode(c, a, &p);
  ++g_seen;
  if (got != want) {
    ++g_bad;
    fprintf(stderr, "%s (paged %d, kv_bytes %d): status %d, want %d\n", what, (int)c.paged, c.kv_bytes, got, want);
  }
}

static void set_ptr(DecodePtrs& a, int i, const void* v) {   // Q, K, V, O, block_table, kv_len
  switch (i) {
    case 0: a.Q = static_cast<const half_t*>(v); break;
    case 1: a.K = v; break;
    case 2: a.V = v; break;
    case 3: a.O = static_cast<half_t*>(const_cast<void*>(v)); break;
    case 4: a.block_table = static_cast<const int*>(v); break;
    default: a.kv_len = static_cast<const int*>(v);
  }
}

int main() {
  const half_t* q16 = reinterpret_cast<const half_t*>(16);
  half_t* o16 = reinterpret_cast<half_t*>(16);
  const void* p16 = reinterpret_cast<const void*>(16);
  const int* i16 = reinterpret_cast<const int*>(16);
  for (int fam = 0; fam < 3; ++fam) {   // contiguous, paged fp16, paged fp8
    const bool paged = fam > 0;
    const int kvb = fam == 2 ? 1 : 2;
    const DecodeCall ok = paged ? DecodeCall{1, 8, 2, 4, 128, 0, kvb, true, 0, 70, 16, 64} : DecodeCall{1, 8, 2, 4, 128, 0, 2, false, 1000, 0, 0, 0};
    const DecodePtrs good{q16, p16, p16, o16, paged ? i16 : nullptr, nullptr, paged ? i16 : nullptr, nullptr, nullptr};
    auto with = [&](auto edit) { DecodeCall c = ok; edit(c); return c; };
    for (const DecodePtrs* a : {&good, (const DecodePtrs*)nullptr}) {
      expect(LC_OK, ok, a, "the good call");
      expect(LC_OK, with([](DecodeCall& c) { c.flags = LC_ATTN_CAUSAL; }), a, "causal");
      for (int bad : {LC_ATTN_V_TRANSPOSED, 4, -1, 1 << 30})   // flags before everything: the shape and the head dim are bad too
        expect(LC_ERR_ARG, with([&](DecodeCall& c) { c.flags = bad; c.Hkv = 3; c.D = 256; }), a, "unknown flag");
      for (int hkv : {0, -1, 3, 5, 9, 16}) expect(LC_ERR_SHAPE, with([&](DecodeCall& c) { c.Hkv = hkv; c.D = 256; }), a, "head groups before head dim");
      expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.B = 0; }), a, "B");
      expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.H = c.Hkv = 0; }), a, "H");
      expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.Nq = 0; }), a, "Nq");
      expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.D = 0; }), a, "D = 0");
      expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.Nq = 17; c.D = 96; }), a, "R > 64 before head dim");
      expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.B = 1 << 24; c.H = c.Hkv = 8; c.Nq = 1; }), a, "the grid");
      if (paged) {
        for (int n : {0, -3}) expect(LC_ERR_SHAPE, with([&](DecodeCall& c) { c.num_pages = n; }), a, "num_pages");
        for (int n : {0, -1}) expect(LC_ERR_SHAPE, with([&](DecodeCall& c) { c.max_pages = n; }), a, "max_pages");
        for (int ps : {8, 24, 0, -16, 1, 48}) expect(LC_ERR_SHAPE, with([&](DecodeCall& c) { c.page_size = ps; c.D = 96; }), a, "page size before head dim");
        expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.page_size = 1 << 16; c.max_pages = 1 << 16; c.D = 64; }), a, "max_pages x page_size past an int");
        // the 2 GiB span counts BYTES: 2^30 elements of D = 128 rows refuse at two bytes, pass at one; twice that refuses at one
        expect(kvb == 2 ? LC_ERR_SHAPE : LC_OK, with([](DecodeCall& c) { c.max_pages = 1 << 19; }), a, "the span at 2^30 elements");
        expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.max_pages = 1 << 20; }), a, "the span at 2^31 elements");
        expect(LC_OK, with([](DecodeCall& c) { c.max_pages = (1 << 20) / c.kv_bytes - 1; }), a, "one page below the span");
      } else {
        for (int n : {0, -5}) expect(LC_ERR_SHAPE, with([&](DecodeCall& c) { c.Ncap = n; }), a, "Ncap");
        expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.Ncap = 1 << 23; }), a, "the span");
      }
      for (int d : {32, 96, 256, 512, 1024, 16, 48}) expect(LC_ERR_HEADDIM, with([&](DecodeCall& c) { c.D = d; }), a, "head dim");
    }
    // the run call's own pointers: a null one before shape and head dim, an odd one after the shape and before the head dim
    for (int i = 0; i < (paged ? 6 : 4); ++i) {
      DecodePtrs a = good;
      set_ptr(a, i, nullptr);
      expect(LC_ERR_ARG, ok, &a, "null pointer");
      expect(LC_ERR_ARG, with([](DecodeCall& c) { c.Hkv = 3; c.D = 256; }), &a, "null pointer before shape and head dim");
    }
    for (int i = 0; i < 4; ++i)
      for (unsigned long odd : {8ul, 1ul, 17ul}) {
        DecodePtrs a = good;
        set_ptr(a, i, reinterpret_cast<const void*>(odd));
        expect(LC_ERR_SHAPE, ok, &a, "odd pointer");
        expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.D = 96; }), &a, "odd pointer before head dim");
        expect(LC_ERR_SHAPE, with([](DecodeCall& c) { c.Nq = 0; }), &a, "shape with an odd pointer");
      }
    DecodePtrs scales = good;   // the scales are never looked at: null, odd, anything
    scales.k_scale = reinterpret_cast<const float*>(3);
    expect(LC_OK, ok, &scales, "an odd k_scale");
  }
  printf("decode_check_walk: %d cases, %d wrong\n", g_seen, g_bad);
  return g_bad ? 1 : 0;
}
