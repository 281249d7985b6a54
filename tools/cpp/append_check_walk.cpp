// append_check_walk.cpp — walks check_kv_append (tu_plan.hip), the one check of the two append-to-cache entries, through their bad-argument cases
// with null and odd pointers, and asserts the status of each; then format_kv_append into exact-fit and short buffers.  It launches nothing and
// needs no GPU, so it is the program to build with the host sanitizers (never load sanitized code into Python):
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/cpp/append_check_walk.cpp leetcuda_amd/csrc/tu_plan.hip -o append_check_walk && ./append_check_walk
#include <stdio.h>
#include <string.h>

#include "../../leetcuda_amd/csrc/lc_plan.h"

namespace lc {   // what tu_plan.hip's HGEMM planner names in the kernel units; the append path never reaches them
void valu_rung_tile(int, int*, int*, int*) {}
const char* valu_rung_kernel_name(int) { return ""; }
size_t launch_hgemm_mid_edge_sk_floats(int, int, int, int) { return 0; }
}  // namespace lc
using namespace lc;

static int g_bad = 0, g_seen = 0;
static void expect(int want, const AppendCall& c, const AppendPtrs* a, const char* what) {
  const int got = check_kv_append(c, a);
  ++g_seen;
  if (got != want) {
    ++g_bad;
    fprintf(stderr, "%s (kv_bytes %d): status %d, want %d\n", what, c.kv_bytes, got, want);
  }
}

static void set_ptr(AppendPtrs& a, int i, const void* v) {   // Knew, Vnew, Kpool, Vpool, block_table, kv_len
  switch (i) {
    case 0: a.Knew = static_cast<const half_t*>(v); break;
    case 1: a.Vnew = static_cast<const half_t*>(v); break;
    case 2: a.Kpool = const_cast<void*>(v); break;
    case 3: a.Vpool = const_cast<void*>(v); break;
    case 4: a.block_table = static_cast<const int*>(v); break;
    default: a.kv_len = static_cast<const int*>(v);
  }
}

int main() {
  const half_t* h16 = reinterpret_cast<const half_t*>(16);
  void* p16 = reinterpret_cast<void*>(16);
  const int* i16 = reinterpret_cast<const int*>(16);
  for (int kvb : {2, 1}) {   // fp16 pools, fp8 pools
    const AppendCall ok{2, 2, 4, 128, 0, kvb, 70, 16, 64};   // B, Hkv, Nq, D, flags, kv_bytes, num_pages, page_size, max_pages
    const AppendPtrs good{h16, h16, p16, p16, i16, i16, nullptr, nullptr, nullptr};
    auto with = [&](auto edit) { AppendCall c = ok; edit(c); return c; };
    for (const AppendPtrs* a : {&good, (const AppendPtrs*)nullptr}) {
      expect(LC_OK, ok, a, "the good call");
      for (int nq : {1, 64, 65, 4096, 0x7fffffff}) expect(LC_OK, with([&](AppendCall& c) { c.B = c.Hkv = 1; c.Nq = nq; }), a, "Nq is not bounded by 64");
      for (int bad : {1, 2, 4, -1, 1 << 30})   // no flag is defined; flags before everything: the shape and the head dim are bad too
        expect(LC_ERR_ARG, with([&](AppendCall& c) { c.flags = bad; c.Hkv = 0; c.D = 256; }), a, "a flag");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.B = 0; c.D = 96; }), a, "B before head dim");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.B = -1; }), a, "B");
      for (int n : {0, -2}) expect(LC_ERR_SHAPE, with([&](AppendCall& c) { c.Hkv = n; }), a, "Hkv");
      for (int n : {0, -4}) expect(LC_ERR_SHAPE, with([&](AppendCall& c) { c.Nq = n; }), a, "Nq");
      for (int n : {0, -3}) expect(LC_ERR_SHAPE, with([&](AppendCall& c) { c.num_pages = n; }), a, "num_pages");
      for (int n : {0, -1}) expect(LC_ERR_SHAPE, with([&](AppendCall& c) { c.max_pages = n; }), a, "max_pages");
      for (int n : {0, -128}) expect(LC_ERR_SHAPE, with([&](AppendCall& c) { c.D = n; }), a, "D");
      for (int ps : {8, 24, 0, -16, 1, 48, (int)0x80000000}) expect(LC_ERR_SHAPE, with([&](AppendCall& c) { c.page_size = ps; c.D = 96; }), a, "page size before head dim");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.page_size = 1 << 16; c.max_pages = 1 << 16; c.D = 64; }), a, "max_pages x page_size past an int");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.page_size = 1 << 30; c.max_pages = 0x7fffffff; c.D = 0x7fffffff; }), a, "the largest ints");
      // the 2 GiB span counts BYTES: 2^30 elements of D = 128 rows refuse at two bytes, pass at one; twice that refuses at one
      expect(kvb == 2 ? LC_ERR_SHAPE : LC_OK, with([](AppendCall& c) { c.max_pages = 1 << 19; }), a, "the span at 2^30 elements");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.max_pages = 1 << 20; }), a, "the span at 2^31 elements");
      expect(LC_OK, with([](AppendCall& c) { c.max_pages = (1 << 20) / c.kv_bytes - 1; }), a, "one page below the span");
      // the grid: B x Hkv x ceil(Nq / 16) workgroups at D = 128 (32 tokens a workgroup at D = 64)
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.B = c.Hkv = 1 << 16; c.Nq = 1; }), a, "B x Hkv past an int");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.B = 1 << 30; c.Hkv = 1; c.Nq = 17; }), a, "the grid at D = 128");
      expect(LC_OK, with([](AppendCall& c) { c.B = 1 << 30; c.Hkv = 1; c.Nq = 16; }), a, "the largest grid at D = 128");
      expect(LC_OK, with([](AppendCall& c) { c.B = 1 << 30; c.Hkv = 1; c.Nq = 32; c.D = 64; }), a, "the largest grid at D = 64");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.B = 1 << 30; c.Hkv = 1; c.Nq = 33; c.D = 64; }), a, "the grid at D = 64");
      expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.B = c.Hkv = c.Nq = 0x7fffffff; }), a, "the largest ints in the grid");
      for (int d : {32, 96, 256, 512, 1024, 16, 48, 8, 1, 0x7fffffff}) expect(d == 0x7fffffff ? LC_ERR_SHAPE : LC_ERR_HEADDIM, with([&](AppendCall& c) { c.D = d; }), a, "head dim");
    }
    // the run call's own pointers: a null one before shape and head dim, an odd one after the shape and before the head dim
    for (int i = 0; i < 6; ++i) {
      AppendPtrs a = good;
      set_ptr(a, i, nullptr);
      expect(LC_ERR_ARG, ok, &a, "null pointer");
      expect(LC_ERR_ARG, with([](AppendCall& c) { c.Hkv = 0; c.D = 256; }), &a, "null pointer before shape and head dim");
      expect(LC_ERR_ARG, with([](AppendCall& c) { c.flags = 1; }), &a, "a flag with a null pointer");
    }
    for (int i = 0; i < 4; ++i)
      for (unsigned long odd : {8ul, 1ul, 17ul}) {
        AppendPtrs a = good;
        set_ptr(a, i, reinterpret_cast<const void*>(odd));
        expect(LC_ERR_SHAPE, ok, &a, "odd pointer");
        expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.D = 96; }), &a, "odd pointer before head dim");
        expect(LC_ERR_SHAPE, with([](AppendCall& c) { c.Nq = 0; }), &a, "shape with an odd pointer");
      }
    for (int i = 4; i < 6; ++i) {   // the table and kv_len are int32 data: no 16-byte rule
      AppendPtrs a = good;
      set_ptr(a, i, reinterpret_cast<const void*>(4ul));
      expect(LC_OK, ok, &a, "a 4-byte aligned table / kv_len");
    }
    AppendPtrs scales = good;   // the scales are never looked at: null, odd, anything
    scales.k_scale = reinterpret_cast<const float*>(3);
    expect(LC_OK, ok, &scales, "an odd k_scale");
    // the name, into a buffer that fits exactly and into shorter ones (heap buffers: the sanitizer sees one byte too many)
    for (int d : {64, 128}) {
      char want[64];
      snprintf(want, sizeof want, kvb == 1 ? "kv_append_paged_kv8_kernel<%d>" : "kv_append_paged_kernel<%d>", d);
      for (int cut = 0; cut < 3; ++cut) {
        const int n = (int)strlen(want) + 1 - 4 * cut;
        char* buf = new char[n];
        format_kv_append(with([&](AppendCall& c) { c.D = d; }), buf, n);
        ++g_seen;
        if (strncmp(buf, want, n - 1) != 0 || buf[n - 1] != 0) {
          ++g_bad;
          fprintf(stderr, "name in %d bytes: \"%s\", want a prefix of \"%s\"\n", n, buf, want);
        }
        delete[] buf;
      }
    }
  }
  printf("append_check_walk: %d cases, %d wrong\n", g_seen, g_bad);
  return g_bad ? 1 : 0;
}
