// gemm_plan_walk.cpp — walks the two GEMM planning rules of tu_plan.hip that the C entry points used to hold: plan_gemm_fp8 / check_gemm_fp8 (which fp8
// kernel a call of lc_gemm_fp8_e4m3 / lc_gemm_mxfp8 runs under every "fp8_mx" value and on both sides of the 32-bit DMA offset bound; the status of
// every bad call, in the order the entries rank them; the tiles and the panel width of a plan) and hgemm_entry_variant (which variant a reference
// entry name of lc_hgemm_call runs on a shape).  Every rule is handed a knob snapshot with "rule_cus" = 256: it launches nothing and needs no GPU,
// so it is the program to build with the host sanitizers (never load sanitized code into Python):
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/cpp/gemm_plan_walk.cpp leetcuda_amd/csrc/tu_plan.hip -o gemm_plan_walk && ./gemm_plan_walk
#include <stdio.h>

#include "../../leetcuda_amd/csrc/lc_plan.h"

namespace lc {   // what tu_plan.hip's HGEMM planner names in the kernel units; no rule walked here reads them
void valu_rung_tile(int, int* tm, int* tn, int* tk) { *tm = *tn = *tk = 1; }
const char* valu_rung_kernel_name(int) { return ""; }
size_t launch_hgemm_mid_edge_sk_floats(int, int, int, int) { return 0; }
}  // namespace lc
using namespace lc;

static int g_bad = 0, g_seen = 0;
static void expect_eq(long got, long want, const char* what, long a = 0, long b = 0, long c = 0) {
  ++g_seen;
  if (got != want) {
    ++g_bad;
    fprintf(stderr, "%s (%ld, %ld, %ld): %ld, want %ld\n", what, a, b, c, got, want);
  }
}

constexpr int kLastFit = 8259456, kFirstBig = 8259584;   // multiples of 128 on either side of K x 260 = 2^31

// plan_gemm_fp8: the kernel of every (entry, "fp8_mx", K) and the plan's tiles and panel width, on one snapshot
static void walk_fp8_plan() {
  for (int knob : {3, 1, 2, 0})
    for (bool mx : {false, true})
      for (int K : {128, kLastFit, kFirstBig})
        for (int raster : {0, 1, 2})
          for (int stride : {1, 512, 2048}) {
            Knobs k = read_knobs();
            k.rule_cus = 256;
            k.fp8_mx = knob;
            k.hgemm_raster = raster;
            const bool fits = K != kFirstBig;
            const int M = mx ? 768 : 512, N = mx ? 768 : 1024;
            GemmFp8Plan p{};
            const int rc = plan_gemm_fp8(k, GemmFp8Call{M, N, K, stride, mx}, &p);
            expect_eq(rc, mx && !fits ? LC_ERR_SHAPE : LC_OK, "status of the fp8 plan", knob, mx, K);
            if (rc != LC_OK) continue;
            const Fp8Kern want = mx ? Fp8Kern::W4K_MX
                                 : knob == 0 ? Fp8Kern::PINGPONG2
                                 : knob == 2 || !fits ? Fp8Kern::PINGPONG2_MX
                                 : knob == 3 ? Fp8Kern::W4K : Fp8Kern::W4;
            expect_eq((int)p.kern, (int)want, "kernel of the fp8 plan", knob, mx, K);
            expect_eq(p.tiles_m, M / 256, "tiles_m", knob, mx, K);
            expect_eq(p.tiles_n, N / 256, "tiles_n", knob, mx, K);
            expect_eq(p.panel_w, panel_tiles(raster, stride, N / 256, 256, ((size_t)M + N) * K), "panel width", raster, stride, K);
            expect_eq(p.call.M == M && p.call.N == N && p.call.K == K && p.call.swizzle_stride == stride && p.call.mx == mx, 1, "the plan's call", knob, mx, K);
          }
  // the rows of the table once more, spelled out (not derived from the rule's own shape)
  struct Row { bool mx; int knob; int K; int want; };   // want: Fp8Kern, or -1 = LC_ERR_SHAPE
  const Row rows[] = {{false, 3, 128, (int)Fp8Kern::W4K},          {false, 3, kLastFit, (int)Fp8Kern::W4K},          {false, 3, kFirstBig, (int)Fp8Kern::PINGPONG2_MX},
                      {false, 1, 128, (int)Fp8Kern::W4},           {false, 1, kLastFit, (int)Fp8Kern::W4},           {false, 1, kFirstBig, (int)Fp8Kern::PINGPONG2_MX},
                      {false, 2, 128, (int)Fp8Kern::PINGPONG2_MX}, {false, 2, kLastFit, (int)Fp8Kern::PINGPONG2_MX}, {false, 2, kFirstBig, (int)Fp8Kern::PINGPONG2_MX},
                      {false, 0, 128, (int)Fp8Kern::PINGPONG2},    {false, 0, kLastFit, (int)Fp8Kern::PINGPONG2},    {false, 0, kFirstBig, (int)Fp8Kern::PINGPONG2},
                      {true, 3, 128, (int)Fp8Kern::W4K_MX},        {true, 3, kLastFit, (int)Fp8Kern::W4K_MX},        {true, 3, kFirstBig, -1},
                      {true, 1, 128, (int)Fp8Kern::W4K_MX},        {true, 1, kLastFit, (int)Fp8Kern::W4K_MX},        {true, 1, kFirstBig, -1},
                      {true, 2, 128, (int)Fp8Kern::W4K_MX},        {true, 2, kLastFit, (int)Fp8Kern::W4K_MX},        {true, 2, kFirstBig, -1},
                      {true, 0, 128, (int)Fp8Kern::W4K_MX},        {true, 0, kLastFit, (int)Fp8Kern::W4K_MX},        {true, 0, kFirstBig, -1}};
  for (const Row& r : rows) {
    Knobs k = read_knobs();
    k.rule_cus = 256;
    k.fp8_mx = r.knob;
    GemmFp8Plan p{};
    const int rc = plan_gemm_fp8(k, GemmFp8Call{256, 256, r.K, 1, r.mx}, &p);
    expect_eq(rc == LC_OK ? (int)p.kern : rc == LC_ERR_SHAPE ? -1 : -2, r.want, "row of the fp8 table", r.knob, r.mx, r.K);
  }
  // the bound itself, at one byte and at two bytes an element
  expect_eq(w4_rows_fit(8259552, 1), 1, "the last K that fits, fp8");
  expect_eq(w4_rows_fit(8259553, 1), 0, "the first K that does not, fp8");
  expect_eq(w4_rows_fit(4129776, 2), 1, "the last K that fits, fp16");
  expect_eq(w4_rows_fit(4129777, 2), 0, "the first K that does not, fp16");
}

// check_gemm_fp8 (and check_mx_pack_scales): the statuses of tests/test_abi_cpu.py::test_fp8_entry_points_refuse_bad_arguments, in its order
struct Fp8Args {
  const void *a, *pa, *b, *pb, *c;
  int m, n, k;
};
static int check(bool mx, const Fp8Args& x, bool with_ptrs = true) {
  const GemmFp8Ptrs ptrs{static_cast<const uint8_t*>(x.a), static_cast<const uint8_t*>(x.b), static_cast<half_t*>(const_cast<void*>(x.c)),
                         static_cast<const uint32_t*>(mx ? x.pa : nullptr), static_cast<const uint32_t*>(mx ? x.pb : nullptr), 1.0f, nullptr};
  GemmFp8Plan p{};
  return check_gemm_fp8(GemmFp8Call{x.m, x.n, x.k, 1, mx}, with_ptrs ? &ptrs : nullptr, &p);
}
static const void** ptr_of(Fp8Args& x, int i) { return i == 0 ? &x.a : i == 1 ? &x.b : i == 2 ? &x.c : i == 3 ? &x.pa : &x.pb; }
static int* dim_of(Fp8Args& x, int i) { return i == 0 ? &x.m : i == 1 ? &x.n : &x.k; }

static void walk_fp8_checks() {
  const void* p = reinterpret_cast<const void*>(4096);   // 16-byte aligned, never dereferenced
  const Fp8Args ok{p, p, p, p, p, 512, 768, 384};
  const int kbig = (int)(((((1ll << 31) + 259) / 260 + 127) / 128) * 128);
  expect_eq(kbig, kFirstBig, "the first K beyond the bound");
  for (bool mx : {false, true}) {
    const int nptr = mx ? 5 : 3;
    expect_eq(check(mx, ok), LC_OK, "the good call", mx);
    expect_eq(check(mx, ok, false), LC_OK, "the good call without pointers", mx);
    // each null pointer, before any shape check (second pass: a dim is bad too; third: everything else is)
    for (int pass = 0; pass < 3; ++pass)
      for (int i = 0; i < nptr; ++i) {
        Fp8Args x = ok;
        *ptr_of(x, i) = nullptr;
        if (pass >= 1) x.m = 0;
        if (pass == 2) { x.n = 255; x.k = kbig + 1; *ptr_of(x, (i + 1) % 3) = reinterpret_cast<const void*>(4097); }
        expect_eq(check(mx, x), LC_ERR_ARG, "null pointer", mx, i, pass);
        expect_eq(check(mx, x, false), pass == 0 ? LC_OK : LC_ERR_SHAPE, "no pointers: the shape alone", mx, i, pass);
      }
    if (!mx) {   // the unit-scale entry never looks at PA / PB
      Fp8Args x = ok;
      x.pa = x.pb = nullptr;
      expect_eq(check(false, x), LC_OK, "PA / PB of the unit-scale entry");
    }
    // non-positive dims; M, N off the 256 x 256 tile; K off the 128-deep K tile
    for (int d = 0; d < 3; ++d)
      for (int v : {0, -256, -1}) {
        Fp8Args x = ok;
        *dim_of(x, d) = v;
        expect_eq(check(mx, x), LC_ERR_SHAPE, "non-positive dim", mx, d, v);
        x.a = reinterpret_cast<const void*>(4100);   // ... and an odd pointer: the same status
        expect_eq(check(mx, x), LC_ERR_SHAPE, "non-positive dim with an odd pointer", mx, d, v);
      }
    for (int d = 0; d < 2; ++d)
      for (int v : {128, 255, 257, 384, 256 * 3 + 16}) {
        Fp8Args x = ok;
        *dim_of(x, d) = v;
        expect_eq(check(mx, x), LC_ERR_SHAPE, "M / N off the tile", mx, d, v);
        x.k = kbig;   // ... and K beyond the bound (unit scales: a legal K): the same status
        expect_eq(check(mx, x), LC_ERR_SHAPE, "M / N off the tile with a long K", mx, d, v);
      }
    for (int v : {32, 64, 96, 127, 129, 192, 128 * 5 + 64}) {
      Fp8Args x = ok;
      x.k = v;
      expect_eq(check(mx, x), LC_ERR_SHAPE, "K off the K tile", mx, v);
    }
    // A / B / C off 16-byte alignment (8 is not enough), PA / PB off 8-byte alignment (4 is not enough)
    for (int off : {1, 2, 4, 8, 12})
      for (int i = 0; i < 3; ++i) {
        Fp8Args x = ok;
        *ptr_of(x, i) = reinterpret_cast<const void*>(4096 + off);
        expect_eq(check(mx, x), LC_ERR_SHAPE, "A / B / C alignment", mx, i, off);
      }
    for (int off : {1, 2, 4, 6})
      for (int i = 3; i < 5; ++i) {
        Fp8Args x = ok;
        *ptr_of(x, i) = reinterpret_cast<const void*>(4096 + off);
        expect_eq(check(mx, x), mx ? LC_ERR_SHAPE : LC_OK, "PA / PB alignment", mx, i, off);
      }
    {
      Fp8Args x = ok;
      x.pa = x.pb = reinterpret_cast<const void*>(4096 + 8);
      expect_eq(check(mx, x), LC_OK, "PA / PB at 8 bytes", mx);
    }
    // block scales only: K x 260 >= 2^31 is beyond the 32-bit DMA offsets of the one kernel that serves them; unit scales: the 8-wave kernel
    for (int k : {kbig, 1 << 23, 0x7fffff80}) {
      Fp8Args x = ok;
      x.k = k;
      expect_eq(check(mx, x), mx ? LC_ERR_SHAPE : LC_OK, "K beyond the DMA offsets", mx, k);
      expect_eq(check(mx, x, false), mx ? LC_ERR_SHAPE : LC_OK, "K beyond the DMA offsets, no pointers", mx, k);
    }
    Fp8Args x = ok;
    x.k = kLastFit;
    expect_eq(check(mx, x), LC_OK, "the last K inside the bound", mx);
  }
  // lc_mxfp8_pack_scales
  const void* odd = reinterpret_cast<const void*>(4100);
  expect_eq(check_mx_pack_scales(p, p, 512, 384), LC_OK, "pack: the good call");
  expect_eq(check_mx_pack_scales(p, reinterpret_cast<const void*>(4104), 512, 384), LC_OK, "pack: P at 8 bytes");
  expect_eq(check_mx_pack_scales(odd, p, 512, 384), LC_OK, "pack: S has no alignment rule");
  expect_eq(check_mx_pack_scales(nullptr, p, 512, 384), LC_ERR_ARG, "pack: S");
  expect_eq(check_mx_pack_scales(p, nullptr, 512, 384), LC_ERR_ARG, "pack: P");
  expect_eq(check_mx_pack_scales(nullptr, p, 0, 384), LC_ERR_ARG, "pack: S before rows");
  for (int v : {0, -256, -1}) {
    expect_eq(check_mx_pack_scales(p, p, v, 384), LC_ERR_SHAPE, "pack: rows", v);
    expect_eq(check_mx_pack_scales(p, p, 512, v), LC_ERR_SHAPE, "pack: K", v);
  }
  for (int v : {128, 255, 257, 384}) expect_eq(check_mx_pack_scales(p, p, v, 384), LC_ERR_SHAPE, "pack: rows off the tile", v);
  for (int v : {32, 64, 127, 129, 192}) expect_eq(check_mx_pack_scales(p, p, 512, v), LC_ERR_SHAPE, "pack: K off the K tile", v);
  for (int off : {1, 2, 4, 6}) expect_eq(check_mx_pack_scales(p, reinterpret_cast<const void*>(4096 + off), 512, 384), LC_ERR_SHAPE, "pack: P alignment", off);
}

// hgemm_entry_variant with "rule_cus" = 256 and every other knob at its default: table variant -> the variant that runs
static void walk_entry_variant() {
  Knobs k = read_knobs();
  k.rule_cus = 256;
  constexpr int A = LC_HGEMM_AUTO, G = LC_HGEMM_GENERIC, V1 = LC_HGEMM_MFMA256, V4 = LC_HGEMM_MFMA256P2, V6 = LC_HGEMM_MFMA128;
  struct Row { int M, N, K; bool al; int nn[3], tn[3]; };   // what V1, V4, V6 run under NN and under TN
  const Row rows[] = {{4096, 4096, 4096, true, {V1, V4, V6}, {V1, V4, V6}},
                      {3072, 3072, 3072, true, {V1, V4, V6}, {V1, V4, A}},
                      {2048, 2048, 2048, true, {A, A, A}, {A, A, A}},
                      {4096, 4096, 4128, true, {A, A, V6}, {A, A, V6}},
                      {4224, 4096, 4096, true, {A, A, V6}, {A, A, V6}},
                      {4096, 4096, 4096, false, {A, A, G}, {A, A, G}},
                      {1024, 1024, 1024, true, {A, A, A}, {A, A, A}},
                      {768, 768, 768, true, {A, A, V6}, {A, A, V6}},
                      {1000, 1024, 1024, true, {A, A, G}, {A, A, G}},
                      {1024, 1024, 32, true, {A, A, G}, {A, A, G}},
                      {512, 512, 8192, true, {A, A, A}, {A, A, A}},
                      {0, 256, 256, true, {A, A, V6}, {A, A, V6}}};
  const int from[3] = {V1, V4, V6};
  for (const Row& r : rows)
    for (int layout : {LC_LAYOUT_NN, LC_LAYOUT_TN}) {
      for (int i = 0; i < 3; ++i)
        expect_eq(hgemm_entry_variant(k, HgemmEntry{"walk", layout, 6, from[i]}, r.M, r.N, r.K, r.al), (layout == LC_LAYOUT_NN ? r.nn : r.tn)[i],
                  "entry variant (M, N, K)", r.M, r.N, r.K);
      // LC_HGEMM_AUTO, LC_HGEMM_GENERIC and the vector-ALU rungs run their table variant on every shape
      for (int same : {A, G, (int)LC_HGEMM_VALU_NAIVE, (int)LC_HGEMM_VALU_T8X8_K16, (int)LC_HGEMM_VALU_T16X8_K32})
        expect_eq(hgemm_entry_variant(k, HgemmEntry{"walk", layout, 3, same}, r.M, r.N, r.K, r.al), same, "an entry that never changes (M, N, K)", r.M, r.N, r.K);
    }
  // every row of the entry table itself: the result is the table variant, LC_HGEMM_AUTO or (128-tile names) LC_HGEMM_GENERIC
  for (int i = 0; i < kNumHgemmEntries; ++i) {
    const HgemmEntry& e = kHgemmEntries[i];
    if (e.variant < 0) continue;
    const int v = hgemm_entry_variant(k, e, 1280, 1280, 1280, true);
    expect_eq(v == e.variant || v == A, 1, "a table entry at 1280^3", i, v);
  }
}

int main() {
  walk_fp8_plan();
  walk_fp8_checks();
  walk_entry_variant();
  printf("gemm_plan_walk: %d cases, %d wrong\n", g_seen, g_bad);
  return g_bad ? 1 : 0;
}
