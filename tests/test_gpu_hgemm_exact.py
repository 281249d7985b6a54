"""Every fp16 HGEMM launch path behind plan_hgemm, bit for bit on EVERY element, on inputs whose result does not depend on the summation order.

tests/test_gpu_hgemm.py holds these kernels to |err| <= 1e-2 |truth| + atol on randn inputs, with 3 % of the outputs allowed not to be the
correctly rounded result, sampled rows on the larger cases and "one output ulp" between families: a kernel that stores an fp16-rounded
partial, an epilogue that converts with round-toward-zero, or a border strip that miscounts one k of 4096 passes all of that.  Here the
operands come from tests/test_abi_cpu_hgemm_exact.py (classes `signed` and `biased`: every product a multiple of 1/4, every partial sum in
any order exact in fp32), so any summation order, split-K factor, stagger, raster and tile shape must give the same bits: the exact product
rounded once to fp16.  Every case

  1. asserts the kernel name lc_hgemm_kernel_name reports for the call (the routes LC_HGEMM_AUTO decides by the CU count: on a 256-CU device),
  2. runs into a NaN-prefilled C inside a NaN guard band of 4096 halves on each side,
  3. requires every element bit-equal to the reference and the guard untouched.

There is no tolerance in this file.  Both input classes, NN and TN where the path has both, swizzle_stride 1 and one non-trivial stride.
The reference is the fp64 product of the same operands rounded to fp16 — numpy on the CPU, torch.float64 on the device from 2^29
multiply-adds on (both exact on these inputs; the CPU file anchors it to the oracle).  On a mismatch the CPU file's locator names the C tile,
the 64 x 64 block and the k-slice / rounding hypothesis that explains it.

K walks: 64, 96, 128, 352, 1056 (shorter than every ring, equal to one, longer, ending in a half K-step); the cross-check kernels need
K % 64 == 0: 64, 128, 448.  4128 / 4192 / 8224 only where a split-K rule needs the length.

What this file rests on: v_mfma_f32_16x16x32_f16, v_mfma_f32_32x32x16_f16 and v_dot2c_f32_f16 must add exactly representable products into
fp32 without an internal rounding.  That follows from fp32 accumulation of exact partial sums, and this file is where it is measured — for the
value range it uses, multiples of 1/4 whose partial sums stay below 2^24 quarter units, no further.  A family that misses bit-equality with a
locator message of "no slice ... explains" and one-ulp differences at large |C| only points at the instruction, anything else at the kernel.

The names of the border split-K launches ("hgemm_splitk") do not carry the split factor (format_hgemm prints no ks for the 256-tile family): those
cases assert the kernel, not that the factor took effect; whichever form runs is held to the same bits."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_abi_cpu_hgemm_exact import CLASSES, exact_inputs, locate, reference
from tests.test_gpu_hgemm import MID_COMBOS

pytestmark = pytest.mark.gpu

GUARD = 4096
DEVICE_REF_FROM = 1 << 29      # M N K from which the reference is computed on the device
KS = (64, 96, 128, 352, 1056)
KS64 = (64, 128, 448)
STAGGER_OFF = 1 << 27
STAGGERS = (STAGGER_OFF, 0, 1 | 16 << 12 | 7 << 20, 1 << 4 | 2 << 12 | 31 << 20, 1 << 8 | 2 << 12 | 31 << 20, 1 << 4 | 3 << 8 | 3 << 12 | 31 << 20,
            15 | 15 << 4 | 15 << 8 | 255 << 12 | 127 << 20)       # off, auto, the five forced codes of test_k_loop_stagger_walks_every_k_tile_once
V = dict(mfma256=1, generic=3, pingpong2=4, mfma128=6, w4b=9, w4c=10, w4x=12, w4y=13, mid=14, edge=15, ragged=16, kpad=17, auto=0)
LAYS = ("nn", "tn")


def _capi():
    from leetcuda_amd import capi
    capi.load()
    return capi


def _nnn(lay):
    return "true" if lay == "nn" else "false"


@contextlib.contextmanager
def _knobs(capi, knobs):
    for k, v in (knobs or {}).items():
        capi.tune(k, v)
    try:
        yield
    finally:
        for k in (knobs or {}):
            capi.tune(k, capi.tune_get(k)[1])


@functools.lru_cache(maxsize=6)
def _inputs(cls, M, N, K):
    """the operands of one (class, shape) on the device, and the reference: computed once, shared, never written"""
    a_np, b_np = exact_inputs(cls, M, N, K)
    x = SimpleNamespace(a_np=a_np, b_np=b_np, M=M, N=N, K=K, cls=cls)
    x.a = torch.from_numpy(np.array(a_np)).cuda()      # (a writable copy: the shared arrays are read-only)
    x.b = torch.from_numpy(np.array(b_np)).cuda()                 # [K,N]: the NN operand
    x.bt = x.b.t().contiguous()                         # [N,K]: the TN operand's storage
    if M * N * K >= DEVICE_REF_FROM:
        x.ref = (x.a.double() @ x.b.double()).half()    # (multiples of 1/4 below 2^16: exact in fp64 and in the fp32 the cast passes through)
    else:
        x.ref = torch.from_numpy(reference(a_np, b_np)).cuda()
    torch.cuda.synchronize()
    return x


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_inputs():
    yield
    _inputs.cache_clear()


def _c_in_guard(M, N):
    buf = torch.full((M * N + 2 * GUARD,), float("nan"), dtype=torch.half, device="cuda")
    return buf, buf[GUARD:GUARD + M * N].view(M, N)


def _require_exact(x, buf, c, what, tile=(256, 256)):
    """every element of C bit-equal to the reference, the guard band still NaN; the locator speaks on failure"""
    M, N = x.M, x.N
    guard_ok = bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + M * N:]).all())
    if guard_ok and torch.equal(c.view(torch.int16), x.ref.view(torch.int16)):
        return
    assert guard_ok, f"{what} [{x.cls}]: wrote outside C (guard band of {GUARD} halves touched)"
    f = locate(c.cpu().numpy(), x.a_np, x.b_np, x.ref.cpu().numpy(), f"{what} [{x.cls}]", tile)
    pytest.fail(f.message)


def _name_ok(name, want):
    kind, txt = want
    return name == txt if kind == "eq" else name.startswith(txt) if kind == "start" else (name.startswith(txt[0]) and name.endswith(txt[1]))


def _run(capi, x, lay, variant, stride=1, knobs=None, entry=None):
    L = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
    buf, c = _c_in_guard(x.M, x.N)
    with _knobs(capi, knobs):
        if entry:
            capi.hgemm_call(entry, x.a, x.b if lay == "nn" else x.bt, c, 2, True, stride)
        else:
            capi.hgemm(x.a, x.b if lay == "nn" else x.bt, c, layout=L, variant=variant, swizzle_stride=stride)
    torch.cuda.synchronize()
    return buf, c


def _case(lay, shapes, variant, want, knobs=None, tile=(256, 256), by_cus=False, strides=(1, 256), classes=CLASSES):
    """One path: the name first, then both classes x the shapes x the strides.  by_cus: what runs is a rule's choice that depends on the CU
    count — the name is asserted on a 256-CU device only (the convention of tests/test_gpu_numerics.py)."""
    capi = _capi()
    L = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
    for (M, N, K) in shapes:
        with _knobs(capi, knobs):
            name = capi.hgemm_kernel_name(M, N, K, L, variant)
        if not by_cus or capi.device_check() == 256:
            assert _name_ok(name, want), (name, want, (M, N, K), knobs)
        for cls in classes:
            x = _inputs(cls, M, N, K)
            for stride in strides:
                buf, c = _run(capi, x, lay, variant, stride, knobs)
                _require_exact(x, buf, c, f"{name} {lay} ({M},{N},{K}) stride {stride} {knobs or ''}", tile)


def test_the_device_reference_equals_the_cpu_reference():
    """torch.float64 on the device (the large shapes) and numpy on the CPU (the others) are the same reference"""
    for cls in CLASSES:
        for (M, N, K) in ((384, 640, 1056), (100, 1032, 4096), (77, 136, 8224)):
            x = _inputs(cls, M, N, K)
            dev = (x.a.double() @ x.b.double()).half()
            assert torch.equal(dev.view(torch.int16), torch.from_numpy(reference(x.a_np, x.b_np)).cuda().view(torch.int16)), (cls, M, N, K)
            assert torch.equal(x.bt, torch.from_numpy(np.ascontiguousarray(x.b_np.T)).cuda())


# ---- the 256-tile families ---------------------------------------------------------------------------------------------------------------
def _names256(fam, lay, sched=None):
    n = _nnn(lay)
    return {"mfma256": f"hgemm_mfma256_kernel<{n}>", "pingpong2": f"hgemm_pingpong2_kernel<{n},false>", "w4b": f"hgemm_w4b_kernel<{n},false,0>",
            "w4c": f"hgemm_w4b_kernel<{n},true,0>", "w4x": "hgemm_w4x_kernel<false>",
            "w4y": f"hgemm_w4y_kernel<{n},{1 if lay == 'nn' else 2 if sched is None else sched}>"}[fam]


FAM256 = [(fam, lay) for lay in LAYS for fam in ("mfma256", "pingpong2", "w4b", "w4c", "w4x", "w4y") if not (fam == "w4x" and lay == "nn")]


@pytest.mark.parametrize("fam,lay", FAM256, ids=[f"{f}-{lay}" for f, lay in FAM256])
def test_256_tile_families(fam, lay):
    ks = KS if fam == "w4y" else KS64         # (hgemm_w4y_kernel alone takes the half K-step, K % 64 == 32)
    _case(lay, [(M, N, K) for (M, N) in ((512, 512), (256, 768)) for K in ks], V[fam], ("eq", _names256(fam, lay)))


@pytest.mark.parametrize("sched", [0, 1, 2])
def test_w4y_every_generated_schedule(sched):
    _case("tn", [(512, 512, K) for K in KS], V["w4y"], ("eq", _names256("w4y", "tn", sched)), {"w4y_sched": sched})


@pytest.mark.parametrize("lay", LAYS)
def test_w4y_border_strips(lay):
    """128-wide right and bottom strips and the corner on the 128-tile kernel in a second launch, every K walk incl. the half step"""
    _case(lay, [(384, 640, K) for K in KS], V["w4y"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"))


@pytest.mark.parametrize("ks", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("lay", LAYS)
def test_w4y_border_strips_split_k(lay, ks):
    """fp32 partials of the border blocks in the workspace + the reduce kernel; K ranges of unequal length, the half step in the last one.
    (The name does not report the factor: the assertion below shows the kernel, not that "hgemm_splitk" took effect.)"""
    _case(lay, [(384, 384, 4192)], V["w4y"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"), {"hgemm_splitk": ks})


@pytest.mark.parametrize("stagger", STAGGERS, ids=[f"stagger{hex(s)}" for s in STAGGERS])
@pytest.mark.parametrize("lay", LAYS)
def test_w4y_k_loop_stagger(lay, stagger):
    """start tile ((index & mask) * step) mod KT, wrapping: KT = 1, 2, 3 (the clamped prefetch of the last iterations wraps too) and 16"""
    _case(lay, [(512, 768, K) for K in (64, 128, 192, 1024)], V["w4y"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"), {"hgemm_stagger": stagger}, strides=(1, 512))


@pytest.mark.parametrize("raster", [1, 2])
@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("lay", LAYS)
def test_w4y_persistent_walk_and_rasters(lay, persist, raster):
    """512 C tiles: two per persistent workgroup on 256 CUs (the cross-tile prefetch is the whole supply of a one-tile K loop at K = 64), K = 160:
    two tiles and the half step; both block -> tile maps"""
    _case(lay, [(8192, 4096, K) for K in (64, 160)], V["w4y"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"), {"hgemm_persist": persist, "hgemm_raster": raster},
          strides=(1, 2048))


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("tail", [0, 1, 2])
@pytest.mark.parametrize("lay", LAYS)
def test_w4y_tail_split(lay, tail, tile):
    """17 x 17 tiles of 256: a last round of 33 tiles — one launch (0), quadrants / eighths on the mid-size kernel (1, "hgemm_tail_tile"), the 128-tile
    kernel (2; unsplit here: K = 96 is one K tile, its split-K needs 8 tiles per range — the next test)"""
    _case(lay, [(256 * 17, 256 * 17, 96)], V["w4y"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"), {"hgemm_tail": tail, "hgemm_tail_tile": tile}, strides=(1, 2048))


@pytest.mark.parametrize("lay", LAYS)
def test_w4y_tail_on_the_128_tile_kernel_with_split_k(lay):
    """"hgemm_tail" = 2 with 16 K tiles and a half step: the 132 quadrant blocks of the last round split K in two (plan_hgemm: about 1.5 blocks per CU,
    at least 8 K tiles per range) through the workspace and the reduce kernel.  (The name does not report the factor.)"""
    _case(lay, [(256 * 17, 256 * 17, 1056)], V["w4y"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"), {"hgemm_tail": 2}, strides=(2048,))


@pytest.mark.parametrize("lay", LAYS)
def test_auto_route_with_a_large_interior(lay):
    _case(lay, [(3200, 3200, 96)], V["auto"], ("start", f"hgemm_w4y_kernel<{_nnn(lay)},"), by_cus=True, strides=(1, 1024))


# ---- the 128-tile kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("lay", LAYS)
def test_128_tile_kernel_four_and_eight_waves(lay, waves):
    _case(lay, [(M, N, K) for (M, N) in ((384, 128), (128, 640)) for K in KS], V["mfma128"], ("eq", f"hgemm_mfma128_kernel<{_nnn(lay)},{waves}>"),
          {"hgemm_128w": waves}, tile=(128, 128))


# ---- the mid-size kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay,tmw,tnw,ns", MID_COMBOS)
def test_mid_kernel_every_tile_and_ring_depth(lay, tmw, tnw, ns):
    tm, tn = 64 * tmw, 64 * tnw
    _case(lay, [(M, N, K) for (M, N) in ((2 * tm, 2 * tn), (3 * tm, tn)) for K in KS], V["mid"], ("eq", f"hgemm_mid_kernel<{_nnn(lay)},{tmw},{tnw},{ns}>"),
          {"hgemm_mid": 10 * tmw + tnw, "hgemm_mid_ns": ns}, tile=(tm, tn), strides=(1, 2 * tn))


@pytest.mark.parametrize("ks", [2, 3, 7, 8])
@pytest.mark.parametrize("tile", [12, 22])
@pytest.mark.parametrize("lay", LAYS)
def test_mid_kernel_split_k(lay, tile, ks):
    _case(lay, [(256, 384, 4128), (512, 512, 8224)], V["mid"], ("start+end", ("hgemm_mid_sk_kernel<", f"> x{ks}")), {"hgemm_mid": tile, "hgemm_mid_splitk": ks},
          tile=(64 * (tile // 10), 128))


@pytest.mark.parametrize("shape", [(1088, 1152, 512), (192, 8256, 320)])
@pytest.mark.parametrize("lay", LAYS)
def test_mid_kernel_on_64_multiples(lay, shape):
    """M, N multiples of 64 that no 128-tile divides: a mid-size tile where one divides the shape (NN has 128-column tiles only: clamped tiles)"""
    pre = "hgemm_mid_kernel<" if lay == "tn" or shape[1] % 128 == 0 else "hgemm_mid_edge_kernel<"
    _case(lay, [shape], V["auto"], ("start", pre), tile=(64, 128))


# ---- ragged shapes -----------------------------------------------------------------------------------------------------------------------
RAGGED_TILES = [(lay, t) for lay in LAYS for t in ((12, 22, 32) if lay == "nn" else (12, 22, 23, 33))]


@pytest.mark.parametrize("lay,tile", RAGGED_TILES)
def test_ragged_whole_problem_on_clamped_tiles(lay, tile):
    """kind 2: every tile the layout has; one tile row (M = 100) and tiles that reach beyond M and N on both sides of a seam (300 x 584)"""
    tmw, tnw = tile // 10, tile % 10
    _case(lay, [(M, N, K) for (M, N) in ((100, 72 * 8), (300, 584)) for K in KS], V["auto"], ("start", f"hgemm_mid_edge_kernel<{_nnn(lay)},{tmw},{tnw},"),
          {"hgemm_ragged_tile": tile}, tile=(64 * tmw, 64 * tnw))


@pytest.mark.parametrize("ks", [2, 3, 7, 8])
@pytest.mark.parametrize("tile", [12, 22])
@pytest.mark.parametrize("lay", LAYS)
def test_ragged_split_k(lay, tile, ks):
    _case(lay, [(100, 1032, 4096), (77, 136, 8224)], V["auto"], ("eq", f"hgemm_mid_edge_sk_kernel<{_nnn(lay)},{tile // 10},3> x{ks}"),
          {"hgemm_ragged_tile": tile, "hgemm_mid_splitk": ks}, tile=(64 * (tile // 10), 128))


RAGGED_FORK_SHAPE = (772, 11016)       # 3 x 43 = 129 tiles of 256 x 256: the fewest that are "more than half a CU's worth" on 256 CUs, + 4 rows and 8 columns


@pytest.mark.parametrize("fork", [1, 2])
@pytest.mark.parametrize("lay", LAYS)
def test_ragged_interior_and_forked_border(lay, fork):
    """kind 1: the interior on hgemm_w4y_kernel, the L-shaped border on hgemm_mid_edge_kernel behind it (1) or beside it on a side stream (2)"""
    n = _nnn(lay)
    _case(lay, [RAGGED_FORK_SHAPE + (K,) for K in (64, 352)], V["ragged"], ("start+end", (f"hgemm_w4y_kernel<{n},", f" + hgemm_mid_edge_kernel<{n},2,2,3>")),
          {"hgemm_ragged_fork": fork}, by_cus=True, strides=(1, 2048))


# ---- edge, generic, K-pad, the vector-ALU ladder ------------------------------------------------------------------------------------------
EDGE_SHAPES = [(64, 64, 64), (128, 128, 32), (100, 72, 56), (1, 8, 8), (257, 136, 72), (384, 640, 96), (129, 1000, 40), (1000, 3000, 520), (130, 130, 64),
               (2880, 2944, 264)]
GENERIC_SHAPES = [(64, 64, 64), (128, 128, 32), (100, 72, 50), (1, 1, 1), (257, 129, 65), (384, 640, 96), (129, 1000, 40)]


@pytest.mark.parametrize("shape", EDGE_SHAPES)
@pytest.mark.parametrize("lay", LAYS)
def test_edge_kernel(lay, shape):
    capi = _capi()
    if lay == "nn" and shape[1] % 8:           # (130, 130, 64) is TN-only: NN rows of B must be whole 16-byte chunks
        with pytest.raises(capi.LcError, match="Tensor size mismatch"):
            capi.hgemm_kernel_name(*shape, capi.LAYOUT_NN, capi.HGEMM_EDGE)
        return
    _case(lay, [shape], V["edge"], ("eq", f"hgemm_edge_kernel<{_nnn(lay)}>"), tile=(128, 128))


@pytest.mark.parametrize("shape", GENERIC_SHAPES)
@pytest.mark.parametrize("lay", LAYS)
def test_generic_kernel(lay, shape):
    _case(lay, [shape], V["generic"], ("eq", f"hgemm_generic_kernel<{_nnn(lay)}>"), tile=(64, 64))


@pytest.mark.parametrize("lay", LAYS)
def test_k_padding_path(lay):
    """K % 32 != 0: zero-padded operand copies in the workspace + the tuned kernels; LC_HGEMM_AUTO under "hgemm_kpad" = 2 on a small problem, the
    explicit family and the rule's own choice on a large one"""
    capi = _capi()
    L = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
    for shape, variant, knobs in (((130, 136, 296), "auto", {"hgemm_kpad": 2}), ((1000, 3000, 520), "kpad", None), ((1000, 3000, 520), "auto", None)):
        M, N, K = shape
        with _knobs(capi, knobs):
            inner = capi.hgemm_kernel_name(M, N, (K + 31) // 32 * 32, L)
        _case(lay, [shape], V[variant], ("eq", "hgemm_pad_copy_kernel + " + inner), knobs, tile=(128, 128), by_cus=variant == "auto" and not knobs)


@pytest.mark.parametrize("rung", list(range(20, 31)))
def test_vector_alu_ladder(rung):
    _case("nn", [(512, 384, 320)], rung, ("start", "hgemm_valu_"), tile=(64, 64))


@pytest.mark.parametrize("cls", CLASSES)
def test_every_reference_entry_name(cls):
    """every entry of the reference's table through lc_hgemm_call at a 256-multiple and at a ragged shape, the two hipBLASLt rows included"""
    capi = _capi()
    seen = 0
    capi.hgemm_call("init_cublas_handle", *[torch.zeros(8, 8, dtype=torch.half, device="cuda")] * 3)
    try:
        for (M, N, K) in ((512, 512, 128), (257, 136, 72)):
            x = _inputs(cls, M, N, K)
            for entry, L, nargs in capi.hgemm_entries():
                if nargs == 0:
                    continue
                lay = "nn" if L == capi.LAYOUT_NN else "tn"
                buf, c = _run(capi, x, lay, None, 256, entry=entry)
                _require_exact(x, buf, c, f"{entry} {lay} ({M},{N},{K})")
                seen += 1
    finally:
        capi.hgemm_call("destroy_cublas_handle", *[torch.zeros(8, 8, dtype=torch.half, device="cuda")] * 3)
    assert seen == 2 * 36, seen


# ---- every family against every other ------------------------------------------------------------------------------------------------------
def _families_for(shape, lay):
    """(label, variant, knobs) of every family that takes the shape"""
    out = [("auto", V["auto"], None), ("edge", V["edge"], None), ("generic", V["generic"], None)]
    mid_tiles = (12, 22, 32) if lay == "nn" else (12, 22, 32, 13, 23, 33)
    if shape in ((512, 512, 352), (384, 640, 96)):
        M, N, _ = shape
        out += [("w4y", V["w4y"], None), ("w4y_plain_walk", V["w4y"], {"hgemm_stagger": STAGGER_OFF}), ("mfma128_4w", V["mfma128"], {"hgemm_128w": 1}),
                ("mfma128_8w", V["mfma128"], {"hgemm_128w": 2})]
        if lay == "tn":
            out += [(f"w4y_sched{s}", V["w4y"], {"w4y_sched": s}) for s in (0, 1)]
        for t in mid_tiles:
            if M % (64 * (t // 10)) == 0 and N % (64 * (t % 10)) == 0:
                out += [(f"mid{t}_ns{ns}", V["mid"], {"hgemm_mid": t, "hgemm_mid_ns": ns}) for ns in (2, 3)]
        if lay == "nn":
            out += [(f"valu{r}", r, None) for r in range(20, 31)]
    else:
        out += [("ragged", V["ragged"], None), ("ragged_unsplit", V["ragged"], {"hgemm_mid_splitk": 1})]
        out += [(f"ragged{t}", V["auto"], {"hgemm_ragged_tile": t, "hgemm_mid_splitk": 1}) for t in ((12, 22, 32) if lay == "nn" else (12, 22, 23, 33))]
        out += [(f"ragged12_x{ks}", V["auto"], {"hgemm_ragged_tile": 12, "hgemm_mid_splitk": ks}) for ks in (2, 3, 8)]
        if lay == "nn":
            out.append(("valu20", 20, None))
    return out


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", [(512, 512, 352), (384, 640, 96), (100, 1032, 4096)])
@pytest.mark.parametrize("lay", LAYS)
def test_cross_family_equality(lay, shape, cls):
    """Every family that takes the shape — the flagship kernel in its schedules and walks, the 128-tile kernel on four and eight waves, every mid-size
    tile and ring depth, the clamped tiles with and without split-K, edge, generic, the vector-ALU rungs, LC_HGEMM_AUTO — gives the SAME bits, the
    reference's.  This is the assertion a change of a K loop's schedule trips."""
    capi = _capi()
    L = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
    M, N, K = shape
    x = _inputs(cls, M, N, K)
    outs = []
    for label, variant, knobs in _families_for(shape, lay):
        with _knobs(capi, knobs):
            name = capi.hgemm_kernel_name(M, N, K, L, variant)
        buf, c = _run(capi, x, lay, variant, 256, knobs)
        _require_exact(x, buf, c, f"{label} = {name} {lay} ({M},{N},{K})")
        outs.append((label, c))
    assert len(outs) >= 11
    for label, c in outs[1:]:
        assert torch.equal(c.view(torch.int16), outs[0][1].view(torch.int16)), (label, outs[0][0])


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------
WS_USERS = [("border_splitk", (3200, 3200, 1056), None, "hgemm_w4y_kernel<"), ("mid_splitk", (512, 512, 8224), None, "hgemm_mid_sk_kernel<"),
            ("ragged_splitk", (100, 1032, 4096), None, "hgemm_mid_edge_sk_kernel<"), ("kpad", (1000, 3000, 520), None, "hgemm_pad_copy_kernel + ")]


@pytest.mark.parametrize("user", WS_USERS, ids=[u[0] for u in WS_USERS])
@pytest.mark.parametrize("lay", LAYS)
def test_captured_auto_call_of_every_workspace_user(lay, user):
    """The four users of the cached workspace run their workspace-free form while a stream is captured (the border and the tiles unsplit, the
    edge kernel for K % 32 != 0): one warm-up on the capture stream, then the replay of one captured LC_HGEMM_AUTO call — both the eager and the
    replayed C bit-equal to the reference.  (The border user's name carries no split factor: by plan_hgemm's rule 49 border blocks with 16 K tiles
    split in two when run eagerly; the name shows the kernel only.)"""
    capi = _capi()
    _, (M, N, K), knobs, pre = user
    L = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
    name = capi.hgemm_kernel_name(M, N, K, L)
    if capi.device_check() == 256:
        assert name.startswith(pre), name
    for cls in CLASSES:
        x = _inputs(cls, M, N, K)
        bb = x.b if lay == "nn" else x.bt
        buf, c = _c_in_guard(M, N)
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            capi.hgemm(x.a, bb, c, layout=L, variant=capi.HGEMM_AUTO, swizzle_stride=256)
            torch.cuda.synchronize()
            _require_exact(x, buf, c, f"{name} {lay} ({M},{N},{K}) eager on a side stream")
            buf.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                capi.hgemm(x.a, bb, c, layout=L, variant=capi.HGEMM_AUTO, swizzle_stride=256)
        torch.cuda.synchronize()
        assert bool(torch.isnan(c).all())               # captured, not run
        g.replay()
        torch.cuda.synchronize()
        _require_exact(x, buf, c, f"{name} {lay} ({M},{N},{K}) replayed from a captured graph")


# ---- operands off 16-byte alignment --------------------------------------------------------------------------------------------------------
def _offset_view(t, off):
    """the same values in a view `off` halves into a larger buffer"""
    big = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = big[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


REFUSING = ("mfma256", "pingpong2", "w4b", "w4c", "w4x", "w4y", "mfma128", "mid", "edge", "ragged", "kpad")
# shape -> the families of REFUSING that TAKE it when the operands are aligned: only for those does a refusal show the alignment check.  The first
# two shapes are the issue's; no shape serves LC_HGEMM_RAGGED (ragged M / N, K % 32 == 0) and LC_HGEMM_KPAD (K % 32 != 0, K >= 256) beside the
# tiled families, so each gets one of its own.
ALIGN_SHAPES = {(256, 256, 64): ("mfma256", "pingpong2", "w4b", "w4c", "w4x", "w4y", "mfma128", "mid", "edge"), (130, 72, 56): ("edge",),
                (100, 576, 64): ("edge", "ragged"), (130, 136, 296): ("edge", "kpad")}


def _takes(capi, L, shape, variant):
    try:
        return bool(capi.hgemm_kernel_name(*shape, L, V[variant]))
    except capi.LcError:
        return False


@pytest.mark.parametrize("shape", list(ALIGN_SHAPES))
@pytest.mark.parametrize("lay", LAYS)
def test_operands_off_16_byte_alignment(lay, shape):
    """A, B or C one half or four halves (2 / 8 bytes) into a larger buffer: LC_HGEMM_AUTO and LC_HGEMM_GENERIC run the element-wise kernel and are
    bit-equal with the guards intact; every family that moves 16-byte chunks refuses with "Tensor size mismatch" and leaves C untouched.  Every
    family of REFUSING is called at every shape, but a refusal proves the alignment check only where the family takes the shape with aligned
    operands: that set is asserted per shape (ALIGN_SHAPES, through lc_hgemm_kernel_name) and each of its families first runs the ALIGNED call,
    bit-equal to the reference, so that the refusal which follows can only come from the pointers.  Every family has such a shape.
    (lc_hgemm_kernel_name plans for aligned operands: there is no name to assert for the misaligned calls.)"""
    capi = _capi()
    L = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
    M, N, K = shape
    takes = ALIGN_SHAPES[shape]
    assert tuple(v for v in REFUSING if _takes(capi, L, shape, v)) == takes
    assert {v for vs in ALIGN_SHAPES.values() for v in vs} == set(REFUSING)
    for cls in CLASSES:
        x = _inputs(cls, M, N, K)
        for variant in takes:
            buf, c = _run(capi, x, lay, V[variant], 256)
            _require_exact(x, buf, c, f"LC_HGEMM_{variant.upper()} {lay} ({M},{N},{K}) aligned", (64, 64))
        b0 = x.b if lay == "nn" else x.bt
        for which in "ABC":
            for off in (1, 4):
                a = _offset_view(x.a, off) if which == "A" else x.a
                bb = _offset_view(b0, off) if which == "B" else b0
                goff = GUARD + (off if which == "C" else 0)
                for variant in ("auto", "generic") + REFUSING:
                    buf = torch.full((M * N + 2 * GUARD + 16,), float("nan"), dtype=torch.half, device="cuda")
                    c = buf[goff:goff + M * N].view(M, N)
                    assert any(t.data_ptr() % 16 for t in (a, bb, c)) and a.is_contiguous() and bb.is_contiguous() and c.is_contiguous()
                    what = f"LC_HGEMM_{variant.upper()} {lay} ({M},{N},{K}) [{cls}] {which} + {off} halves"
                    if variant in REFUSING:
                        with pytest.raises(capi.LcError, match="Tensor size mismatch"):
                            capi.hgemm(a, bb, c, layout=L, variant=V[variant], swizzle_stride=256)
                        torch.cuda.synchronize()
                        assert bool(torch.isnan(buf).all()), what + ": refused, yet C was written"
                        continue
                    capi.hgemm(a, bb, c, layout=L, variant=V[variant], swizzle_stride=256)
                    torch.cuda.synchronize()
                    assert bool(torch.isnan(buf[:goff]).all()) and bool(torch.isnan(buf[goff + M * N:]).all()), what + ": wrote outside C"
                    if not torch.equal(c.view(torch.int16), x.ref.view(torch.int16)):
                        pytest.fail(locate(c.cpu().numpy(), x.a_np, x.b_np, x.ref.cpu().numpy(), what, (64, 64)).message)
