"""CPU tests of the append-to-cache boundary (lc_kv_append_paged_f16, lc_kv_append_paged_kv8 and their two name calls; no call here reaches a
device): the error codes and their order for both entries (NULL scales are accepted), the span bound at one byte per element against two, Nq
beyond the decode kernels' 64 rows, the name grid, the Python wrappers' refusals, the audit report of the four kernels — then the reference's own
proof (append_ref fills a pool exactly as decode_lib.paginate lays it out) and a test of the GPU tests' inputs: on them the pools of nine wrong
kernels differ from the reference's.

The reference, the wrong kernels and the inputs are shared with tests/test_gpu_kv_append.py: tests/append_lib.py."""
import ctypes as C
import json

import pytest
import torch

from leetcuda_amd import capi
from tests import append_lib as al
from tests.decode_lib import K_SCALES, V_SCALES, decode_inputs, paginate, quantize, scales

ENTRIES = ("f16", "kv8")


def _run(lib, entry, ptrs, shape, flags, sc=(None, None)):
    """ptrs: Knew, Vnew, Kpool, Vpool, block_table, kv_len; shape: B, Hkv, Nq, num_pages, page_size, max_pages, D"""
    if entry == "kv8":
        return lib.lc_kv_append_paged_kv8(*ptrs, *sc, *shape, flags, None)
    return lib.lc_kv_append_paged_f16(*ptrs, *shape, flags, None)


def _name(entry, B, Hkv, Nq, ps, mp, D, flags=0):
    buf = C.create_string_buffer(128)
    fn = capi.load().lc_kv_append_paged_kv8_kernel_name if entry == "kv8" else capi.load().lc_kv_append_paged_kernel_name
    return fn(B, Hkv, Nq, ps, mp, D, flags, buf, 128), buf.value.decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_and_their_order(built, entry):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    p = C.c_void_p(16)
    ok = (2, 2, 4, 70, 16, 64, 128)           # B, Hkv, Nq, num_pages, page_size, max_pages, D
    bad_shape = (2, 0, 4, 70, 24, 64, 256)
    bad_dim = (2, 2, 4, 70, 16, 64, 96)
    for sc in ((p, p), (None, None), (p, None), (None, p)) if entry == "kv8" else ((None, None),):
        def f(ptrs, shape, flags=0, sc=sc):
            return _run(lib, entry, ptrs, shape, flags, sc)
        for bad in (1, 2, 3, 4, -1, 1 << 30):                    # no flag is defined: flags before everything
            assert f([p] * 6, ok, bad) == capi.LC_ERR_ARG, bad
            assert f([p] * 6, bad_shape, bad) == capi.LC_ERR_ARG
            assert f([None] + [p] * 5, ok, bad) == capi.LC_ERR_ARG
            assert _name(entry, 2, 2, 4, 16, 64, 128, bad)[0] == capi.LC_ERR_ARG
            assert _name(entry, 2, 0, 4, 24, 64, 256, bad)[0] == capi.LC_ERR_ARG
        for nul in range(6):                                     # a null pointer before shape and head dim
            ptrs = [p] * 6
            ptrs[nul] = None
            for shape in (ok, bad_shape, bad_dim):
                assert f(ptrs, shape) == capi.LC_ERR_ARG, (nul, shape)
        for shape in ((0, 2, 4, 70, 16, 64, 128), (-1, 2, 4, 70, 16, 64, 128), (2, 0, 4, 70, 16, 64, 128), (2, -2, 4, 70, 16, 64, 128),
                      (2, 2, 0, 70, 16, 64, 128), (2, 2, -4, 70, 16, 64, 128), (2, 2, 4, 0, 16, 64, 128), (2, 2, 4, -3, 16, 64, 128),
                      (2, 2, 4, 70, 16, 0, 128), (2, 2, 4, 70, 16, -1, 128), (2, 2, 4, 70, 16, 64, 0), (2, 2, 4, 70, 16, 64, -128),
                      (2, 2, 4, 70, 8, 64, 128), (2, 2, 4, 70, 24, 64, 128), (2, 2, 4, 70, 0, 64, 128), (2, 2, 4, 70, -16, 64, 128),
                      (2, 2, 4, 70, 1, 64, 128), (2, 2, 4, 70, 48, 64, 128),
                      (2, 2, 4, 70, 1 << 16, 1 << 16, 64),       # max_pages x page_size is no int
                      (2, 2, 4, 70, 16, 1 << 21, 128), (2, 2, 4, 70, 1 << 21, 16, 64),      # a (page, head) span of 4 GiB (fp8: 2 GiB)
                      (1 << 16, 1 << 16, 1, 70, 16, 64, 64), (1 << 15, 1 << 15, 64, 70, 16, 64, 64), (1 << 30, 1, 17, 70, 16, 64, 128)):   # the grid
            assert f([p] * 6, shape) == capi.LC_ERR_SHAPE, shape
            assert _name(entry, *shape[:3], *shape[4:])[0] == capi.LC_ERR_SHAPE or shape[3] <= 0, shape      # (the name call takes no num_pages)
            assert f([p] * 6, shape[:6] + (96,)) == capi.LC_ERR_SHAPE or shape[6] <= 0, shape                # shape before head dim
        assert f([p] * 6, bad_shape) == capi.LC_ERR_SHAPE
        # the order inside LC_ERR_SHAPE cannot be seen from outside; what can: every one of them comes before the head dim ...
        for mis in range(4):                                     # ... the alignment of Knew, Vnew and the pools too
            ptrs = [p] * 6
            ptrs[mis] = C.c_void_p(8)
            assert f(ptrs, ok) == capi.LC_ERR_SHAPE, mis
            assert f(ptrs, bad_dim) == capi.LC_ERR_SHAPE
        for mis in (4, 5):                                       # block_table and kv_len are int32 arrays: 4-byte data, no 16-byte rule
            ptrs = [p] * 6
            ptrs[mis] = C.c_void_p(8)
            assert f(ptrs, bad_dim) == capi.LC_ERR_HEADDIM
        for d in (32, 96, 256, 512, 1024, 16, 48, 8, 1):
            assert f([p] * 6, ok[:6] + (d,)) == capi.LC_ERR_HEADDIM, d
            assert _name(entry, 2, 2, 4, 16, 64, d)[0] == capi.LC_ERR_HEADDIM
    assert _name(entry, 2, 2, 4, 8, 64, 128)[0] == capi.LC_ERR_SHAPE
    assert _name(entry, 2, 2, 4, 8, 64, 96)[0] == capi.LC_ERR_SHAPE


def test_the_span_bound_is_one_byte_an_element_for_fp8_and_two_for_fp16(built):
    """max_pages x page_size x D x (element bytes) below 2 GiB — the decode calls' bound, so a pool geometry append takes, decode takes"""
    for ps, mp, D in ((16, 1 << 19, 128), (1 << 20, 16, 64)):        # 2^30 elements: 2 GiB of halves, 1 GiB of bytes
        assert _name("f16", 1, 2, 4, ps, mp - 1, D)[0] == capi.LC_OK
        assert _name("f16", 1, 2, 4, ps, mp, D)[0] == capi.LC_ERR_SHAPE
        assert _name("kv8", 1, 2, 4, ps, mp, D)[0] == capi.LC_OK
        assert _name("kv8", 1, 2, 4, ps, 2 * mp - 1, D)[0] == capi.LC_OK
        assert _name("kv8", 1, 2, 4, ps, 2 * mp, D)[0] == capi.LC_ERR_SHAPE
        # the largest geometry each append entry takes is one its reader takes (a name call that raised would have refused it)
        assert capi.attn_decode_paged_kernel_name(1, 8, 2, 4, ps, mp - 1, D).startswith("attn_decode_paged_kernel")
        assert capi.attn_decode_paged_kv8_kernel_name(1, 8, 2, 4, ps, 2 * mp - 1, D).startswith("attn_decode_paged_kv8_kernel")


@pytest.mark.parametrize("entry", ENTRIES)
def test_nq_is_not_bounded_by_the_decode_kernels_row_tiles(built, entry):
    lib = capi.load()
    p = C.c_void_p(16)
    for nq in (64, 65, 800, 4096):
        assert _name(entry, 2, 2, nq, 16, 64, 128)[0] == capi.LC_OK, nq
        assert _name(entry, 8, 8, nq, 16, 512, 64)[0] == capi.LC_OK, nq
    assert _name(entry, 1, 1, 2 ** 31 - 1, 16, 64, 128)[0] == capi.LC_OK          # the largest grid one (batch entry, head) can ask for
    # (the run call with these shapes is the GPU module's business: here every pointer is a fake)
    assert _run(lib, entry, [p] * 6, (2, 2, 4096, 70, 16, 64, 96), 0) == capi.LC_ERR_HEADDIM


def test_name_grid_and_name_buffer_errors(built):
    lib = capi.load()
    for entry, stem in (("f16", "kv_append_paged_kernel"), ("kv8", "kv_append_paged_kv8_kernel")):
        for D in (64, 128):
            for Bn, Hkv, Nq in ((3, 2, 1), (3, 2, 5), (1, 4, 512), (64, 8, 1), (8, 8, 4096), (1, 1, 100)):
                for ps, mp in ((16, 64), (256, 4), (1024, 1)):
                    assert _name(entry, Bn, Hkv, Nq, ps, mp, D) == (capi.LC_OK, f"{stem}<{D}>")
                    assert capi.kv_append_paged_kernel_name(Bn, Hkv, Nq, ps, mp, D, kv8=entry == "kv8") == f"{stem}<{D}>"
        fn = lib.lc_kv_append_paged_kv8_kernel_name if entry == "kv8" else lib.lc_kv_append_paged_kernel_name
        assert fn(2, 2, 4, 16, 64, 128, 0, None, 128) == capi.LC_ERR_ARG
        assert fn(2, 2, 4, 16, 64, 128, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
        assert fn(2, 2, 4, 16, 64, 128, 0, C.create_string_buffer(4), 0) == capi.LC_ERR_ARG
        assert fn(2, 2, 4, 16, 64, 128, 0, C.create_string_buffer(4), -1) == capi.LC_ERR_ARG
    with pytest.raises(capi.LcError):
        capi.kv_append_paged_kernel_name(2, 2, 4, 24, 64, 128)


def test_capi_wrappers_check_shapes_dtypes_and_devices_without_a_gpu(built):
    Bn, Hkv, Nq, D, ps = 2, 2, 4, 64, 16
    k_new, v_new = al.new_rows(Bn, Hkv, Nq, D, seed=1)
    table, P = al.make_table(Bn, 8, seed=2)
    lens = torch.tensor([100, 17], dtype=torch.int32)
    kp, vp = al.sentinel_pools(P, Hkv, ps, D, kv8=False)
    kp8, vp8 = al.sentinel_pools(P, Hkv, ps, D, kv8=True)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    want = (Bn, Hkv, Nq, P, ps, 8, D)
    assert capi._kv_append_args(k_new, v_new, kp, vp, table, lens) == want
    assert capi._kv_append_args(k_new, v_new, kp8, vp8, table, lens, ks, vs, kv8=True) == want
    assert capi._kv_append_args(k_new, v_new, kp8, vp8, table, lens, None, None, kv8=True) == want
    assert capi._kv_append_args(k_new, v_new, kp8.view(torch.float8_e4m3fn), vp8.view(torch.float8_e4m3fn), table, lens, ks, None, kv8=True) == want
    with pytest.raises(RuntimeError, match="MI355X"):           # CPU tensors: no CPU path
        capi.kv_append_paged(k_new, v_new, kp, vp, table, lens)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.kv_append_paged_kv8(k_new, v_new, kp8, vp8, table, lens, ks, vs)
    for bad, kv8 in (((k_new.float(), v_new, kp, vp, table, lens), False), ((k_new, v_new.float(), kp, vp, table, lens), False),
                     ((k_new, v_new, kp8, vp8, table, lens), False), ((k_new, v_new, kp, vp.float(), table, lens), False),
                     ((k_new, v_new, kp, vp, table.long(), lens), False), ((k_new, v_new, kp, vp, table, lens.long()), False),
                     ((k_new, v_new, kp, vp, table, lens, ks, vs), True), ((k_new, v_new, kp8, vp8.to(torch.int8), table, lens, ks, vs), True),
                     ((k_new, v_new, kp8, vp8.view(torch.float8_e5m2), table, lens, ks, vs), True),
                     ((k_new, v_new, kp8, vp8, table, lens, ks.double(), vs), True), ((k_new, v_new, kp8, vp8, table, lens, ks, vs.half()), True)):
        with pytest.raises(TypeError):
            capi._kv_append_args(*bad, kv8=kv8)
    for bad, kv8 in (((k_new, v_new[:, :, :3].contiguous(), kp, vp, table, lens), False), ((k_new[0], v_new[0], kp, vp, table, lens), False),
                     ((k_new, v_new, kp, vp[:P - 1].contiguous(), table, lens), False), ((k_new, v_new, kp[:, :1].contiguous(), vp[:, :1].contiguous(), table, lens), False),
                     ((k_new, v_new, kp[..., :32].contiguous(), vp[..., :32].contiguous(), table, lens), False),
                     ((k_new, v_new, kp, vp, table[:1], lens), False), ((k_new, v_new, kp, vp, None, lens), False),
                     ((k_new, v_new, kp, vp, table, None), False), ((k_new, v_new, kp, vp, table, torch.zeros(3, dtype=torch.int32)), False),
                     ((k_new, v_new, kp8, vp8, table, lens, scales(K_SCALES, 3), vs), True), ((k_new, v_new, kp8, vp8, table, lens, ks, vs.view(2, 1)), True)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._kv_append_args(*bad, kv8=kv8)


def test_audit_knows_the_four_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    rep = json.loads((obj / build.AUDIT_OWN_REPORT["tu_kv_append"]).read_text())
    names = " ".join(r["kernel"] for r in rep)
    for d in (64, 128):
        assert f"kv_append_paged_kernelILi{d}E" in names and f"kv_append_paged_kv8_kernelILi{d}E" in names, d
    assert len(rep) == 4
    for r in rep:
        assert r["scratch"] == 0 and not r["violations"], r
        assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]          # plain HIP: listed for rule R2 only
        assert r["asm_loads"] == 0 and r["agpr"] == 0
    # the three existing reports keep their entry counts and know nothing of the new unit
    counts = {"isa_audit.json": None, build.AUDIT_OWN_REPORT["tu_attn_decode_paged"]: 6, build.AUDIT_OWN_REPORT["tu_attn_decode_paged_kv8"]: 6}
    for other, n in counts.items():
        text = (obj / other).read_text()
        assert "kv_append" not in text, other
        assert n is None or len(json.loads(text)) == n, other
    main = json.loads((obj / "isa_audit.json").read_text())
    assert len([r for r in main if "attn_decode" in r["kernel"]]) == 8          # (the count the decode modules read it by)


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference's own proof

@pytest.mark.parametrize("ps", al.PAGE_SIZES)
def test_append_ref_fills_a_pool_as_paginate_lays_it_out(ps):
    """a NaN pool filled by ONE left-padded call of Nq = 800, and one filled by a left-padded prefill to L - 3 plus three Nq = 1 steps, equal
    decode_lib.paginate's pool bit for bit — fp16, and quantised under per-head scales"""
    Bn, Hkv, Ncap, D = 3, 2, 1024, 64
    lens = al.LENS
    _, k, v = decode_inputs(Bn, 8, Hkv, 1, Ncap, D, seed=ps)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    for kv8 in (False, True):
        fill = 0x7F if kv8 else float("nan")
        kc, vc = (quantize(k, ks), quantize(v, vs)) if kv8 else (k, v)
        kp, vp, table = paginate(kc, vc, lens, ps, seed=5, fill=fill)
        sk, sv = (ks, vs) if kv8 else (None, None)
        one = [torch.full_like(kp, fill), torch.full_like(vp, fill)]
        al.append_ref(one[0], al.left_padded(k, lens, 800), table, lens, sk)
        al.append_ref(one[1], al.left_padded(v, lens, 800), table, lens, sv)
        assert torch.equal(al.bits(one[0]), al.bits(kp)) and torch.equal(al.bits(one[1]), al.bits(vp))
        steps = [torch.full_like(kp, fill), torch.full_like(vp, fill)]
        short = [x - 3 for x in lens]
        al.append_model(steps[0], steps[1], al.left_padded(k, short, 800), al.left_padded(v, short, 800), table, short, sk, sv)
        for step in range(3):
            now = [x + step + 1 for x in short]
            kn = torch.stack([k[b, :, now[b] - 1:now[b]] for b in range(Bn)])
            vn = torch.stack([v[b, :, now[b] - 1:now[b]] for b in range(Bn)])
            al.append_model(steps[0], steps[1], kn, vn, table, now, sk, sv)
        assert torch.equal(al.bits(steps[0]), al.bits(kp)) and torch.equal(al.bits(steps[1]), al.bits(vp))


# ------------------------------------------------------------------------------------------------------------------------------------
# a test of the GPU tests' inputs

def _pools_after(inputs, kv8, k_scale, v_scale, fault):
    k_new, v_new, table, P, lens = inputs[:5]
    kp, vp = al.sentinel_pools(P, k_new.shape[1], (al.NCAP // table.shape[1]), k_new.shape[3], kv8)
    return al.append_model(kp, vp, k_new, v_new, table, lens, k_scale, v_scale, fault)


def _differs(a, b):
    return not (torch.equal(al.bits(a[0]), al.bits(b[0])) and torch.equal(al.bits(a[1]), al.bits(b[1])))


@pytest.mark.parametrize("ps", al.PAGE_SIZES)
@pytest.mark.parametrize("D", al.DS)
def test_wrong_placement_or_wrong_operand_changes_the_pools_of_the_grid(D, ps):
    """on EVERY case of the GPU grid: K and V swapped, kv_len taken as the length before the append, row p % 16 (page sizes above 16); with
    scales: the two scale arrays swapped, head 0's scale for every head"""
    ks, vs = al.kind_scales("kv8")
    for Nq in al.GRID_NQ:
        inputs = al.grid_inputs(D, ps, Nq)
        for kv8, sk, sv in ((False, None, None), (True, ks, vs), (True, None, None)):
            ref = _pools_after(inputs, kv8, sk, sv, None)
            for fault in ["kv_swapped", "len_before"] + (["scales_swapped", "head0_scale"] if sk is not None else []):
                assert _differs(_pools_after(inputs, kv8, sk, sv, fault), ref), (fault, D, ps, Nq, kv8)
            # row p % 16 shows wherever a token's row inside its page is 16 or more: on every case with Nq >= 4 at page sizes above 16 (with
            # Nq = 1 the three tokens sit at positions 776, 128 and 64: rows 8, 0, 0 of a 64-key page), never at page size 16
            rows = [p % ps for L in al.LENS for p in range(max(L - Nq, 0), L)]
            assert _differs(_pools_after(inputs, kv8, sk, sv, "row_mod16"), ref) == (max(rows) >= 16), (D, ps, Nq, kv8)
            assert (max(rows) >= 16) == (ps > 16 and (Nq >= 4 or ps == 256))


@pytest.mark.parametrize("ps", al.PAGE_SIZES)
def test_a_clamped_page_id_changes_the_pools_of_the_table_test(ps):
    D = 64
    inputs = al.table_inputs(D, ps)
    table, P, dropped = inputs[2], inputs[3], inputs[5]
    assert sorted(int(x) for x in table.flatten() if not 0 <= int(x) < P) == [-1, P, 2 ** 31 - 1]
    assert all(dropped[b] for b in range(al.B))                 # every batch entry loses tokens
    for kv8 in (False, True):
        ref = _pools_after(inputs, kv8, None, None, None)
        assert _differs(_pools_after(inputs, kv8, None, None, "clamped_page"), ref)
        written = (al.bits(ref[0]) != (al.SENT8 if kv8 else al.SENT16)).any(dim=-1).any(dim=1).sum()      # (page, row) pairs that hold a token
        want = sum(len(range(max(L - 100, 0), L)) - len(dropped[b]) for b, L in enumerate(al.LENS))
        assert int(written) == want


def test_a_reciprocal_a_missing_clamp_or_fnuz_codes_change_the_codes_of_all_fp16_values():
    """every fp16 value under the per-head scales of GPU test 4.  Multiplying by the rounded reciprocal gives another code than dividing on
    some input under the scale 0.3 (an 11-bit input over a non-power-of-two scale lands on a rounding tie of e4m3 only rarely: the counts are
    printed) and under no power of two; without the clamp 0x7E becomes 0x7F; e4m3fnuz codes differ nearly everywhere"""
    inputs = al.all_values_inputs()
    k_new, v_new, ks, vs = inputs[0], inputs[1], inputs[5], inputs[6]
    ref = _pools_after(inputs, True, ks, vs, None)
    for fault in ("reciprocal", "no_clamp", "fnuz", "scales_swapped", "head0_scale", "kv_swapped"):
        assert _differs(_pools_after(inputs, True, ks, vs, fault), ref), fault
    moved = {}
    for x, sc in ((k_new, al.ALL_K_SCALES), (v_new, al.ALL_V_SCALES)):
        for h, s in enumerate(sc):
            xs = x[:, h:h + 1]
            good, recip, raw = al._codes(xs, s, None), al._codes(xs, s, "reciprocal"), al._codes(xs, s, "no_clamp")
            finite = ~torch.isnan(xs.float())
            n = int((good != recip)[finite].sum())
            pow2 = float(torch.tensor(s).log2()) == int(torch.tensor(s).log2())
            assert n == 0 or not pow2, (s, n)                            # a power of two: the reciprocal is exact
            moved[s] = n
            print(f"[kv append] scale {s:.6g}: {n} of 65536 fp16 values get another code from x * (1 / s)")
            over = finite & ((xs.float() / s).abs() > 464.0)            # beyond the last value that rounds to 448
            assert over.any() and ((good[over] & 0x7F) == 0x7E).all() and ((raw[over] & 0x7F) == 0x7F).all(), s
            assert sorted(set(good[finite].tolist())) == [c for c in range(256) if c & 0x7F != 0x7F], s      # all 254 finite codes are reached
    assert moved[0.3] >= 1 and all(moved[s] == 0 for s in (1.0, 2.0 ** -3, 4.0, 2.0 ** 2, 2.0 ** -5))
