"""CPU tests of causal attention's plan (lc_attn_kernel_name_ex never launches): which kernel a causal call reaches, its error codes,
and that the _ex entries without LC_ATTN_CAUSAL report exactly what lc_attn_kernel_name_bh does."""
import ctypes as C
import json

import pytest

from leetcuda_amd import capi


def _name_ex(bh, n, d, flags):
    buf = C.create_string_buffer(128)
    rc = capi.load().lc_attn_kernel_name_ex(bh, n, d, flags, buf, 128)
    return rc, buf.value.decode()


def _name_bh(bh, n, d, vt):
    buf = C.create_string_buffer(128)
    rc = capi.load().lc_attn_kernel_name_bh(bh, n, d, vt, 0, buf, 128)
    return rc, buf.value.decode()


def test_flag_values_are_pinned(built):
    assert (capi.ATTN_CAUSAL, capi.ATTN_V_TRANSPOSED) == (1, 2)
    assert capi.load().lc_abi_version() == 2          # additive: the ABI version stays


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("vt", [False, True])
def test_merged_phase_causal_for_d64_d128_at_any_batch(built, d, vt):
    flags = capi.ATTN_CAUSAL | (capi.ATTN_V_TRANSPOSED if vt else 0)
    want = f"attn_fwd_w4u_causal_kernel<{d},{'true' if vt else 'false'}>"
    for n in (256, 512, 1024, 4096, 8192):
        names = {_name_ex(bh, n, d, flags) for bh in (-1, 1, 2, 48, 4096)}
        assert names == {(capi.LC_OK, want)}, (n, names)   # the same kernel at B x H = 1 and 4096: no grid-size switch
    assert capi.attn_kernel_name(4096, d, v_transposed=vt, causal=True) == want
    assert capi.attn_kernel_name(4096, d, v_transposed=vt, bh=1, causal=True) == want


@pytest.mark.parametrize("vt", [False, True])
def test_lockstep_causal_for_the_other_cases(built, vt):
    v = "true" if vt else "false"
    flags = capi.ATTN_CAUSAL | (capi.ATTN_V_TRANSPOSED if vt else 0)
    for d in (32, 96):
        for bh in (-1, 1, 4096):
            assert _name_ex(bh, 1024, d, flags) == (capi.LC_OK, f"attn_fwd_causal_kernel<{d},8,{v}>")
            assert _name_ex(bh, 384, d, flags) == (capi.LC_OK, f"attn_fwd_causal_kernel<{d},4,{v}>")
            assert _name_ex(bh, 192, d, flags) == (capi.LC_OK, f"attn_fwd_causal_kernel<{d},2,{v}>")
    for d in (64, 128):          # N % 256 != 0: the lock-step kernel, whatever N is
        for n, nw in ((64, 2), (128, 4), (192, 2), (320, 2), (1152, 4), (4160, 2)):
            assert _name_ex(1, n, d, flags) == (capi.LC_OK, f"attn_fwd_causal_kernel<{d},{nw},{v}>"), n


@pytest.mark.parametrize("nw", [8, 4, 2])
def test_attn_nw_forces_the_lockstep_cross_check(built, nw):
    old = capi.tune_get("attn_nw")[0]
    capi.tune("attn_nw", nw)
    try:
        for d in (64, 128):
            for vt in (0, capi.ATTN_V_TRANSPOSED):
                v = "true" if vt else "false"
                assert _name_ex(8, 4096, d, capi.ATTN_CAUSAL | vt) == (capi.LC_OK, f"attn_fwd_causal_kernel<{d},{nw},{v}>")
    finally:
        capi.tune("attn_nw", old)
    for want in (513, 515, 517, 514):           # the merged-phase selections keep the causal merged-phase kernel
        capi.tune("attn_nw", want)
        try:
            assert _name_ex(8, 4096, 128, capi.ATTN_CAUSAL) == (capi.LC_OK, "attn_fwd_w4u_causal_kernel<128,false>")
        finally:
            capi.tune("attn_nw", old)


def test_causal_order_knob_changes_no_name(built):
    assert capi.tune_get("attn_causal_order") == (0, 0)
    for bad in (-1, 3):
        assert capi.load().lc_tune_set(b"attn_causal_order", bad) == capi.LC_ERR_ARG
    for order in (1, 2):
        capi.tune("attn_causal_order", order)
        try:
            assert _name_ex(32, 4096, 128, capi.ATTN_CAUSAL) == (capi.LC_OK, "attn_fwd_w4u_causal_kernel<128,false>")
        finally:
            capi.tune("attn_causal_order", 0)


def test_causal_errors(built):
    lib = capi.load()
    c = capi.ATTN_CAUSAL
    for d in (256, 512, 1024, 16, 48, 0):
        assert _name_ex(4, 1024, d, c)[0] == capi.LC_ERR_HEADDIM, d
        assert _name_ex(4, 1024, d, c | capi.ATTN_V_TRANSPOSED)[0] == capi.LC_ERR_HEADDIM, d
    for n in (96, 100, 1000, 4100):
        assert _name_ex(4, n, 128, c)[0] == capi.LC_ERR_SHAPE, n   # (the code the causal launch returns)
    for bad in (4, 8, 1 << 30, -1, c | 4):
        assert _name_ex(4, 1024, 128, bad)[0] == capi.LC_ERR_ARG, bad
    # the launch entry: argument checks before any device work (no GPU is touched on these paths)
    p = C.c_void_p(16)
    assert lib.lc_attn_fwd_f16_ex(p, p, p, p, 1, 1, 1024, 128, 4, None) == capi.LC_ERR_ARG
    assert lib.lc_attn_fwd_f16_ex(p, p, p, p, 1, 1, 1024, 128, -1, None) == capi.LC_ERR_ARG
    assert lib.lc_attn_fwd_f16_ex(None, p, p, p, 1, 1, 1024, 128, c, None) == capi.LC_ERR_ARG
    assert lib.lc_attn_fwd_f16_ex(p, p, p, p, 1, 1, 1000, 128, c, None) == capi.LC_ERR_SHAPE   # N % 64 != 0
    assert lib.lc_attn_fwd_f16_ex(p, p, p, p, 1, 1, 100, 256, c, None) == capi.LC_ERR_SHAPE    # (shape first, as lc_attn_fwd_f16)
    assert lib.lc_attn_fwd_f16_ex(p, p, p, p, 0, 1, 1024, 128, c, None) == capi.LC_ERR_SHAPE
    for flags in (0, capi.ATTN_V_TRANSPOSED):   # without the mask: lc_attn_fwd_f16's checks
        assert lib.lc_attn_fwd_f16_ex(p, p, p, p, 1, 1, 1000, 128, flags, None) == capi.LC_ERR_SHAPE
        assert lib.lc_attn_fwd_f16_ex(None, p, p, p, 1, 1, 1024, 128, flags, None) == capi.LC_ERR_ARG


def test_non_causal_flags_name_what_lc_attn_kernel_name_bh_names(built):
    for vt in (0, 1):
        flags = capi.ATTN_V_TRANSPOSED if vt else 0
        for bh in (-1, 1, 2, 8, 24, 64, 256, 4096):
            for n in (64, 128, 192, 256, 384, 1024, 1152, 2048, 4096, 4224, 8192, 16384):
                for d in (32, 64, 96, 128, 256, 512, 1024, 48):
                    assert _name_ex(bh, n, d, flags) == _name_bh(bh, n, d, vt), (bh, n, d, vt)


def test_audit_report_lists_the_causal_merged_phase_kernel(built):
    """leetcuda_amd/isa_audit.py audits the causal merged-phase kernel under the rules and AGPR range of its non-causal twin."""
    rep = json.loads((built["abi"].parent / "obj" / "isa_audit.json").read_text())
    causal = [r for r in rep if "attn_fwd_w4u_causal_kernel" in r["kernel"]]
    assert len(causal) == 4, [r["kernel"] for r in causal]          # D = 64 / 128 x both V layouts
    assert all(r["scratch"] == 0 and not r["violations"] and r["compiler_accvgpr"] == 0 for r in causal)
    twin_agpr = {r["kernel"].split("ELb")[0].split("ILi")[-1]: r["agpr"] for r in rep if "attn_fwd_w4u_kernel" in r["kernel"]}
    assert all(r["agpr"] == twin_agpr[r["kernel"].split("ELb")[0].split("ILi")[-1]] for r in causal)
    from leetcuda_amd import isa_audit
    assert all(isa_audit._owned(r["kernel"]) == set(range(256)) for r in causal)
