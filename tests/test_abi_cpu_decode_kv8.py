"""CPU tests of fp8-cache paged decode attention's boundary (lc_attn_decode_paged_kv8, lc_attn_decode_paged_kv8_kernel_name,
lc_attn_decode_paged_kv8_workspace_bytes; no call here reaches a device): the error codes and their order (NULL scales are accepted), the name
grid, S and the workspace bytes against the fp16 paged call of the same shape, the Python shape and dtype checks, the audit report of the six
new kernels, the exactness of the quantisation helpers — and a test of the GPU tests' pinned inputs: on their quantised form a kernel that
ignores k_scale, ignores v_scale, swaps the two, uses head 0's scales for every head, decodes the bytes as e4m3fnuz (bias 8), swaps the two
fp16 chunks of one fp8 V chunk or takes K bytes 8 s .. 8 s + 7 in the wrong k-step leaves the bound by >= 20 x on EVERY row it touches.

`quantize` / `dequant`, the per-head scales and the float64 reference are shared with tests/test_gpu_decode_kv8.py: tests/decode_lib.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests.decode_lib import (FINITE_CODES, FNUZ, K_SCALES, NAN_BYTE, OCP, PIN_LENS, PIN_NQ, PIN_SHAPE, TEETH, V_SCALES, _moved, _wrong_kernel,
                              auto_split, decode_inputs, decode_truth, dequant, dequant64, paginate, quantize, reset_knobs, rt_of, scales,
                              seam_inputs_kv8, softmax64)
from tests.decode_lib import name_kv8 as _name

# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def knobs(built):
    yield from reset_knobs()


def test_kv8_errors_and_their_order(built):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    c, vt = capi.ATTN_CAUSAL, capi.ATTN_V_TRANSPOSED
    p = C.c_void_p(16)
    ok = (1, 8, 2, 4, 70, 16, 64, 128)        # B, H, Hkv, Nq, num_pages, page_size, max_pages, D
    bad_shape = (1, 8, 3, 4, 70, 16, 64, 256)
    for sc in ((p, p), (None, None), (p, None), (None, p)):      # the scales may be NULL: the same code either way
        def f(*a, sc=sc):
            return lib.lc_attn_decode_paged_kv8(*a[:6], *sc, *a[6:])
        for flags in (0, c):
            for nul in range(6):                  # Q, Kpool8, Vpool8, O, block_table, kv_len
                ptrs = [p] * 6
                ptrs[nul] = None
                assert f(*ptrs, *ok, flags, None, 0, None) == capi.LC_ERR_ARG, nul
                assert f(*ptrs, *bad_shape, flags, None, 0, None) == capi.LC_ERR_ARG      # null pointer before shape and head dim
            for hkv in (0, -1, 3, 5, 9, 16):
                assert f(*[p] * 6, 1, 8, hkv, 4, 70, 16, 64, 128, flags, None, 0, None) == capi.LC_ERR_SHAPE, hkv
            for shape in ((0, 8, 2, 4, 70, 16, 64, 128), (1, 0, 0, 4, 70, 16, 64, 128), (1, 8, 2, 0, 70, 16, 64, 128), (1, 8, 2, 4, 0, 16, 64, 128),
                          (1, 8, 2, 4, -3, 16, 64, 128), (1, 8, 2, 4, 70, 16, 0, 128), (1, 8, 2, 4, 70, 16, -1, 128), (1, 8, 2, 4, 70, 16, 64, 0),
                          (1, 8, 2, 4, 70, 8, 64, 128), (1, 8, 2, 4, 70, 24, 64, 128), (1, 8, 2, 4, 70, 0, 64, 128), (1, 8, 2, 4, 70, -16, 64, 128),
                          (1, 8, 2, 4, 70, 1, 64, 128), (1, 8, 2, 4, 70, 48, 64, 128),
                          (1, 8, 2, 17, 70, 16, 64, 128), (1, 8, 8, 65, 70, 16, 64, 64), (1, 64, 1, 2, 70, 16, 64, 64),
                          (1, 8, 2, 4, 70, 16, 1 << 20, 128), (1, 8, 2, 4, 70, 1 << 21, 16, 64), (1, 8, 2, 4, 70, 1 << 16, 1 << 16, 64),
                          (1 << 24, 8, 8, 1, 70, 16, 64, 64)):
                assert f(*[p] * 6, *shape, flags, None, 0, None) == capi.LC_ERR_SHAPE, shape
                assert _name(*shape[:4], *shape[5:], flags)[0] == capi.LC_ERR_SHAPE or shape[4] <= 0, shape      # (the name call takes no num_pages)
                assert lib.lc_attn_decode_paged_kv8_workspace_bytes(*shape[:4], *shape[5:]) == 0 or shape[4] <= 0
            assert f(*[p] * 6, *bad_shape, flags, None, 0, None) == capi.LC_ERR_SHAPE                           # shape before head dim
            assert f(*[p] * 6, 1, 8, 2, 4, 70, 24, 64, 96, flags, None, 0, None) == capi.LC_ERR_SHAPE           # page size before head dim
            assert f(*[p] * 6, 1, 8, 2, 17, 70, 16, 64, 96, flags, None, 0, None) == capi.LC_ERR_SHAPE          # R > 64 before head dim
            for mis in range(4):                                                                               # Q, pools, O: 16-byte aligned
                ptrs = [p] * 6
                ptrs[mis] = C.c_void_p(8)
                assert f(*ptrs, *ok, flags, None, 0, None) == capi.LC_ERR_SHAPE, mis
                assert f(*ptrs, 1, 8, 2, 4, 70, 16, 64, 96, flags, None, 0, None) == capi.LC_ERR_SHAPE          # alignment before head dim
            for d in (32, 96, 256, 512, 1024, 16, 48):
                assert f(*[p] * 6, 1, 8, 2, 4, 70, 16, 64, d, flags, None, 0, None) == capi.LC_ERR_HEADDIM, d
                assert _name(1, 8, 2, 4, 16, 64, d, flags)[0] == capi.LC_ERR_HEADDIM
                assert lib.lc_attn_decode_paged_kv8_workspace_bytes(1, 8, 2, 4, 16, 64, d) == 0
        for bad in (vt, c | vt, 4, -1, 1 << 30):
            assert f(*[p] * 6, *ok, bad, None, 0, None) == capi.LC_ERR_ARG, bad
            assert f(*[p] * 6, *bad_shape, bad, None, 0, None) == capi.LC_ERR_ARG                               # flags before everything
            assert f(None, p, p, p, p, p, *ok, bad, None, 0, None) == capi.LC_ERR_ARG
            assert _name(1, 8, 2, 4, 16, 64, 128, bad)[0] == capi.LC_ERR_ARG
            assert _name(1, 8, 3, 4, 24, 64, 256, bad)[0] == capi.LC_ERR_ARG
    assert _name(1, 8, 3, 4, 16, 64, 256)[0] == capi.LC_ERR_SHAPE
    assert _name(1, 8, 2, 4, 8, 64, 128)[0] == capi.LC_ERR_SHAPE
    assert lib.lc_attn_decode_paged_kv8_kernel_name(1, 8, 2, 4, 16, 64, 128, 0, None, 128) == capi.LC_ERR_ARG
    assert lib.lc_attn_decode_paged_kv8_kernel_name(1, 8, 2, 4, 16, 64, 128, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
    rc, name = _name(1, 8, 2, 4, 16, 64, 128)
    assert rc == capi.LC_OK and name.startswith("attn_decode_paged_kv8_kernel<128,1>")


def test_the_span_bound_is_that_of_one_byte_elements(built):
    """max_pages x page_size x D below 2 GiB of BYTES: twice the logical length the fp16 call takes, and not one row more"""
    lib = capi.load()
    for ps, mp, D in ((16, 1 << 19, 128), (1 << 20, 16, 64)):        # 2^30 elements: 2 GiB of halves, 1 GiB of bytes
        assert lib.lc_attn_decode_paged_workspace_bytes(1, 8, 2, 4, ps, mp, D) == 0
        assert _name(1, 8, 2, 4, ps, mp, D)[0] == capi.LC_OK
        assert _name(1, 8, 2, 4, ps, 2 * mp - 1, D)[0] == capi.LC_OK
        assert _name(1, 8, 2, 4, ps, 2 * mp, D)[0] == capi.LC_ERR_SHAPE


def test_a_small_or_misaligned_workspace_is_refused_before_any_device_work(knobs):
    lib = capi.load()
    p = C.c_void_p(16)
    capi.tune("attn_decode_split", 4)
    need = lib.lc_attn_decode_paged_kv8_workspace_bytes(1, 8, 2, 4, 16, 64, 128)
    assert need == 4 * (1 * 8 * 4) * 129 * 4
    f = lib.lc_attn_decode_paged_kv8
    for sc in ((p, p), (None, None)):
        for nbytes in (0, 16, need - 1):
            assert f(*[p] * 6, *sc, 1, 8, 2, 4, 70, 16, 64, 128, 0, C.c_void_p(256), nbytes, None) == capi.LC_ERR_ARG, nbytes
        assert f(*[p] * 6, *sc, 1, 8, 2, 4, 70, 16, 64, 128, 0, C.c_void_p(8), need, None) == capi.LC_ERR_ARG
        assert f(*[p] * 6, *sc, 1, 8, 2, 4, 70, 16, 64, 96, 0, C.c_void_p(256), 0, None) == capi.LC_ERR_HEADDIM    # head dim before the workspace
        assert f(*[p] * 6, *sc, 1, 8, 2, 4, 70, 24, 64, 128, 0, C.c_void_p(256), 0, None) == capi.LC_ERR_SHAPE


def test_name_grid_head_dim_row_tiles_and_split_suffix(knobs):
    for D in (64, 128):
        for (B, H, Hkv), Nq in (((3, 8, 2), 1), ((3, 8, 2), 4), ((3, 8, 2), 5), ((3, 8, 2), 8), ((3, 8, 2), 9), ((3, 8, 2), 16), ((2, 4, 1), 1),
                                ((2, 4, 1), 5), ((2, 4, 1), 16), ((2, 4, 4), 16), ((2, 4, 4), 17), ((2, 4, 4), 33), ((2, 4, 4), 64), ((1, 64, 1), 1)):
            rt = rt_of(H, Hkv, Nq)
            for flags in (0, capi.ATTN_CAUSAL):
                for ps, mp in ((16, 64), (256, 4), (1024, 1)):
                    for s in (1, 2, 3, 8, 64):
                        capi.tune("attn_decode_split", s)
                        want = f"attn_decode_paged_kv8_kernel<{D},{rt}>" + (f" x{s}" if s > 1 else "")
                        assert _name(B, H, Hkv, Nq, ps, mp, D, flags) == (capi.LC_OK, want)
                        assert capi.attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=bool(flags)) == want
                        assert capi.attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == (s * B * H * Nq * (D + 1) * 4 if s > 1 else 0)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_auto_split_and_workspace_are_those_of_the_fp16_paged_call(knobs, cus):
    """no new rule and no new knob: the suffix and the bytes of lc_attn_decode_paged_* for the same shape"""
    capi.tune("rule_cus", cus)
    for B, H, Hkv, Nq, ps, mp, D in ((1, 32, 8, 1, 16, 512, 128), (1, 32, 8, 1, 8192, 1, 128), (16, 32, 8, 1, 64, 64, 128), (64, 32, 8, 1, 256, 8, 128),
                                     (4, 64, 8, 1, 16, 2048, 128), (8, 32, 8, 4, 128, 32, 128), (8, 32, 32, 1, 16, 256, 64), (1, 8, 1, 1, 1024, 1024, 64),
                                     (1, 8, 8, 1, 16, 15, 64), (1, 8, 8, 1, 16, 16, 64), (1, 8, 2, 1, 16, 64, 128), (3, 8, 2, 5, 64, 16, 128),
                                     (1, 1, 1, 1, 16, 1, 64), (1, 1, 1, 1, 16, 31, 128), (1, 1, 1, 1, 16, 32, 128), (300, 8, 1, 1, 32, 128, 64)):
        s = auto_split(B * Hkv, ps * mp, cus)
        rc, name = _name(B, H, Hkv, Nq, ps, mp, D)
        assert rc == capi.LC_OK
        assert name == f"attn_decode_paged_kv8_kernel<{D},{rt_of(H, Hkv, Nq)}>" + (f" x{s}" if s > 1 else ""), (B, Hkv, ps, mp, cus, s, name)
        assert name.replace("_kv8", "") == capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D)
        assert capi.attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == capi.attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D)
        assert capi.attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == (s * B * H * Nq * (D + 1) * 4 if s > 1 else 0)


def test_capi_wrapper_checks_shapes_and_dtypes_without_a_gpu(built):
    q, k, v = decode_inputs(2, 8, 2, 4, 128, 64, seed=1)
    o = torch.empty_like(q)
    lens = torch.tensor([100, 17], dtype=torch.int32)
    ks, vs = scales(K_SCALES, 2), scales(V_SCALES, 2)
    kp, vp, table = paginate(quantize(k, ks), quantize(v, vs), (100, 17), 16, seed=2, fill=NAN_BYTE)
    assert kp.dtype == torch.uint8 and tuple(kp.shape) == (2 * 8 + 3, 2, 16, 64)
    want = (2, 8, 2, 4, 19, 16, 8, 64)
    assert capi._kv8_args(q, kp, vp, o, table, lens, ks, vs) == want
    assert capi._kv8_args(q, kp, vp, o, table, lens, None, None) == want
    assert capi._kv8_args(q, kp.view(torch.float8_e4m3fn), vp.view(torch.float8_e4m3fn), o, table, lens, ks, None) == want
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_decode_paged_kv8(q, kp, vp, o, table, lens, ks, vs)
    for bad in ((q.float(), kp, vp, o, table, lens, ks, vs), (q, kp.half(), vp, o, table, lens, ks, vs), (q, kp, vp.to(torch.int8), o, table, lens, ks, vs),
                (q, kp, vp.view(torch.float8_e5m2), o, table, lens, ks, vs), (q, kp, vp, o.float(), table, lens, ks, vs),
                (q, kp, vp, o, table.long(), lens, ks, vs), (q, kp, vp, o, table, lens.long(), ks, vs), (q, kp, vp, o, table, lens, ks.double(), vs),
                (q, kp, vp, o, table, lens, ks, vs.half())):
        with pytest.raises(TypeError):
            capi._kv8_args(*bad)
    for bad in ((q, kp, vp[:18].contiguous(), o, table, lens, ks, vs), (q, kp, vp[:, :, :8].contiguous(), o, table, lens, ks, vs),
                (q, kp, vp, o[:, :, :3].contiguous(), table, lens, ks, vs), (q, kp, vp, o, table[:1], lens, ks, vs), (q, kp, vp, o, None, lens, ks, vs),
                (q, kp, vp, o, table, torch.zeros(3, dtype=torch.int32), ks, vs), (q, kp, vp, o, table, lens, scales(K_SCALES, 3), vs),
                (q, kp, vp, o, table, lens, ks, vs.view(2, 1)), (q, kp, vp, o, table, lens, ks, scales(V_SCALES, 1))):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._kv8_args(*bad)


def test_audit_knows_the_kv8_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    rep = json.loads((obj / build.AUDIT_OWN_REPORT["tu_attn_decode_paged_kv8"]).read_text())
    dec = [r for r in rep if "attn_decode_paged_kv8_kernel" in r["kernel"]]
    names = " ".join(r["kernel"] for r in dec)
    for d in (64, 128):
        for rt in (1, 2, 4):
            assert f"attn_decode_paged_kv8_kernelILi{d}ELi{rt}E" in names, (d, rt)
    assert len(dec) == 6 and len(rep) == 6
    for r in dec:
        assert r["scratch"] == 0 and not r["violations"], r
        assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]          # plain HIP: listed for rule R2 only
        assert r["asm_loads"] == 0
    for other in ("isa_audit.json", build.AUDIT_OWN_REPORT["tu_attn_decode_paged"]):      # the reports that are read by entry counts keep theirs
        assert "kv8" not in (obj / other).read_text()


def test_dequant_is_exact_and_every_value_a_normal_fp16():
    """the 254 finite codes under every power-of-two scale 2^-5 .. 2^2: dequant's fp16 is the exact product, zero or a NORMAL fp16 (the smallest
    e4m3 magnitude 2^-9 times 2^-5 is fp16's smallest normal 2^-14), and quantize brings every code back"""
    assert torch.equal(OCP[FINITE_CODES.long()], FINITE_CODES.view(torch.float8_e4m3fn).float())        # the table is torch's e4m3fn
    assert torch.isnan(OCP[0x7F]) and torch.isnan(OCP[0xFF]) and FINITE_CODES.numel() == 254
    assert float(OCP[1]) == 2.0 ** -9 and float(OCP[0x7E]) == 448.0
    for e in range(-5, 3):
        s = 2.0 ** e
        h = dequant(FINITE_CODES, s)
        assert torch.equal(h.double(), OCP[FINITE_CODES.long()].double() * s)
        mag = h.abs().float()
        assert ((mag == 0) | (mag >= 2.0 ** -14)).all() and torch.isfinite(h).all()
        back = quantize(h, s)
        same = back == FINITE_CODES
        assert (same | ((FINITE_CODES & 0x7F) == 0)).all()          # (+-0: the sign of a zero is torch's business)
        assert torch.equal(dequant(back, s), h)
    assert float(dequant(torch.tensor([1], dtype=torch.uint8), 2.0 ** -5)) == 2.0 ** -14
    for hkv in (1, 2, 4):                                            # the per-head scales of the GPU tests are such scales, pairwise different
        ks, vs = K_SCALES[:hkv], V_SCALES[:hkv]
        assert all(2.0 ** -5 <= s <= 4.0 and np.log2(s) == int(np.log2(s)) for s in ks + vs)
        assert len(set(ks)) == hkv and len(set(vs)) == hkv and all(a != b for a, b in zip(ks, vs))
    # quantize rounds to nearest and saturates instead of making NaN
    x = torch.tensor([[[[0.3, -1000.0, 1e-4, 448.0]]]]).half()
    assert torch.equal(dequant(quantize(x, 1.0), 1.0).float(), torch.tensor([[[[0.3125, -448.0, 0.0, 448.0]]]]))
    # per-head scales broadcast over [B, Hkv, rows, D]
    y = torch.ones(2, 2, 3, 4).half()
    assert torch.equal(dequant(quantize(y, scales(K_SCALES, 2)), scales(K_SCALES, 2)), y)
    assert torch.equal(OCP[quantize(y, scales(K_SCALES, 2)).long()][0, :, 0, 0], torch.tensor([8.0, 2.0]))


def test_the_float64_reference_agrees_with_the_oracle(oracle):
    """tests/test_gpu_decode_kv8.py checks non-power-of-two scales against softmax64 under tol.attn_close unchanged.  That bound was made for
    the oracle's truth, so the two references are compared here on one power-of-two case (where the dequantised cache is fp16 and the oracle
    can be asked): worst |softmax64 - decode_truth| / bound = 1.03e-05 (D = 64, causal, lens (300, 65); printed below), the oracle's own
    rounding — the bound carries over"""
    B, H, Hkv, Nq, D = 2, 4, 2, 5, 64
    lens = (300, 65)
    q, k, v = decode_inputs(B, H, Hkv, Nq, 320, D, seed=64)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    truth, nks = decode_truth(oracle, q, dequant(k8, ks), dequant(v8, vs), lens, True)
    ref, nks64 = softmax64(q, dequant64(k8, ks), dequant64(v8, vs), lens, True)
    assert (nks == nks64).all()
    worst = float(_moved(truth, nks, ref).max())
    print(f"[decode kv8] float64 reference against the oracle: worst |err| / bound {worst:.2e}")
    assert worst <= 0.05


# ------------------------------------------------------------------------------------------------------------------------------------
# a test of the GPU tests' inputs

def _swap_d(x, bit):
    """x[..., d ^ bit]"""
    return x[..., torch.arange(x.shape[-1]) ^ bit]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_a_wrong_scale_format_or_byte_order_moves_every_row_it_touches(oracle, D, causal):
    B, H, Hkv = PIN_SHAPE
    Nq, G = PIN_NQ, H // Hkv
    q, k8, v8, ks, vs, lens = seam_inputs_kv8(D, causal)
    assert lens == PIN_LENS
    k, v = dequant(k8, ks), dequant(v8, vs)
    truth, nks = decode_truth(oracle, q, k, v, lens, causal)
    every = np.ones((B, H, Nq), bool)
    head_moves = np.array([[[h // G != 0] * Nq for h in range(H)] for _ in range(B)])
    one = torch.ones(Hkv)
    variants = {       # name -> (the cache a wrong kernel sees, the rows it touches)
        "k_scale ignored": (dequant(k8, one), v, every),
        "v_scale ignored": (k, dequant(v8, one), every),
        "k_scale and v_scale swapped": (dequant(k8, vs), dequant(v8, ks), every),
        "head 0's scales for every head": (dequant(k8, ks[:1].expand(Hkv)), dequant(v8, vs[:1].expand(Hkv)), head_moves),
        "e4m3fnuz (bias 8) decoding": (dequant(k8, ks, FNUZ), dequant(v8, vs, FNUZ), every),
        "the two fp16 chunks of an fp8 V chunk swapped": (k, _swap_d(v, 8), every),
        # a lane holds D / 4 contiguous K bytes; k-step s is bytes 8 s .. 8 s + 7 of them, against Q elements 8 s .. of the same quarter
        "K bytes of k-step s ^ 1 in k-step s": (_swap_d(k, 8), v, every),
    }
    assert (_wrong_kernel(oracle, q, k, v, lens, causal, truth, nks) == 0).all()
    smallest = np.inf
    for name, (kw, vw, touched) in variants.items():
        ratio = _wrong_kernel(oracle, q, kw, vw, lens, causal, truth, nks)
        assert touched.any(), name
        smallest = min(smallest, float(ratio[touched].min()))
        assert ratio[touched].min() >= TEETH, (name, D, causal, float(ratio[touched].min()))
        assert ratio[~touched].max(initial=0.0) == 0.0, name
    print(f"[decode kv8] D={D} causal={causal}: the smallest factor over the bound of a wrong kernel {smallest:.1f}")
