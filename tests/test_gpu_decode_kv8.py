"""Decode attention over a paged fp8 (e4m3) KV cache on the GPU (lc_attn_decode_paged_kv8 / capi.attn_decode_paged_kv8).  Every e4m3 value is
an fp16 value and the kernel converts exactly, so with power-of-two scales correctness is (a) BIT equality with capi.attn_decode_paged — an
existing, separately tested call — on the dequantised fp16 pool under the same split, and (b) every row against the CPU oracle on the
dequantised logical cache (tests/decode_lib.py decode_truth / check_decode, tol.attn_close with N = the row's visible keys).
Non-power-of-two scales are checked against a float64 softmax on the exactly dequantised values under the same bound.  Ncap = 1024 throughout;
pools come from `paginate` on the quantised cache: scattered pages, the NaN code 0x7f in every pool byte of a position >= L_b and in the spare
page every unused table entry names.  Helpers and scales: tests/decode_lib.py."""
import functools

import numpy as np
import pytest
import torch

from tests.decode_lib import NCAP_POW2 as NCAP
from tests.decode_lib import (FINITE_CODES, GRID_SHAPES, K_SCALES, NAN_BYTE, V_SCALES, _capi, _cuda, _dev_lens, _lens_of, _oracle, check_decode,
                              decode_inputs, decode_truth, dequant, dequant64, forced_split, paginate, pinned_inputs, quantize, rt_of, scales,
                              seam_inputs_kv8, softmax64)
from tests.decode_lib import run_kv8 as _run_kv8
from tests.decode_lib import run_paged as _run_f16

pytestmark = pytest.mark.gpu


def _pools(k8, v8, lens, ps, seed, ks, vs, spare=3, fill=NAN_BYTE):
    """(kp8, vp8, table, the dequantised fp16 pools) on the GPU; the fp16 pools hold NaN exactly where the fp8 ones hold the NaN code"""
    kp8, vp8, table = paginate(k8, v8, lens, ps, seed=seed, spare=spare, fill=fill)
    return _cuda(kp8, vp8, table, dequant(kp8, ks), dequant(vp8, vs))


@functools.lru_cache(maxsize=4)
def _grid_case(D, shape, Nq, causal):
    B, H, Hkv = shape
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=D * 1000 + H * 100 + Hkv * 10 + Nq)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    lens = _lens_of(B, Hkv)
    truth, nks = decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), lens, causal)
    return q, k8, v8, ks, vs, lens, truth, nks


@functools.lru_cache(maxsize=4)
def _grid_pool(D, shape, Nq, causal, ps):
    q, k8, v8, ks, vs, lens, _, _ = _grid_case(D, shape, Nq, causal)
    return _pools(k8, v8, lens, ps, ps + Nq, ks, vs)


def _names(capi, B, H, Hkv, Nq, ps, D, split):
    return forced_split(split, lambda: (capi.attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, NCAP // ps, D),
                                        capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, NCAP // ps, D)))


@pytest.mark.parametrize("split", [0, 1, 3, 8])
@pytest.mark.parametrize("ps", [16, 64, 256])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Nq", [1, 5, 16])
@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", [64, 128])
def test_grid_bit_identical_to_the_fp16_call_on_the_dequantised_pool(D, shape, Nq, causal, ps, split):
    """per-head power-of-two scales, different between K / V heads and between K and V"""
    capi = _capi()
    B, H, Hkv = shape
    name, f16_name = _names(capi, B, H, Hkv, Nq, ps, D, split)
    assert name.startswith(f"attn_decode_paged_kv8_kernel<{D},{rt_of(H, Hkv, Nq)}>") and name.replace("_kv8", "") == f16_name
    if split == 1:
        assert " x" not in name
    elif split > 1:
        assert name.endswith(f" x{split}")
    q, k8, v8, ks, vs, lens, truth, nks = _grid_case(D, shape, Nq, causal)
    kp8, vp8, table, kp16, vp16 = _grid_pool(D, shape, Nq, causal, ps)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, name)
    assert torch.equal(out, _run_f16(capi, q, kp16, vp16, table, lens, causal, split)), name
    print(f"[decode kv8] {name} {shape} Nq={Nq} page={ps} causal={causal}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_null_scales_are_one(D, split):
    """randn rounded to e4m3 as it is (subnormal codes included), k_scale = v_scale = NULL: the fp16 call on the plainly upcast pool; and one
    NULL scale next to one given scale"""
    capi = _capi()
    B, H, Hkv, Nq = 3, 8, 2, 5
    lens = (1000, 129, 65)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=88 + D)
    k8, v8 = quantize(k, 1.0), quantize(v, 1.0)
    kp8, vp8, table, kp16, vp16 = _pools(k8, v8, lens, 16, 3, 1.0, 1.0)
    ref = _run_f16(capi, q, kp16, vp16, table, lens, True, split)
    assert torch.isfinite(ref).all()
    assert torch.equal(_run_kv8(capi, q, kp8, vp8, table, lens, None, None, True, split), ref)
    truth, nks = decode_truth(_oracle(), q, dequant(k8, 1.0), dequant(v8, 1.0), lens, True)
    check_decode(ref.float().cpu().numpy(), truth, nks, "null scales")
    vs = scales(V_SCALES, Hkv)
    assert torch.equal(_run_kv8(capi, q, kp8, vp8, table, lens, None, vs, True, split), _run_f16(capi, q, kp16, dequant(vp8.cpu(), vs), table, lens, True, split))
    ks = scales(K_SCALES, Hkv)
    assert torch.equal(_run_kv8(capi, q, kp8, vp8, table, lens, ks, None, True, split), _run_f16(capi, q, dequant(kp8.cpu(), ks), vp16, table, lens, True, split))


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("Nq", [1, 20], ids=["RT1", "RT4"])
@pytest.mark.parametrize("D", [64, 128])
def test_every_code_in_k(D, Nq, split):
    """K bytes drawn uniformly from the 254 finite codes, k_scale = 2^-5 (the smallest: code 1 is fp16's smallest normal); query rows one-hot
    in d, a different d per row: a score is ONE K element exactly.  V is quantised randn.  The fp16 call on the dequantised pool, bit for bit"""
    capi = _capi()
    B, H, Hkv = 2, 4, 2
    lens = (1000, 129)
    g = torch.Generator().manual_seed(254 + D + Nq)
    k8 = FINITE_CODES[torch.randint(0, 254, (B, Hkv, NCAP, D), generator=g)]
    for b in range(B):
        assert set(k8[b, :, :lens[b]].flatten().tolist()) == set(FINITE_CODES.tolist())
    ks, vs = torch.full((Hkv,), 2.0 ** -5), scales(V_SCALES, Hkv)
    v8 = quantize(torch.randn(B, Hkv, NCAP, D, generator=g).half(), vs)
    q = torch.zeros(B, H, Nq, D)
    for b in range(B):
        for h in range(H):
            for i in range(Nq):
                q[b, h, i, (37 * (h * Nq + i) + 11 * b) % D] = 1.0
    q = q.half()
    kp8, vp8, table, kp16, vp16 = _pools(k8, v8, lens, 16, 21, ks, vs)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, False, split)
    assert torch.isfinite(out).all()
    assert torch.equal(out, _run_f16(capi, q, kp16, vp16, table, lens, False, split))
    truth, nks = decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), lens, False)
    check_decode(out.float().cpu().numpy(), truth, nks, "every code in K")


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
def test_every_code_in_v_with_one_key(D, split):
    """kv_len = 1, not causal: the one V row of the batch entries holds the 254 finite codes (each K / V head in another order); the softmax
    weight is exactly 1, so O is dequant(V8 row) x v_scale for every element"""
    capi = _capi()
    B, H, Hkv, Nq = 256 // D, 4, 2, 3
    codes = torch.cat([FINITE_CODES, FINITE_CODES[:2]])
    g = torch.Generator().manual_seed(D)
    k8 = FINITE_CODES[torch.randint(0, 254, (B, Hkv, NCAP, D), generator=g)]
    v8 = FINITE_CODES[torch.randint(0, 254, (B, Hkv, NCAP, D), generator=g)]
    v8[:, 0, 0] = codes.view(B, D)
    v8[:, 1, 0] = codes.flip(0).view(B, D)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    q = torch.randn(B, H, Nq, D, generator=g).half()
    lens = (1,) * B
    kp8, vp8, table, _, _ = _pools(k8, v8, lens, 16, 22, ks, vs)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, False, split).cpu()
    want = dequant(v8[:, :, :1], vs)                                    # [B, Hkv, 1, D]
    G = H // Hkv
    for h in range(H):
        assert torch.equal(out[:, h], want[:, h // G].expand(B, Nq, D)), h
    assert set(v8[:, 0, 0].flatten().tolist()) == set(FINITE_CODES.tolist())


GENERAL_K = (0.037, 0.052, 0.029, 0.044)      # randn / scale has a standard deviation of 19 .. 34: inside +-448, about 2^-4 relative rounding
GENERAL_V = (1.7, 0.9, 2.3, 1.1)              # V8 of a standard deviation around 1


@pytest.mark.parametrize("split", [0, 1, 3, 8])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("shape_nq", [((3, 8, 2), 5), ((2, 4, 4), 16), ((2, 4, 1), 16)], ids=["RT2", "RT1", "RT4"])
@pytest.mark.parametrize("D", [64, 128])
def test_general_scales_against_a_float64_softmax(D, shape_nq, causal, split):
    """scales that are no powers of two: nothing to be bit-equal to, the truth is the definition in float64 on value(code) x float32 scale
    (the dequantised cache has about unit variance).  tol.attn_close unchanged: the kernel's error is the fp16 kernel's — the conversion is
    exact and the scales enter in fp32 (tests/test_abi_cpu_decode_kv8.py compares the two references)"""
    capi = _capi()
    (B, H, Hkv), Nq = shape_nq
    q, k8, v8, ks, vs, lens, truth, nks = _general_case(D, shape_nq, causal)
    kp8, vp8, table = paginate(k8, v8, lens, 64, seed=31, fill=NAN_BYTE)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, f"general scales D={D} S={split}")
    print(f"[decode kv8] general scales D={D} {shape_nq} causal={causal} S={split}: worst |err| / bound {worst:.3f}")


@functools.lru_cache(maxsize=2)
def _general_case(D, shape_nq, causal):
    (B, H, Hkv), Nq = shape_nq
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=7 * D + H + Nq)
    ks, vs = scales(GENERAL_K, Hkv), scales(GENERAL_V, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    lens = _lens_of(B, Hkv)
    k64, v64 = dequant64(k8, ks), dequant64(v8, vs)
    assert 0.9 < float(k64.std()) < 1.1 and 0.9 < float(v64.std()) < 1.1
    truth, nks = softmax64(q, k64, v64, lens, causal)
    return q, k8, v8, ks, vs, lens, truth.astype(np.float32), nks


EDGE_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024)


@functools.lru_cache(maxsize=2)
def _edge_case(D, causal):
    B, H, Hkv, Nq = len(EDGE_LENS), 4, 2, 5
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=177 + D)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    truth, nks = decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), EDGE_LENS, causal)
    return q, k8, v8, ks, vs, truth, nks


@pytest.mark.parametrize("split", [1, 8])
@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_length_edges_in_one_launch(D, causal, ps, split):
    """one batch entry per L, around every page and tile seam: L = 0 uses no table entry at all, L = 1024 every one"""
    capi = _capi()
    q, k8, v8, ks, vs, truth, nks = _edge_case(D, causal)
    kp8, vp8, table, kp16, vp16 = _pools(k8, v8, EDGE_LENS, ps, 5, ks, vs)
    out = _run_kv8(capi, q, kp8, vp8, table, EDGE_LENS, ks, vs, causal, split)
    check_decode(out.float().cpu().numpy(), truth, nks, f"edges D={D} page={ps} S={split}")
    assert torch.equal(out, _run_f16(capi, q, kp16, vp16, table, EDGE_LENS, causal, split))


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("ps", [16, 64])
def test_placement_invariance(ps, split):
    """the same logical cache under two pool permutations and with 3 or 40 spare pages: the same bits"""
    capi = _capi()
    B, H, Hkv, Nq, D = 3, 8, 2, 5, 128
    lens = (1000, 129, 65)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=51)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    outs, tables = [], []
    for seed, spare in ((1, 3), (2, 3), (3, 40)):
        kp8, vp8, table = paginate(k8, v8, lens, ps, seed=seed, spare=spare, fill=NAN_BYTE)
        tables.append(table)
        outs.append(_run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, True, split))
    assert not torch.equal(tables[0], tables[1])
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("D", [64, 128])
def test_tail_and_unused_entries_never_matter(D, ps, causal, split):
    """pool bytes of positions >= L_b and the spare page behind every unused table entry hold zero, then the NaN codes 0x7f and 0xff, then the
    largest finite codes: the same bits"""
    capi = _capi()
    B, H, Hkv, Nq = 3, 8, 2, 5
    lens = (999, 129, 65)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=71 + D)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    kp8, vp8, table = paginate(k8, v8, lens, ps, seed=7, fill=0)
    ref = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split)
    assert torch.isfinite(ref).all()
    for fill in (0x7F, 0xFF, 0x7E, 0xFE):
        kp8, vp8, table2 = paginate(k8, v8, lens, ps, seed=7, fill=fill)
        assert torch.equal(table2, table) and (kp8 == fill).any()
        assert torch.equal(_run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split), ref), fill


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("Nq", [5, 20], ids=["R5", "R20"])
@pytest.mark.parametrize("D", [64, 128])
def test_output_guard(D, Nq, split):
    """O is a view in the middle of a NaN-filled buffer (R = 5 and R = 20: padded row tiles): everything outside stays NaN, O is all finite"""
    capi = _capi()
    B, H, Hkv = 2, 2, 2                       # G = 1: R = Nq
    lens = (129, 1000)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=9 + D + Nq)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(k, ks), quantize(v, vs)
    kp8, vp8, table = paginate(k8, v8, lens, 16, seed=8, fill=NAN_BYTE)
    n = B * H * Nq * D
    guard = 64 * D
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.half, device="cuda")
    o = buf[guard:guard + n].view(B, H, Nq, D)
    _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, True, split, o=o)
    assert torch.isfinite(o).all()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    truth, nks = decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), lens, True)
    check_decode(o.float().cpu().numpy(), truth, nks, "guard")


@functools.lru_cache(maxsize=4)
def _seam_truth(D, causal):
    q, k8, v8, ks, vs, lens = seam_inputs_kv8(D, causal)
    return decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), lens, causal)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_pinned_page_seam_inputs(D, causal, ps, split):
    """one key per row, next to a page seam, outweighs the rest, the cache quantised under scales that differ between heads and between K and
    V: a kernel that ignores or swaps a scale, uses head 0's, decodes e4m3fnuz, swaps the fp16 halves of an fp8 V chunk or takes K bytes in
    the wrong k-step moves the row by >= 20 x the bound (tests/test_abi_cpu_decode_kv8.py); so does a wrong page map (…_decode_paged.py)"""
    capi = _capi()
    q, k8, v8, ks, vs, lens = seam_inputs_kv8(D, causal)
    truth, nks = _seam_truth(D, causal)
    kp8, vp8, table = paginate(k8, v8, lens, ps, seed=17 + D, fill=NAN_BYTE)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, f"pinned seams D={D} page={ps} S={split}")
    print(f"[decode kv8] pinned seams D={D} page={ps} causal={causal} S={split}: worst |err| / bound {worst:.3f}")


@functools.lru_cache(maxsize=4)
def _pinned_case(D, place, causal):
    """tests/decode_lib.py pinned_inputs (Ncap 1000, every L_b below it) in a logical cache of 1024, quantised; the truth is the
    oracle's on the dequantised cache"""
    q, k, v, lens = pinned_inputs(D, place, causal)
    pad = lambda x: torch.cat([x, torch.zeros(*x.shape[:2], NCAP - x.shape[2], x.shape[3], dtype=x.dtype)], dim=2)      # noqa: E731
    Hkv = k.shape[1]
    ks, vs = scales((2.0, 4.0), Hkv), scales(V_SCALES, Hkv)
    k8, v8 = quantize(pad(k), ks), quantize(pad(v), vs)
    assert torch.equal(dequant(k8, ks), pad(k))
    truth, nks = decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), lens, causal)
    return q, k8, v8, ks, vs, lens, truth, nks


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("place", ["last", "first_invisible"])
@pytest.mark.parametrize("D", [64, 128])
def test_pinned_last_visible_and_first_invisible_inputs(D, place, causal, split):
    """the dominant key is the last visible one, or the first invisible one (a large V row there): the mask is still exact to the key"""
    capi = _capi()
    q, k8, v8, ks, vs, lens, truth, nks = _pinned_case(D, place, causal)
    # first_invisible: position L_b keeps ITS row (a mask one key too long has to see the large V row there); the NaN code starts behind it
    kept = tuple(x + 1 for x in lens) if place == "first_invisible" else lens
    kp8, vp8, table = paginate(k8, v8, kept, 16, seed=19 + D, fill=NAN_BYTE)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, f"pinned {place} D={D} S={split}")
    print(f"[decode kv8] pinned {place} D={D} causal={causal} S={split}: worst |err| / bound {worst:.3f}")


def _graph_state(D, ps):
    B, H, Hkv, Nq = 3, 8, 2, 2
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=33 + D)
    lens = (500, 129, 64)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    kp8, vp8, table = paginate(quantize(k, ks), quantize(v, vs), lens, ps, seed=9, spare=40, fill=NAN_BYTE)
    return B, H, Hkv, Nq, q.cuda(), k, v, lens, kp8.cuda(), vp8.cuda(), table.cuda(), _dev_lens(lens), ks.cuda(), vs.cuda()


@pytest.mark.parametrize("split", [4, 0], ids=["S4", "auto"])
def test_graph_capture_with_a_caller_workspace(split):
    """captured once with a caller workspace and replayed: the eager bits.  Then one decode step under NEW scales: a new K / V row per
    sequence, the whole cache requantised, every page moved to another pool slot, block_table, kv_len, k_scale and v_scale rewritten IN PLACE;
    the replay has the bits of an eager call on the new state (only the kernel reads the table, kv_len and the scales)"""
    capi = _capi()
    D, ps = 128, 16
    B, H, Hkv, Nq, q, k, v, lens, kp8, vp8, table, dl, ks, vs = _graph_state(D, ps)
    mp = NCAP // ps
    capi.tune("attn_decode_split", split)
    try:
        name = capi.attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D)
        ws = torch.empty(max(capi.attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D), 16), dtype=torch.uint8, device="cuda")
        if split == 4:
            assert name.endswith(" x4") and ws.numel() == 4 * B * H * Nq * (D + 1) * 4
        eager = torch.full_like(q, float("nan"))
        capi.attn_decode_paged_kv8(q, kp8, vp8, eager, table, dl, ks, vs, causal=True, workspace=ws)
        o = torch.full_like(q, float("nan"))
        st = torch.cuda.Stream()                 # (a non-default stream: capture needs one)
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            capi.attn_decode_paged_kv8(q, kp8, vp8, o, table, dl, ks, vs, causal=True, workspace=ws)      # warm-up on the capture stream
            torch.cuda.synchronize()
            o.fill_(float("nan"))
            with torch.cuda.graph(g, stream=st):
                capi.attn_decode_paged_kv8(q, kp8, vp8, o, table, dl, ks, vs, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.isnan(o).all()               # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager)
        # ---- the next decode step, in place: one more row per sequence, new scales, pages moved, table and kv_len rewritten
        gen = torch.Generator().manual_seed(4)
        for b in range(B):
            k[b, :, lens[b]] = torch.randn(Hkv, D, generator=gen).half()
            v[b, :, lens[b]] = torch.randn(Hkv, D, generator=gen).half()
        new_lens = tuple(x + 1 for x in lens)
        ks2, vs2 = torch.tensor([2.0 ** -2, 2.0 ** -4]), torch.tensor([2.0 ** -3, 2.0 ** -1])
        k8, v8 = quantize(k, ks2), quantize(v, vs2)
        kp2, vp2, table2 = paginate(k8, v8, new_lens, ps, seed=10, spare=40, fill=NAN_BYTE)
        assert not torch.equal(table2.cuda(), table) and not torch.equal(ks2.cuda(), ks) and not torch.equal(vs2.cuda(), vs)
        kp8.copy_(kp2)
        vp8.copy_(vp2)
        table.copy_(table2)
        ks.copy_(ks2)
        vs.copy_(vs2)
        dl += 1
        q.copy_(torch.randn(q.shape, generator=gen).half())
        g.replay()
        torch.cuda.synchronize()
        assert tuple(int(x) for x in dl.cpu()) == (501, 130, 65)
        again = torch.full_like(q, float("nan"))
        capi.attn_decode_paged_kv8(q, kp8, vp8, again, table, dl, ks, vs, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(o, again)
        truth, nks = decode_truth(_oracle(), q.cpu(), dequant(k8, ks2), dequant(v8, vs2), new_lens, True)
        check_decode(o.float().cpu().numpy(), truth, nks, f"replay {name}")
        stale = torch.full_like(q, float("nan"))                      # the old scales on the new bytes are another result: the replay read the new ones
        capi.attn_decode_paged_kv8(q, kp8, vp8, stale, table, dl, scales(K_SCALES, Hkv).cuda(), scales(V_SCALES, Hkv).cuda(), causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert not torch.equal(stale, o)
    finally:
        capi.tune("attn_decode_split", 0)


def test_graph_capture_without_a_workspace_runs_one_range():
    """no caller buffer while the stream is being captured: the S = 1 kernel runs and matches the eager S = 1 call bit for bit"""
    capi = _capi()
    D, ps = 64, 64
    B, H, Hkv, Nq, q, k, v, lens, kp8, vp8, table, dl, ks, vs = _graph_state(D, ps)
    s1 = _run_kv8(capi, q, kp8, vp8, table, dl, ks, vs, False, 1)
    s4 = _run_kv8(capi, q, kp8, vp8, table, dl, ks, vs, False, 4)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    o = torch.full_like(q, float("nan"))
    o2 = torch.full_like(q, float("nan"))
    capi.tune("attn_decode_split", 4)
    try:
        with torch.cuda.stream(st):
            capi.attn_decode_paged_kv8(q, kp8, vp8, o2, table, dl, ks, vs)      # a non-default stream, split through the stream's cached workspace
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                capi.attn_decode_paged_kv8(q, kp8, vp8, o, table, dl, ks, vs)
        g.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    assert torch.equal(o2, s4)
    assert torch.equal(o, s1)


def test_one_model_sized_shape():
    """(4, 32 / 8, Nq 1, Ncap 8192, D 128) in pages of 16 keys — a 2051-page pool, a [4, 512] table — lengths {8192, 8191, 4097, 1}, auto split,
    eight K / V heads each with its own two scales: all 128 rows against the oracle, and the bits of the fp16 paged call"""
    capi = _capi()
    B, H, Hkv, Nq, Ncap, D, ps = 4, 32, 8, 1, 8192, 128, 16
    lens = (8192, 8191, 4097, 1)
    q, k, v = decode_inputs(B, H, Hkv, Nq, Ncap, D, seed=8192)
    ks = torch.tensor([2.0 ** -(1 + h % 4) for h in range(Hkv)])
    vs = torch.tensor([2.0 ** -(4 - h % 4) for h in range(Hkv)])
    k8, v8 = quantize(k, ks), quantize(v, vs)
    name = capi.attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, Ncap // ps, D)
    assert name.startswith("attn_decode_paged_kv8_kernel<128,1> x"), name      # 32 head groups do not fill the GPU: split
    kp8, vp8, table, kp16, vp16 = _pools(k8, v8, lens, ps, 12, ks, vs)
    assert kp8.shape[0] == 2051
    truth, nks = decode_truth(_oracle(), q, dequant(k8, ks), dequant(v8, vs), lens, False)
    out = _run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, False)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, name)
    assert torch.equal(out, _run_f16(capi, q, kp16, vp16, table, lens, False))
    print(f"[decode kv8] {name}: worst |err| / bound {worst:.3f}")
