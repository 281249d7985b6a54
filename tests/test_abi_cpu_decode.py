"""CPU tests of decode attention's boundary (lc_attn_decode_f16, lc_attn_decode_kernel_name, lc_attn_decode_workspace_bytes; no call here
reaches a device): the error codes and their order, the name grid (D x RT x split suffix), the auto split rule under "rule_cus", the
workspace size of the named plan, the audit report of the new kernels — and a test of the GPU tests' inputs: on the pinned inputs of
tests/test_gpu_decode.py a mask one key too long or too short, top-left alignment, an ignored kv_len, the head map `h % Hkv` and "every batch
reads batch 0" each leave the bound by >= 20 x on EVERY row they touch.

The inputs, the visible-key count of a row and the oracle truth of a decode call (Oracle.attn_rows once per distinct count of a batch entry, on
K / V expanded to H heads) are shared with that file: tests/decode_lib.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests.decode_lib import NCAP_RAGGED as NCAP
from tests.decode_lib import (PIN_LENS, PIN_NQ, PIN_SHAPE, PLACES, SCORE, TEETH, _moved, auto_split, decode_inputs, decode_truth, pin_target,
                              pinned_inputs, reset_knobs, rt_of, visible)
from tests.decode_lib import name_flat as _name

# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def knobs(built):
    yield from reset_knobs()


def test_decode_errors_and_their_order(built):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    c, vt = capi.ATTN_CAUSAL, capi.ATTN_V_TRANSPOSED
    p = C.c_void_p(16)
    f = lib.lc_attn_decode_f16
    ok = (1, 8, 2, 4, 1000, 128)              # B, H, Hkv, Nq, Ncap, D
    for flags in (0, c):
        for nul in range(4):
            ptrs = [p, p, p, p]
            ptrs[nul] = None
            assert f(*ptrs, None, *ok, flags, None, 0, None) == capi.LC_ERR_ARG, nul
            assert f(*ptrs, None, 1, 8, 3, 4, 1000, 256, flags, None, 0, None) == capi.LC_ERR_ARG      # null pointer before shape and head dim
        for hkv in (0, -1, 3, 5, 9, 16):
            assert f(p, p, p, p, None, 1, 8, hkv, 4, 1000, 128, flags, None, 0, None) == capi.LC_ERR_SHAPE, hkv
        for B, H, Hkv, Nq, Ncap, D in ((0, 8, 2, 4, 1000, 128), (1, 0, 0, 4, 1000, 128), (1, 8, 2, 0, 1000, 128), (1, 8, 2, 4, 0, 128),
                                       (1, 8, 2, 4, -5, 128), (1, 8, 2, 4, 1000, 0), (1, 8, 2, 17, 1000, 128), (1, 8, 8, 65, 1000, 64),
                                       (1, 64, 1, 2, 1000, 64), (1, 8, 2, 4, 1 << 23, 128), (1, 8, 2, 4, 1 << 24, 64)):
            assert f(p, p, p, p, None, B, H, Hkv, Nq, Ncap, D, flags, None, 0, None) == capi.LC_ERR_SHAPE, (B, H, Hkv, Nq, Ncap, D)
        assert f(p, p, p, p, None, 1, 8, 3, 4, 1000, 256, flags, None, 0, None) == capi.LC_ERR_SHAPE       # shape before head dim
        assert f(p, p, p, p, None, 1, 8, 2, 17, 1000, 96, flags, None, 0, None) == capi.LC_ERR_SHAPE       # R > 64 before head dim
        assert f(C.c_void_p(8), p, p, p, None, *ok, flags, None, 0, None) == capi.LC_ERR_SHAPE             # alignment, as lc_attn_fwd_f16
        for d in (32, 96, 256, 512, 1024, 16, 48):
            assert f(p, p, p, p, None, 1, 8, 2, 4, 1000, d, flags, None, 0, None) == capi.LC_ERR_HEADDIM, d
            assert _name(1, 8, 2, 4, 1000, d, flags)[0] == capi.LC_ERR_HEADDIM
    for bad in (vt, c | vt, 4, -1, 1 << 30):
        assert f(p, p, p, p, None, *ok, bad, None, 0, None) == capi.LC_ERR_ARG, bad                        # a [D,N] cache is not a thing
        assert f(p, p, p, p, None, 1, 8, 3, 4, 1000, 256, bad, None, 0, None) == capi.LC_ERR_ARG           # flags before everything
        assert _name(*ok, bad)[0] == capi.LC_ERR_ARG
        assert _name(1, 8, 3, 4, 1000, 256, bad)[0] == capi.LC_ERR_ARG
    assert _name(1, 8, 3, 4, 1000, 256)[0] == capi.LC_ERR_SHAPE
    assert _name(1, 8, 2, 17, 1000, 128)[0] == capi.LC_ERR_SHAPE
    assert lib.lc_attn_decode_kernel_name(*ok, 0, None, 128) == capi.LC_ERR_ARG
    assert lib.lc_attn_decode_kernel_name(*ok, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
    assert lib.lc_attn_decode_workspace_bytes(1, 8, 3, 4, 1000, 128) == 0                                  # a shape the call refuses
    assert lib.lc_attn_decode_workspace_bytes(1, 8, 2, 4, 1000, 96) == 0


def test_a_small_or_misaligned_workspace_is_refused_before_any_device_work(knobs):
    lib = capi.load()
    p = C.c_void_p(16)
    capi.tune("attn_decode_split", 4)
    need = lib.lc_attn_decode_workspace_bytes(1, 8, 2, 4, 1000, 128)
    assert need == 4 * (1 * 8 * 4) * 129 * 4
    f = lib.lc_attn_decode_f16
    for nbytes in (0, 16, need - 1):
        assert f(p, p, p, p, None, 1, 8, 2, 4, 1000, 128, 0, C.c_void_p(256), nbytes, None) == capi.LC_ERR_ARG, nbytes
        assert f(p, p, p, p, p, 1, 8, 2, 4, 1000, 128, 1, C.c_void_p(256), nbytes, None) == capi.LC_ERR_ARG
    assert f(p, p, p, p, None, 1, 8, 2, 4, 1000, 128, 0, C.c_void_p(8), need, None) == capi.LC_ERR_ARG
    assert f(p, p, p, p, None, 1, 8, 2, 4, 1000, 96, 0, C.c_void_p(256), 0, None) == capi.LC_ERR_HEADDIM    # head dim before the workspace
    assert f(p, p, p, p, None, 1, 8, 3, 4, 1000, 128, 0, C.c_void_p(256), 0, None) == capi.LC_ERR_SHAPE


def test_name_grid_head_dim_row_tiles_and_split_suffix(knobs):
    for D in (64, 128):
        for (B, H, Hkv), Nq, rt in (((3, 8, 2), 1, 1), ((3, 8, 2), 4, 1), ((3, 8, 2), 5, 2), ((3, 8, 2), 8, 2), ((3, 8, 2), 9, 4),
                                    ((3, 8, 2), 16, 4), ((2, 4, 1), 1, 1), ((2, 4, 1), 4, 1), ((2, 4, 1), 5, 2), ((2, 4, 1), 16, 4),
                                    ((2, 4, 4), 1, 1), ((2, 4, 4), 16, 1), ((2, 4, 4), 17, 2), ((2, 4, 4), 33, 4), ((2, 4, 4), 64, 4),
                                    ((1, 64, 1), 1, 4)):
            assert rt == rt_of(H, Hkv, Nq)
            for flags in (0, capi.ATTN_CAUSAL):
                for s in (1, 2, 3, 8, 64):
                    capi.tune("attn_decode_split", s)
                    want = f"attn_decode_kernel<{D},{rt}>" + (f" x{s}" if s > 1 else "")
                    assert _name(B, H, Hkv, Nq, NCAP, D, flags) == (capi.LC_OK, want)
                    assert capi.attn_decode_workspace_bytes(B, H, Hkv, Nq, NCAP, D) == (s * B * H * Nq * (D + 1) * 4 if s > 1 else 0)
    capi.tune("attn_decode_split", 0)
    assert capi.load().lc_tune_set(b"attn_decode_split", 65) == capi.LC_ERR_ARG
    assert capi.load().lc_tune_set(b"attn_decode_split", -1) == capi.LC_ERR_ARG
    assert capi.tune_get("attn_decode_split") == (0, 0)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_auto_split_rule(knobs, cus):
    """S from (B x Hkv, ceil(Ncap / 64), the CU count) alone; the workspace size is that of the named S"""
    capi.tune("rule_cus", cus)
    for B, H, Hkv, Nq, Ncap, D in ((1, 32, 8, 1, 8192, 128), (16, 32, 8, 1, 4096, 128), (64, 32, 8, 1, 2048, 128), (4, 64, 8, 1, 32768, 128),
                                   (8, 32, 8, 4, 4096, 128), (8, 32, 32, 1, 4096, 64), (1, 8, 1, 1, 1 << 20, 64), (1, 8, 8, 1, 255, 64),
                                   (1, 8, 8, 1, 256, 64), (1, 8, 2, 1, 1000, 128), (3, 8, 2, 5, 1000, 128), (1, 1, 1, 1, 1, 64),
                                   (1, 1, 1, 1, 511, 128), (1, 1, 1, 1, 512, 128), (300, 8, 1, 1, 4096, 64)):
        s = auto_split(B * Hkv, Ncap, cus)
        rc, name = _name(B, H, Hkv, Nq, Ncap, D)
        assert rc == capi.LC_OK
        assert name == f"attn_decode_kernel<{D},{rt_of(H, Hkv, Nq)}>" + (f" x{s}" if s > 1 else ""), (B, Hkv, Ncap, cus, s, name)
        assert capi.attn_decode_workspace_bytes(B, H, Hkv, Nq, Ncap, D) == (s * B * H * Nq * (D + 1) * 4 if s > 1 else 0)
    spot = {64: (8, 1, 1, 2, 1, 1), 256: (32, 2, 1, 8, 4, 1), 304: (32, 3, 1, 10, 5, 2)}[cus]
    assert tuple(auto_split(g, n, cus) for g, n in ((8, 8192), (128, 4096), (512, 2048), (32, 32768), (64, 4096), (256, 4096))) == spot


def test_capi_wrapper_checks_shapes_without_a_gpu(built):
    q, k, v = decode_inputs(2, 8, 2, 4, 100, 64, seed=1)
    o = torch.empty_like(q)
    assert capi._attn_dims_decode(q, k, v, o) == (2, 8, 2, 4, 100, 64)
    assert capi._attn_dims_decode(q, k, v, o, torch.zeros(2, dtype=torch.int32)) == (2, 8, 2, 4, 100, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_decode(q, k, v, o)
    for bad_k in (torch.empty(2, 3, 100, 64), torch.empty(1, 2, 100, 64), torch.empty(2, 2, 100, 32), torch.empty(2, 16, 100, 64)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._attn_dims_decode(q, bad_k.half(), bad_k.half(), o)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_decode(q, k, v[:, :, :99].contiguous(), o)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_decode(q, k, v, o[:, :, :3].contiguous())
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_decode(q, k, v, o, torch.zeros(3, dtype=torch.int32))


def test_audit_knows_the_decode_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import isa_audit
    rep = json.loads((built["abi"].parent / "obj" / "isa_audit.json").read_text())
    dec = [r for r in rep if "attn_decode" in r["kernel"]]
    names = " ".join(r["kernel"] for r in dec)
    for d in (64, 128):
        for rt in (1, 2, 4):
            assert f"attn_decode_kernelILi{d}ELi{rt}E" in names, (d, rt)
        assert f"attn_decode_combine_kernelILi{d}E" in names, d
    assert len(dec) == 8
    for r in dec:
        assert r["scratch"] == 0 and not r["violations"], r
        assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]          # plain HIP: listed for rule R2 only, owns no AGPR
        assert r["asm_loads"] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# a test of the GPU tests' inputs

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_a_wrong_mask_or_map_moves_every_row_it_touches(oracle, D, causal):
    B, H, Hkv = PIN_SHAPE
    Nq, G = PIN_NQ, H // Hkv
    lens = PIN_LENS
    right = lambda b, i: visible(lens[b], Nq, NCAP, causal, i)      # noqa: E731
    # variant -> (the placement that pins it, the wrong kernel as decode_truth keywords, the rows [B, H, Nq] it touches)
    every = np.ones((B, H, Nq), bool)
    br_ne_tl = np.array([[[right(b, i) != min(i + 1, lens[b]) for i in range(Nq)] for _ in range(H)] for b in range(B)])
    head_moves = np.array([[[h % Hkv != h // G] * Nq for h in range(H)] for _ in range(B)])
    batch_moves = np.array([[[b != 0] * Nq for _ in range(H)] for b in range(B)])
    variants = {
        "mask one key too long": ("first_invisible", dict(nk_of=lambda b, i: right(b, i) + 1), every),
        "mask one key too short": ("last", dict(nk_of=lambda b, i: right(b, i) - 1), every),
        "kv_len ignored": ("first_invisible", dict(nk_of=lambda b, i: visible(NCAP, Nq, NCAP, causal, i)), every),
        "head map h % Hkv": ("last", dict(kv_head=lambda h: h % Hkv), head_moves),
        "every batch reads batch 0": ("key0", dict(kv_batch=lambda b: 0), batch_moves),
    }
    if causal:
        variants["top-left alignment"] = ("last", dict(nk_of=lambda b, i: min(i + 1, lens[b])), br_ne_tl)
    for name, (place, kw, touched) in variants.items():
        q, k, v, _ = pinned_inputs(D, place, causal)
        truth, nks = decode_truth(oracle, q, k, v, lens, causal)
        assert (nks >= 1).all() and (nks < NCAP).all()              # every row of the pinned shapes has a visible and an invisible key
        wrong, _ = decode_truth(oracle, q, k, v, lens, causal, **kw)
        ratio = _moved(truth, nks, wrong)
        assert touched.any(), name
        assert ratio[touched].min() >= TEETH, (name, D, causal, float(ratio[touched].min()))
        assert ratio[~touched].max(initial=0.0) == 0.0, name


def test_the_pinned_inputs_are_what_the_docstring_says():
    for causal in (False, True):
        for place in PLACES:
            q, k, v, lens = pinned_inputs(64, place, causal)
            B, H, Hkv = PIN_SHAPE
            G = H // Hkv
            assert (k.abs() == 1).all() and torch.isfinite(v).all()
            hits = 0
            for b in range(B):
                for h in range(H):
                    for i in range(PIN_NQ):
                        t = pin_target(place, lens[b], PIN_NQ, NCAP, causal, (h % G) * PIN_NQ + i, 3)
                        if t is None:
                            continue
                        hits += 1
                        s = (q[b, h, i].double() @ k[b, h // G].double().T) / 8.0
                        assert abs(s[t].item() - SCORE) <= SCORE * 2.0 ** -11 and s.argmax().item() == t
                        lim = visible(lens[b], PIN_NQ, NCAP, causal, i)
                        assert (t == lim) if place == "first_invisible" else (t < lim)
                        if place == "first_invisible":
                            assert v[b, h // G, t].abs().min().item() == 8.0
            assert hits >= B * H * PIN_NQ - (H * PIN_NQ if place.endswith("_seam") else 0), (place, hits)      # (L = 65: one seam, few rows past it)
    # both sides of a seam occur
    for place, split in (("tile_seam", 3), ("range_seam", 3), ("range_seam", 8)):
        ts = {pin_target(place, 777, PIN_NQ, NCAP, False, r, split) % 64 for r in range(20)}
        assert ts == {63, 0}, (place, split, ts)
