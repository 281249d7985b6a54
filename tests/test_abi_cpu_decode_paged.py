"""CPU tests of paged decode attention's boundary (lc_attn_decode_paged_f16, lc_attn_decode_paged_kernel_name,
lc_attn_decode_paged_workspace_bytes; no call here reaches a device): the error codes and their order, the name grid, the split rule and the
workspace bytes against the contiguous call of Ncap = max_pages x page_size, the Python shape checks, the audit report of the six new kernels —
and a test of the GPU tests' pinned page-seam inputs: on them a kernel that ignores the table, is off by one page, reads table row 0 for every
batch entry, ignores the K / V head in the page base or takes the in-page offset modulo 16 leaves the bound by >= 20 x on EVERY row it touches.

`paginate` (a contiguous cache scattered over a pool, NaN wherever the kernel must not read), its inverse `gather`, the inputs, truth and row
check are shared with tests/test_gpu_decode_paged.py: tests/decode_lib.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests.decode_lib import NCAP_POW2 as NCAP
from tests.decode_lib import (PIN_NQ, PIN_SHAPE, SCORE, TEETH, _wrong_kernel, auto_split, decode_inputs, decode_truth, gather, paginate,
                              reset_knobs, rt_of, seam_inputs, seam_target, visible)
from tests.decode_lib import name_paged as _name

# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def knobs(built):
    yield from reset_knobs()


def test_paged_errors_and_their_order(built):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    c, vt = capi.ATTN_CAUSAL, capi.ATTN_V_TRANSPOSED
    p = C.c_void_p(16)
    f = lib.lc_attn_decode_paged_f16
    ok = (1, 8, 2, 4, 70, 16, 64, 128)        # B, H, Hkv, Nq, num_pages, page_size, max_pages, D
    bad_shape = (1, 8, 3, 4, 70, 16, 64, 256)
    for flags in (0, c):
        for nul in range(6):                  # Q, Kpool, Vpool, O, block_table, kv_len
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
                      (1, 8, 2, 4, 70, 16, 1 << 19, 128), (1, 8, 2, 4, 70, 1 << 20, 16, 64), (1, 8, 2, 4, 70, 1 << 16, 1 << 16, 64),
                      (1 << 24, 8, 8, 1, 70, 16, 64, 64)):
            assert f(*[p] * 6, *shape, flags, None, 0, None) == capi.LC_ERR_SHAPE, shape
            assert _name(*shape[:4], *shape[5:], flags)[0] == capi.LC_ERR_SHAPE or shape[4] <= 0, shape      # (the name call takes no num_pages)
            assert lib.lc_attn_decode_paged_workspace_bytes(*shape[:4], *shape[5:]) == 0 or shape[4] <= 0
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
            assert lib.lc_attn_decode_paged_workspace_bytes(1, 8, 2, 4, 16, 64, d) == 0
    for bad in (vt, c | vt, 4, -1, 1 << 30):
        assert f(*[p] * 6, *ok, bad, None, 0, None) == capi.LC_ERR_ARG, bad
        assert f(*[p] * 6, *bad_shape, bad, None, 0, None) == capi.LC_ERR_ARG                               # flags before everything
        assert f(None, p, p, p, p, p, *ok, bad, None, 0, None) == capi.LC_ERR_ARG
        assert _name(1, 8, 2, 4, 16, 64, 128, bad)[0] == capi.LC_ERR_ARG
        assert _name(1, 8, 3, 4, 24, 64, 256, bad)[0] == capi.LC_ERR_ARG
    assert _name(1, 8, 3, 4, 16, 64, 256)[0] == capi.LC_ERR_SHAPE
    assert _name(1, 8, 2, 4, 8, 64, 128)[0] == capi.LC_ERR_SHAPE
    assert lib.lc_attn_decode_paged_kernel_name(1, 8, 2, 4, 16, 64, 128, 0, None, 128) == capi.LC_ERR_ARG
    assert lib.lc_attn_decode_paged_kernel_name(1, 8, 2, 4, 16, 64, 128, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
    rc, name = _name(1, 8, 2, 4, 16, 64, 128)
    assert rc == capi.LC_OK and name.startswith("attn_decode_paged_kernel<128,1>")


def test_a_small_or_misaligned_workspace_is_refused_before_any_device_work(knobs):
    lib = capi.load()
    p = C.c_void_p(16)
    capi.tune("attn_decode_split", 4)
    need = lib.lc_attn_decode_paged_workspace_bytes(1, 8, 2, 4, 16, 64, 128)
    assert need == 4 * (1 * 8 * 4) * 129 * 4
    f = lib.lc_attn_decode_paged_f16
    for nbytes in (0, 16, need - 1):
        assert f(*[p] * 6, 1, 8, 2, 4, 70, 16, 64, 128, 0, C.c_void_p(256), nbytes, None) == capi.LC_ERR_ARG, nbytes
    assert f(*[p] * 6, 1, 8, 2, 4, 70, 16, 64, 128, 0, C.c_void_p(8), need, None) == capi.LC_ERR_ARG
    assert f(*[p] * 6, 1, 8, 2, 4, 70, 16, 64, 96, 0, C.c_void_p(256), 0, None) == capi.LC_ERR_HEADDIM    # head dim before the workspace
    assert f(*[p] * 6, 1, 8, 2, 4, 70, 24, 64, 128, 0, C.c_void_p(256), 0, None) == capi.LC_ERR_SHAPE


def test_name_grid_head_dim_row_tiles_and_split_suffix(knobs):
    for D in (64, 128):
        for (B, H, Hkv), Nq in (((3, 8, 2), 1), ((3, 8, 2), 4), ((3, 8, 2), 5), ((3, 8, 2), 8), ((3, 8, 2), 9), ((3, 8, 2), 16), ((2, 4, 1), 1),
                                ((2, 4, 1), 5), ((2, 4, 1), 16), ((2, 4, 4), 16), ((2, 4, 4), 17), ((2, 4, 4), 33), ((2, 4, 4), 64), ((1, 64, 1), 1)):
            rt = rt_of(H, Hkv, Nq)
            for flags in (0, capi.ATTN_CAUSAL):
                for ps, mp in ((16, 64), (256, 4), (1024, 1)):
                    for s in (1, 2, 3, 8, 64):
                        capi.tune("attn_decode_split", s)
                        want = f"attn_decode_paged_kernel<{D},{rt}>" + (f" x{s}" if s > 1 else "")
                        assert _name(B, H, Hkv, Nq, ps, mp, D, flags) == (capi.LC_OK, want)
                        assert capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=bool(flags)) == want
                        assert capi.attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == (s * B * H * Nq * (D + 1) * 4 if s > 1 else 0)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_auto_split_and_workspace_are_those_of_the_contiguous_call(knobs, cus):
    """S from (B x Hkv, max_pages x page_size, the CU count) alone: the suffix and the bytes of lc_attn_decode_* at that Ncap"""
    capi.tune("rule_cus", cus)
    for B, H, Hkv, Nq, ps, mp, D in ((1, 32, 8, 1, 16, 512, 128), (1, 32, 8, 1, 8192, 1, 128), (16, 32, 8, 1, 64, 64, 128), (64, 32, 8, 1, 256, 8, 128),
                                     (4, 64, 8, 1, 16, 2048, 128), (8, 32, 8, 4, 128, 32, 128), (8, 32, 32, 1, 16, 256, 64), (1, 8, 1, 1, 1024, 1024, 64),
                                     (1, 8, 8, 1, 16, 15, 64), (1, 8, 8, 1, 16, 16, 64), (1, 8, 2, 1, 16, 64, 128), (3, 8, 2, 5, 64, 16, 128),
                                     (1, 1, 1, 1, 16, 1, 64), (1, 1, 1, 1, 16, 31, 128), (1, 1, 1, 1, 16, 32, 128), (300, 8, 1, 1, 32, 128, 64)):
        ncap = ps * mp
        s = auto_split(B * Hkv, ncap, cus)
        rc, name = _name(B, H, Hkv, Nq, ps, mp, D)
        assert rc == capi.LC_OK
        assert name == f"attn_decode_paged_kernel<{D},{rt_of(H, Hkv, Nq)}>" + (f" x{s}" if s > 1 else ""), (B, Hkv, ps, mp, cus, s, name)
        flat = capi.attn_decode_kernel_name(B, H, Hkv, Nq, ncap, D)
        assert name.replace("_paged", "") == flat
        assert capi.attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == capi.attn_decode_workspace_bytes(B, H, Hkv, Nq, ncap, D)
        assert capi.attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == (s * B * H * Nq * (D + 1) * 4 if s > 1 else 0)


def test_capi_wrapper_checks_shapes_without_a_gpu(built):
    q, k, v = decode_inputs(2, 8, 2, 4, 128, 64, seed=1)
    o = torch.empty_like(q)
    lens = torch.tensor([100, 17], dtype=torch.int32)
    kp, vp, table = paginate(k, v, (100, 17), 16, seed=2)
    assert tuple(kp.shape) == (2 * 8 + 3, 2, 16, 64) and tuple(table.shape) == (2, 8)
    assert capi._attn_dims_decode_paged(q, kp, vp, o, table, lens) == (2, 8, 2, 4, 19, 16, 8, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_decode_paged(q, kp, vp, o, table, lens)
    for bad in (torch.empty(19, 3, 16, 64), torch.empty(19, 2, 16, 32), torch.empty(19, 16, 16, 64)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._attn_dims_decode_paged(q, bad.half(), bad.half(), o, table, lens)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_decode_paged(q, kp, vp[:18].contiguous(), o, table, lens)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_decode_paged(q, kp, vp[:, :, :8].contiguous(), o, table, lens)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_decode_paged(q, kp, vp, o[:, :, :3].contiguous(), table, lens)
    for bad_table in (None, table[:1], table.view(-1), torch.zeros(3, 8, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._attn_dims_decode_paged(q, kp, vp, o, bad_table, lens)
    for bad_lens in (None, torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._attn_dims_decode_paged(q, kp, vp, o, table, bad_lens)


def test_audit_knows_the_paged_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    rep = json.loads((built["abi"].parent / "obj" / build.AUDIT_OWN_REPORT["tu_attn_decode_paged"]).read_text())
    dec = [r for r in rep if "attn_decode_paged_kernel" in r["kernel"]]
    names = " ".join(r["kernel"] for r in dec)
    for d in (64, 128):
        for rt in (1, 2, 4):
            assert f"attn_decode_paged_kernelILi{d}ELi{rt}E" in names, (d, rt)
    assert len(dec) == 6 and len(rep) == 6
    for r in dec:
        assert r["scratch"] == 0 and not r["violations"], r
        assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]          # plain HIP: listed for rule R2 only
        assert r["asm_loads"] == 0


def test_paginate_and_gather_are_inverse_and_poison_what_must_not_be_read():
    B, Hkv, D, ps = 3, 2, 64, 16
    _, k, v = decode_inputs(B, 4, Hkv, 1, NCAP, D, seed=3)
    lens = (777, 129, 0)
    kp, vp, table = paginate(k, v, lens, ps, seed=11)
    mp = NCAP // ps
    assert kp.shape[0] == B * mp + 3 and table.min() >= 0 and table.max() < kp.shape[0]
    for pool, x in ((kp, k), (vp, v)):
        back = gather(pool, table)
        for b, L in enumerate(lens):
            assert torch.equal(back[b, :, :L], x[b, :, :L]) and torch.isnan(back[b, :, L:]).all()
    used = [-(-L // ps) for L in lens]
    spares = {int(x) for b in range(B) for x in table[b, used[b]:]}
    assert len(spares) <= 3 and all(torch.isnan(kp[s]).all() and torch.isnan(vp[s]).all() for s in spares)
    live = table[0, :used[0]].tolist()
    assert live != sorted(live) and len(set(live)) == len(live)                   # scattered, non-monotone
    lo, hi = min(live), max(live)
    assert any(lo < int(x) < hi for x in table[1, :used[1]])                      # interleaved with another entry's pages
    assert not torch.equal(paginate(k, v, lens, ps, seed=12)[2], table)
    z = paginate(k, v, lens, ps, seed=11, fill=0.0)
    assert torch.equal(z[2], table) and torch.isfinite(z[0]).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# a test of the GPU tests' inputs

@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_a_wrong_page_map_moves_every_row_it_touches(oracle, D, causal):
    B, H, Hkv = PIN_SHAPE
    Nq, G = PIN_NQ, H // Hkv
    q, k, v, lens = seam_inputs(D, causal)
    truth, nks = decode_truth(oracle, q, k, v, lens, causal)
    assert (nks >= 33).all() and (nks < NCAP).all()
    has_target = np.array([[[seam_target(lens[b], Nq, NCAP, causal, (h % G) * Nq + i) is not None for i in range(Nq)] for h in range(H)]
                           for b in range(B)])
    assert has_target.all()                                             # every row of the pinned shapes has a seam below its limit
    pages = {seam_target(lens[0], Nq, NCAP, causal, r) // 16 for r in range(G * Nq)}
    assert len(pages) >= 8                                              # the rows of one K / V head cover many pages
    assert {seam_target(lens[0], Nq, NCAP, causal, r) % 16 for r in range(G * Nq)} == {15, 0}
    every = np.ones((B, H, Nq), bool)
    batch_moves = np.array([[[b != 0] * Nq for _ in range(H)] for b in range(B)])
    head_moves = np.array([[[h // G != 0] * Nq for h in range(H)] for _ in range(B)])
    mp16 = NCAP // 16
    variants = {       # name -> (page size, the wrong kernel as gather keywords, the rows it touches)
        "the table ignored (identity pages)": (16, dict(page_of=lambda b, p: p), every),
        "page index off by one": (16, dict(page_of=None), every),       # (filled in below: needs the table)
        "every batch entry uses table row 0": (16, dict(batch_of=lambda b: 0), batch_moves),
        "the page base ignores the K / V head": (16, dict(head_of=lambda h: 0), head_moves),
        "the in-page offset modulo 16 at page_size 64": (64, dict(row_of=lambda j: j % 16), every),
    }
    pools = {ps: paginate(k, v, lens, ps, seed=17 + D) for ps in (16, 64)}
    for ps, (kp, vp, table) in pools.items():       # the right map gives the truth back exactly (the NaN tail is never visible)
        assert (_wrong_kernel(oracle, q, gather(kp, table), gather(vp, table), lens, causal, truth, nks) == 0).all(), ps
    for name, (ps, kw, touched) in variants.items():
        kp, vp, table = pools[ps]
        if name == "page index off by one":
            kw = dict(page_of=lambda b, p, t=table: int(t[b, min(p + 1, mp16 - 1)]))
        ratio = _wrong_kernel(oracle, q, gather(kp, table, **kw), gather(vp, table, **kw), lens, causal, truth, nks)
        assert touched.any(), name
        assert ratio[touched].min() >= TEETH, (name, D, causal, float(ratio[touched].min()))
        assert ratio[~touched].max(initial=0.0) == 0.0, name


def test_the_seam_inputs_are_what_the_docstring_says():
    for causal in (False, True):
        q, k, v, lens = seam_inputs(64, causal)
        B, H, Hkv = PIN_SHAPE
        G = H // Hkv
        assert (k.abs() == 1).all() and torch.isfinite(v).all()
        for b in range(B):
            for h in range(H):
                for i in range(PIN_NQ):
                    t = seam_target(lens[b], PIN_NQ, NCAP, causal, (h % G) * PIN_NQ + i)
                    s = (q[b, h, i].double() @ k[b, h // G].double().T) / 8.0
                    assert abs(s[t].item() - SCORE) <= SCORE * 2.0 ** -11 and s.argmax().item() == t
                    assert t < visible(lens[b], PIN_NQ, NCAP, causal, i) and t % 16 in (15, 0)       # next to a 16-key page seam, visible
                    assert t % 64 >= 16                                                              # lost by "offset modulo 16" in a 64-key page
