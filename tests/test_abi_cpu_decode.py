"""CPU tests of decode attention's boundary (lc_attn_decode_f16, lc_attn_decode_kernel_name, lc_attn_decode_workspace_bytes; no call here
reaches a device): the error codes and their order, the name grid (D x RT x split suffix), the auto split rule under "rule_cus", the
workspace size of the named plan, the audit report of the new kernels — and a test of the GPU tests' inputs: on the pinned inputs of
tests/test_gpu_decode.py a mask one key too long or too short, top-left alignment, an ignored kv_len, the head map `h % Hkv` and "every batch
reads batch 0" each leave the bound by >= 20 x on EVERY row they touch.

This module also holds what both files share: the inputs, the visible-key count of a row and the oracle truth of a decode call
(Oracle.attn_rows once per distinct count of a batch entry, on K / V expanded to H heads)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import tol

NCAP = 1000
GRID_SHAPES = [(3, 8, 2), (2, 4, 1), (2, 4, 4)]                     # (B, H, Hkv)
GRID_LENS = {3: (NCAP, 129, 65), 2: (65, NCAP)}                      # per-batch kv_len of the grid test, by B (B = 2 with Hkv = 4: reversed)
GRID_NQ = (1, 4, 5, 16)
SCORE = 12.0      # natural units: the dominant key of a pinned row (the construction of tests/test_gpu_causal_mask.py)
TEETH = 20.0
PIN_SHAPE = (3, 8, 2)
PIN_NQ = 5
PIN_LENS = (777, 129, 65)       # all < NCAP: position L_b exists, so "the first invisible key" does for every row
PLACES = ("last", "first_invisible", "key0", "tile_seam", "range_seam")


def decode_inputs(B, H, Hkv, Nq, Ncap, D, seed):
    """fp16 randn q [B,H,Nq,D], k, v [B,Hkv,Ncap,D] on the CPU (the GPU tests move them over: both files test the same inputs)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, Nq, D, generator=g).half(), torch.randn(B, Hkv, Ncap, D, generator=g).half(),
            torch.randn(B, Hkv, Ncap, D, generator=g).half())


def visible(L, Nq, Ncap, causal, i):
    """number of keys query i of a batch entry with kv_len L sees: keys 0 .. visible - 1 (lc_abi.h: bottom-right aligned)"""
    L = min(max(int(L), 0), Ncap)
    return max(0, L - Nq + i + 1) if causal else L


def rt_of(H, Hkv, Nq):
    R = (H // Hkv) * Nq
    return 1 if R <= 16 else 2 if R <= 32 else 4


def decode_truth(oracle, q, k, v, lens, causal, nk_of=None, kv_head=None, kv_batch=None):
    """(truth fp32 [B,H,Nq,D], nk int [B,Nq]): the oracle on every row.  lens: per-batch kv_len (None: Ncap).  The keyword arguments restate a
    WRONG kernel for the tests of the inputs: nk_of(b, i) -> visible keys, kv_head(h) -> K / V head, kv_batch(b) -> batch entry read."""
    B, H, Nq, D = q.shape
    Hkv, Ncap = k.shape[1], k.shape[2]
    G = H // Hkv
    heads = [kv_head(h) if kv_head else h // G for h in range(H)]
    truth = np.zeros((B, H, Nq, D), np.float32)
    nks = np.zeros((B, Nq), np.int64)
    for b in range(B):
        L = Ncap if lens is None else lens[b]
        for i in range(Nq):
            nks[b, i] = nk_of(b, i) if nk_of else visible(L, Nq, Ncap, causal, i)
        bb = kv_batch(b) if kv_batch else b
        kb, vb = k[bb][heads], v[bb][heads]                     # [H, Ncap, D]: expanded to the query heads
        for nk in sorted(set(int(x) for x in nks[b])):
            rows = [i for i in range(Nq) if nks[b, i] == nk]
            if nk == 0:
                continue                                        # no visible key: exactly 0
            o = oracle.attn_rows(q[b][:, rows].contiguous(), kb[:, :nk].contiguous(), vb[:, :nk].contiguous(), H, len(rows), nk, D)
            truth[b][:, rows] = o
    return truth, nks


def check_decode(out, truth, nks, what=""):
    """every row under tol.attn_close with N = the row's visible keys; rows without a visible key are exactly 0.  Returns the worst
    |err| / bound (for the docstrings)."""
    out = np.asarray(out, np.float32)
    worst = 0.0
    B, H, Nq, D = truth.shape
    for b in range(B):
        for i in range(Nq):
            nk = int(nks[b, i])
            o, t = out[b, :, i], truth[b, :, i]
            if nk == 0:
                assert (o == 0).all(), (what, "row without a visible key is not 0", b, i, float(np.abs(o).max()))
                continue
            assert np.isfinite(o).all(), (what, "non-finite", b, i)
            ok, err, excess = tol.attn_close(o, t, N=nk)
            bound = tol.attn_max_abs(nk) + tol.ATTN_RTOL_F16 * np.abs(t.astype(np.float64))
            worst = max(worst, float((np.abs(o.astype(np.float64) - t) / bound).max()))
            assert ok, (what, f"batch {b} query {i} nk {nk}: max |err| {err:.3e}, excess over the bound {excess:.3e}")
    return worst


def pin_target(place, L, Nq, Ncap, causal, r, split):
    """the key that scores SCORE for row r = g Nq + i of a K / V head (None: the row keeps a random query)"""
    i = r % Nq
    lim = visible(L, Nq, Ncap, causal, i)
    if place == "last":
        return lim - 1 if lim >= 1 else None
    if place == "first_invisible":
        return lim if lim < Ncap else None
    if place == "key0":
        return 0 if lim >= 1 else None
    if place == "tile_seam":                        # either side of the last tile seam below the row's limit
        p = 64 * ((lim - 1) // 64) if lim >= 1 else 0
        if p == 0:
            return None
        return p - 1 if r % 2 == 0 else p
    if place == "range_seam":                       # either side of a seam between two KV ranges of the kernel's partition (split ranges)
        T = (L + 63) // 64
        seams = sorted({64 * (s * T // split) for s in range(1, split)} - {0})
        seams = [p for p in seams if p < lim]
        if not seams:
            return None
        p = seams[(r // 2) % len(seams)]
        return p - 1 if r % 2 == 0 else p
    raise KeyError(place)


@functools.lru_cache(maxsize=16)
def pinned_inputs(D, place, causal, split=3):
    """(q, k, v, lens): per row ONE key outweighs the rest — K random +-1, Q_row = (SCORE / sqrt(D)) K[target], V randn; the target of
    `first_invisible` carries a large distinctive V row (+-8).  Rows without a target (no visible key, no seam below the limit) keep randn."""
    B, H, Hkv = PIN_SHAPE
    Nq, G = PIN_NQ, PIN_SHAPE[1] // PIN_SHAPE[2]
    g = torch.Generator().manual_seed(7919 * D + 31 * PLACES.index(place) + int(causal))
    k = (torch.randint(0, 2, (B, Hkv, NCAP, D), generator=g) * 2 - 1).float()
    v = torch.randn(B, Hkv, NCAP, D, generator=g)
    q = torch.randn(B, H, Nq, D, generator=g)
    big = torch.tensor([8.0, -8.0]).repeat(D // 2)
    for b in range(B):
        for h in range(H):
            kvh, gq = h // G, h % G
            for i in range(Nq):
                t = pin_target(place, PIN_LENS[b], Nq, NCAP, causal, gq * Nq + i, split)
                if t is None:
                    continue
                q[b, h, i] = (SCORE / D ** 0.5) * k[b, kvh, t]
                if place == "first_invisible":
                    v[b, kvh, t] = big
    return q.half(), k.half(), v.half(), PIN_LENS


# ------------------------------------------------------------------------------------------------------------------------------------
def _name(B, H, Hkv, Nq, Ncap, D, flags=0):
    buf = C.create_string_buffer(128)
    rc = capi.load().lc_attn_decode_kernel_name(B, H, Hkv, Nq, Ncap, D, flags, buf, 128)
    return rc, buf.value.decode()


def auto_split(groups, ncap, cus):
    """the documented rule, restated: the smallest S that gives every CU a workgroup, >= 4 tiles of Ncap per range, <= 64"""
    tiles = (ncap + 63) // 64
    return max(1, min(-(-cus // groups), tiles // 4, 64))


@pytest.fixture
def knobs(built):
    capi.load()
    yield
    capi.tune("attn_decode_split", 0)
    capi.tune("rule_cus", 0)


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

def _moved(truth, nks, wrong):
    """[B, H, Nq]: largest |wrong - truth| / bound over a row's columns, the bound being that of the row's visible keys"""
    atol = np.array([[tol.attn_max_abs(int(n)) for n in row] for row in nks]).reshape(nks.shape[0], 1, nks.shape[1], 1)
    bound = atol + tol.ATTN_RTOL_F16 * np.abs(truth.astype(np.float64))
    return (np.abs(wrong.astype(np.float64) - truth) / bound).max(axis=-1)


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
