"""Chunked-prefill attention over the three KV caches on the GPU (lc_attn_chunk_f16 / _paged_f16 / _paged_kv8; capi.attn_chunk*): the decode
calls with R = (H / Hkv) x Nq > 64.  Correctness is (a) every row against the CPU oracle (tests/decode_lib.py decode_truth / check_decode:
tol.attn_close with N = the row's visible keys — the decode calls' bound, no new tolerance), (b) BIT equality between the cache kinds at equal
S, (c) BIT equality with the decode entries wherever a chunk call states a decode call: R <= 64, and every 64-row block of an aligned call.
Shapes, inputs and the calls under a forced split: tests/chunk_lib.py; the proof that its pinned inputs catch a wrong row-block kernel:
tests/test_abi_cpu_chunk.py."""
import functools

import numpy as np
import pytest
import torch

from leetcuda_amd import capi as _capi_mod
from tests import chunk_lib as cl
from tests import decode_lib as dl
from tests import tol
from tests.decode_lib import _capi, _cuda, _dev_lens, _oracle, check_decode, decode_inputs, decode_truth, forced_split, gather, paginate

pytestmark = pytest.mark.gpu

CASES = [(s, cl.LENS) for s in cl.SHAPES] + [(cl.SHORT_SHAPE, cl.SHORT_LENS)]
_case_id = lambda c: "x".join(map(str, c[0])) + ("-short" if c[1] != cl.LENS else "")      # noqa: E731


def _names(B, shape, D, split, ps=16):
    H, Hkv, Nq = shape
    return forced_split(split, lambda: (_capi_mod.attn_chunk_kernel_name(B, H, Hkv, Nq, cl.NCAP, D),
                                        _capi_mod.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, cl.NCAP_PAGED // ps, D),
                                        _capi_mod.attn_chunk_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, cl.NCAP_PAGED // ps, D)))


# ---- 1. the oracle, every row of every case, the three cache kinds

@pytest.mark.parametrize("split", cl.SPLITS, ids=lambda s: f"S{s}" if s else "auto")
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("D", cl.DS)
def test_grid_against_the_oracle(D, case, causal, split):
    _capi()
    shape, lens = case
    H, Hkv, Nq = shape
    names = _names(len(lens), shape, D, split)
    for kind, name in zip(("", "_paged", "_paged_kv8"), names):
        assert name.startswith(f"attn_chunk{kind}_kernel<{D}>"), name
        assert name.endswith(f" x{split}") if split > 1 else (split == 0 or " x" not in name), name
    q, _, _ = cl.grid_inputs(D, shape, lens)
    truth, nks = cl.grid_truth(D, shape, causal, lens)
    if lens == cl.SHORT_LENS and causal:
        assert (nks == 0).sum() >= 64 + 130 and (nks > 0).any()          # rows, and a whole block, without a visible key
    worst = {}
    k, v = cl.grid_flat(D, shape, lens)
    worst["flat"] = check_decode(cl.run_flat(q, k, v, lens, causal, split).float().cpu().numpy(), truth, nks, names[0])
    truth8, nks8 = cl.grid_truth_kv8(D, shape, causal, lens)
    for ps in (16, 64):
        kp, vp, table, _, _ = cl.grid_pool(D, shape, ps, lens)
        worst[f"paged{ps}"] = check_decode(cl.run_paged(q, kp, vp, table, lens, causal, split).float().cpu().numpy(), truth, nks, names[1])
        kp8, vp8, table8, ks, vs, _, _ = cl.grid_kv8(D, shape, ps, lens)
        out8 = cl.run_kv8(q, kp8, vp8, table8, lens, ks, vs, causal, split)
        worst[f"kv8-{ps}"] = check_decode(out8.float().cpu().numpy(), truth8, nks8, names[2])
    print(f"[chunk] {names[0]} {shape} lens={lens} causal={causal}: worst |err| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


# ---- 1b. the pinned inputs whose teeth tests/test_abi_cpu_chunk.py proves

@functools.lru_cache(maxsize=None)
def _pinned_truth(D, shape, place):
    q, k, v = cl.pinned_inputs(D, shape, place)
    return decode_truth(_oracle(), q, k, v, cl.PIN_LENS, True)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("place", cl.PIN_PLACES)
@pytest.mark.parametrize("shape", cl.PIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", cl.DS)
def test_pinned_inputs(D, shape, place, split):
    """causal; one key per row outweighs the rest — the row's last visible key, or the first invisible one with a V row no blend resembles: a
    limit from the block-local row, L_blk as the limit, a straddling block cut at its last row's limit or block 0's Q rows in every block
    would move a row by >= 20 x the bound"""
    _capi()
    q, k, v = cl.pinned_inputs(D, shape, place)
    truth, nks = _pinned_truth(D, shape, place)
    worst = check_decode(cl.run_flat(q, k, v, cl.PIN_LENS, True, split).float().cpu().numpy(), truth, nks, f"pinned {place}")
    pad = lambda x: torch.cat([x, torch.zeros(*x.shape[:2], cl.NCAP_PAGED - cl.NCAP, x.shape[3], dtype=x.dtype)], dim=2)      # noqa: E731
    kp, vp, table = paginate(pad(k), pad(v), cl.PIN_LENS, 16, seed=21)
    check_decode(cl.run_paged(q, kp, vp, table, cl.PIN_LENS, True, split).float().cpu().numpy(), truth, nks, f"pinned {place} paged")
    print(f"[chunk] pinned {place} {shape} D={D} S={split}: worst |err| / bound {worst:.3f}")


# ---- 2. the cache kinds agree bit for bit at equal forced S

@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("D", cl.DS)
def test_cache_kinds_agree_bit_for_bit(D, case, causal, ps, split):
    _bits_across_kinds(D, case, causal, ps, split)


def test_cache_kinds_agree_bit_for_bit_at_256_key_pages():
    _bits_across_kinds(128, ((2, 1, 130), cl.LENS), True, 256, 3)


def _bits_across_kinds(D, case, causal, ps, split):
    _capi()
    shape, lens = case
    q, _, _ = cl.grid_inputs(D, shape, lens)
    kp, vp, table, kflat, vflat = cl.grid_pool(D, shape, ps, lens)
    paged = cl.run_paged(q, kp, vp, table, lens, causal, split)
    assert torch.equal(paged, cl.run_flat(q, kflat, vflat, lens, causal, split))          # the gathered cache: Ncap = 1024, NaN past L_b
    kp8, vp8, table8, ks, vs, kpd, vpd = cl.grid_kv8(D, shape, ps, lens)
    assert torch.equal(cl.run_kv8(q, kp8, vp8, table8, lens, ks, vs, causal, split), cl.run_paged(q, kpd, vpd, table8, lens, causal, split))
    assert torch.isfinite(paged).all()


# ---- 3. R <= 64 through the chunk entries is the decode call

@pytest.mark.parametrize("split", [0, 1, 3])
@pytest.mark.parametrize("shape_nq", [((3, 8, 2), 5), ((3, 8, 2), 16), ((2, 4, 4), 64), ((2, 4, 1), 1)], ids=str)
@pytest.mark.parametrize("D", cl.DS)
def test_up_to_64_rows_is_the_decode_call(D, shape_nq, split):
    capi = _capi()
    (B, H, Hkv), Nq = shape_nq
    lens = dl.GRID_LENS[B]
    ps, mp = 16, cl.NCAP_PAGED // 16
    q, k, v = decode_inputs(B, H, Hkv, Nq, cl.NCAP_PAGED, D, seed=cl.seed_of(D, H, Hkv, Nq))
    kp, vp, table = paginate(k, v, lens, ps, seed=3)
    ks, vs = dl.scales(dl.K_SCALES, Hkv), dl.scales(dl.V_SCALES, Hkv)
    kp8, vp8, table8 = paginate(dl.quantize(k, ks), dl.quantize(v, vs), lens, ps, seed=3, fill=dl.NAN_BYTE)
    same = forced_split(split, lambda: (capi.attn_chunk_kernel_name(B, H, Hkv, Nq, cl.NCAP_PAGED, D) == capi.attn_decode_kernel_name(B, H, Hkv, Nq, cl.NCAP_PAGED, D),
                                        capi.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D) == capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D),
                                        capi.attn_chunk_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D)
                                        == capi.attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D)))
    assert same == (True, True, True)
    for causal in (False, True):
        ref = dl.run_flat(capi, q, k, v, lens, causal, split)
        assert torch.isfinite(ref).all()
        assert torch.equal(cl.run_flat(q, k, v, lens, causal, split), ref)
        assert torch.equal(cl.run_paged(q, kp, vp, table, lens, causal, split), dl.run_paged(capi, q, kp, vp, table, lens, causal, split))
        assert torch.equal(cl.run_kv8(q, kp8, vp8, table8, lens, ks, vs, causal, split),
                           dl.run_kv8(capi, q, kp8, vp8, table8, lens, ks, vs, causal, split))


# ---- 4. a 64-row block of an aligned call is a decode call

@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("heads", [(2, 2), (4, 2), (2, 1)], ids=str)
@pytest.mark.parametrize("D", cl.DS)
def test_aligned_blocks_are_decode_calls(D, heads, causal, split):
    _aligned(D, heads, causal, split, paged=False)


def test_aligned_blocks_are_decode_calls_paged():
    _aligned(128, (4, 2), True, 3, paged=True)


def _aligned(D, heads, causal, split, paged):
    """rows [:, kvh G + g, 64 j : 64 j + 64] of the chunk call's O = attn_decode on that Q slice (H' = Hkv, Nq' = 64) with kv_len' = L_blk"""
    capi = _capi()
    H, Hkv = heads
    Nq, G = 128, H // Hkv
    lens = (1000, 129, 65)
    ncap = cl.NCAP_PAGED if paged else cl.NCAP
    q, k, v = decode_inputs(3, H, Hkv, Nq, ncap, D, seed=cl.seed_of(D, H, Hkv, Nq) + 5)
    qg, = _cuda(q)
    if paged:
        kp, vp, table = paginate(k, v, lens, 16, seed=4, fill=0.0)                       # (a decode call at kv_len' < L_b still reads below L_b only)
        out = cl.run_paged(q, kp, vp, table, lens, causal, split)
    else:
        out = cl.run_flat(q, k, v, lens, causal, split)
    assert torch.isfinite(out).all()
    for g in range(G):
        for j in range(2):
            qs = qg.view(3, Hkv, G, Nq, D)[:, :, g, 64 * j:64 * j + 64].contiguous()       # [B, Hkv, 64, D]
            sub = tuple(min(max(L - 128 + 64 * (j + 1), 0), ncap) if causal else L for L in lens)
            if paged:
                ref = dl.run_paged(capi, qs, kp, vp, table, sub, causal, split)
            else:
                ref = dl.run_flat(capi, qs, k, v, sub, causal, split)
            got = out.view(3, Hkv, G, Nq, D)[:, :, g, 64 * j:64 * j + 64]
            assert torch.equal(got, ref), (g, j)


# ---- 5. what lies past L_b never matters

@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_tails_spare_pages_and_unused_table_entries_never_matter(causal, split):
    _capi()
    D, shape, lens, ps = 128, (4, 2, 48), (999, 129, 65), 16
    H, Hkv, Nq = shape
    q, k, v = decode_inputs(3, H, Hkv, Nq, cl.NCAP_PAGED, D, seed=71)
    tail = torch.arange(cl.NCAP_PAGED).view(1, 1, -1, 1) >= torch.tensor(lens).view(-1, 1, 1, 1)
    ref_flat = cl.run_flat(q, k.masked_fill(tail, 0.0), v.masked_fill(tail, 0.0), lens, causal, split)
    kp, vp, table = paginate(k, v, lens, ps, seed=7, fill=0.0)
    ref = cl.run_paged(q, kp, vp, table, lens, causal, split)
    ks, vs = dl.scales(dl.K_SCALES, Hkv), dl.scales(dl.V_SCALES, Hkv)
    k8, v8 = dl.quantize(k, ks), dl.quantize(v, vs)
    kp8, vp8, table8 = paginate(k8, v8, lens, ps, seed=7, fill=0)
    ref8 = cl.run_kv8(q, kp8, vp8, table8, lens, ks, vs, causal, split)
    assert torch.isfinite(ref).all() and torch.equal(ref, ref_flat) and torch.isfinite(ref8).all()
    for fill in (float("nan"), float("inf"), -float("inf")):
        assert torch.equal(cl.run_flat(q, k.masked_fill(tail, fill), v.masked_fill(tail, fill), lens, causal, split), ref_flat), fill
        kp, vp, table2 = paginate(k, v, lens, ps, seed=7, fill=fill)
        assert torch.equal(table2, table) and not torch.isfinite(kp).all()
        assert torch.equal(cl.run_paged(q, kp, vp, table, lens, causal, split), ref), fill
        garbage = table.clone()                                      # entries past ceil(L_b / page_size): never read (and clamped if they were)
        for b, L in enumerate(lens):
            garbage[b, -(-L // ps):] = torch.tensor([2 ** 31 - 1, -7, 10 ** 6])[torch.arange(cl.NCAP_PAGED // ps - -(-L // ps)) % 3]
        assert torch.equal(cl.run_paged(q, kp, vp, garbage, lens, causal, split), ref), fill
    for code in (0x7F, 0xFF):
        kp8, vp8, _ = paginate(k8, v8, lens, ps, seed=7, fill=code)
        assert torch.equal(cl.run_kv8(q, kp8, vp8, table8, lens, ks, vs, causal, split), ref8), code


# ---- 6. nothing outside O is written

@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("shape", [(2, 2, 65), (2, 1, 130)], ids=str)
@pytest.mark.parametrize("D", cl.DS)
def test_output_guard(D, shape, split):
    """O is a view in the middle of a NaN-filled buffer; R = 65: the 63 padding rows of the last block store nothing"""
    _capi()
    H, Hkv, Nq = shape
    B, lens = 2, (129, 1000)
    q, k, v = decode_inputs(B, H, Hkv, Nq, cl.NCAP_PAGED, D, seed=9 + D + Nq)
    truth, nks = decode_truth(_oracle(), q, k, v, lens, False)
    kp, vp, table = paginate(k, v, lens, 16, seed=8)
    n = B * H * Nq * D
    guard = 64 * D
    for kind in ("flat", "paged"):
        buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.half, device="cuda")
        o = buf[guard:guard + n].view(B, H, Nq, D)
        if kind == "flat":
            cl.run_flat(q, k, v, lens, False, split, o=o)
        else:
            cl.run_paged(q, kp, vp, table, lens, False, split, o=o)
        assert torch.isfinite(o).all(), kind
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all(), kind
        check_decode(o.float().cpu().numpy(), truth, nks, f"guard {kind}")


# ---- 7. one batch entry's bits do not depend on the others

@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_batch_invariance(causal, split):
    _capi()
    D, shape = 128, (2, 1, 130)
    H, Hkv, Nq = shape
    q, k, v = decode_inputs(3, H, Hkv, Nq, cl.NCAP, D, seed=77)
    a = cl.run_flat(q, k, v, (1000, 333, 65), causal, split)
    b = cl.run_flat(q, k, v, (7, 333, 1000), causal, split)
    one = cl.run_flat(q[1:2].contiguous(), k[1:2].contiguous(), v[1:2].contiguous(), (333,), causal, split)
    assert torch.isfinite(a[1]).all()
    assert torch.equal(a[1], b[1]) and torch.equal(a[1], one[0])
    assert not torch.equal(a[0], b[0])


# ---- 8. graph capture

def test_graph_capture_with_a_caller_workspace_and_in_place_rewrites():
    """captured once with a caller workspace (S = 3) and replayed: the eager bits.  Then kv_len, block_table, the pages and Q are rewritten IN
    PLACE: the replay has the bits of an eager call on the new state, and matches the oracle"""
    capi = _capi()
    D, ps, shape = 128, 16, (4, 2, 48)
    H, Hkv, Nq = shape
    B, mp = 3, cl.NCAP_PAGED // ps
    lens = (500, 129, 64)
    q, k, v = decode_inputs(B, H, Hkv, Nq, cl.NCAP_PAGED, D, seed=33 + D)
    kp, vp, table = paginate(k, v, lens, ps, seed=9, spare=40)
    q, kp, vp, table = _cuda(q, kp, vp, table)
    lens_dev = _dev_lens(lens)
    capi.tune("attn_decode_split", 3)
    try:
        name = capi.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D)
        assert name == "attn_chunk_paged_kernel<128> x3"
        ws = torch.empty(capi.attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D), dtype=torch.uint8, device="cuda")
        assert ws.numel() == 3 * B * H * Nq * (D + 1) * 4
        eager = torch.full_like(q, float("nan"))
        capi.attn_chunk_paged(q, kp, vp, eager, table, lens_dev, causal=True, workspace=ws)
        o = torch.full_like(q, float("nan"))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            capi.attn_chunk_paged(q, kp, vp, o, table, lens_dev, causal=True, workspace=ws)      # warm-up on the capture stream
            torch.cuda.synchronize()
            o.fill_(float("nan"))
            with torch.cuda.graph(g, stream=st):
                capi.attn_chunk_paged(q, kp, vp, o, table, lens_dev, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.isnan(o).all()               # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager)
        gen = torch.Generator().manual_seed(4)
        new_lens = (577, 48, 300)
        k2, v2 = (torch.randn(k.shape, generator=gen).half() for _ in range(2))
        kp2, vp2, table2 = paginate(k2, v2, new_lens, ps, seed=10, spare=40)
        assert not torch.equal(table2.cuda(), table)
        kp.copy_(kp2)
        vp.copy_(vp2)
        table.copy_(table2)
        lens_dev.copy_(torch.tensor(new_lens, dtype=torch.int32))
        q.copy_(torch.randn(q.shape, generator=gen).half())
        g.replay()
        torch.cuda.synchronize()
        again = torch.full_like(q, float("nan"))
        capi.attn_chunk_paged(q, kp, vp, again, table, lens_dev, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(o, again)
        truth, nks = decode_truth(_oracle(), q.cpu(), k2, v2, new_lens, True)
        check_decode(o.float().cpu().numpy(), truth, nks, f"replay {name}")
    finally:
        capi.tune("attn_decode_split", 0)


def test_graph_capture_without_a_workspace_runs_one_range():
    """no caller buffer while the stream is being captured: S = 1 runs, with the bits of the eager S = 1 call, and matches the oracle"""
    capi = _capi()
    D, shape, lens = 64, (2, 1, 130), cl.LENS
    q, _, _ = cl.grid_inputs(D, shape)
    truth, nks = cl.grid_truth(D, shape, True)
    k, v = cl.grid_flat(D, shape)
    s1 = cl.run_flat(q, k, v, lens, True, 1)
    qg, = _cuda(q)
    lens_dev = _dev_lens(lens)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    o = torch.full_like(qg, float("nan"))
    o2 = torch.full_like(qg, float("nan"))
    capi.tune("attn_decode_split", 3)
    try:
        with torch.cuda.stream(st):
            capi.attn_chunk(qg, k, v, o2, lens_dev, causal=True)            # split through the stream's cached workspace
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                capi.attn_chunk(qg, k, v, o, lens_dev, causal=True)
        g.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    assert torch.equal(o2, cl.run_flat(q, k, v, lens, True, 3))
    assert torch.equal(o, s1)
    check_decode(o.float().cpu().numpy(), truth, nks, "captured without a workspace")


# ---- 9. a prefill in chunks, end to end

@pytest.mark.parametrize("kv8", [False, True], ids=["f16", "kv8"])
def test_a_prefill_in_chunks_end_to_end(kv8):
    """a 320-token prompt in chunks of 128, 128 and 64: kv_append_paged, then attn_chunk_paged(causal) per chunk.  The concatenated O is causal
    attention over the whole prompt (the oracle; fp8: on the dequantised pool) and agrees with attn_fwd_gqa(causal) on the contiguous prompt"""
    capi = _capi()
    B, H, Hkv, D, ps, N = 2, 8, 2, 128, 16, 320
    mp = 24
    q, k, v = decode_inputs(B, H, Hkv, N, N, D, seed=320)
    perm = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(5))
    table = perm[:B * mp].view(B, mp).to(torch.int32).cuda()
    ks, vs = _cuda(dl.scales(dl.K_SCALES, Hkv), dl.scales(dl.V_SCALES, Hkv))
    if kv8:
        kp, vp = (torch.full((B * mp + 3, Hkv, ps, D), dl.NAN_BYTE, dtype=torch.uint8, device="cuda") for _ in range(2))
    else:
        kp, vp = (torch.full((B * mp + 3, Hkv, ps, D), float("nan"), dtype=torch.half, device="cuda") for _ in range(2))
    outs, done = [], 0
    for n in (128, 128, 64):
        lens_dev = torch.full((B,), done + n, dtype=torch.int32, device="cuda")
        kn, vn, qn = _cuda(k[:, :, done:done + n].contiguous(), v[:, :, done:done + n].contiguous(), q[:, :, done:done + n].contiguous())
        o = torch.full_like(qn, float("nan"))
        if kv8:
            capi.kv_append_paged_kv8(kn, vn, kp, vp, table, lens_dev, ks, vs)
            capi.attn_chunk_paged_kv8(qn, kp, vp, o, table, lens_dev, ks, vs, causal=True)
        else:
            capi.kv_append_paged(kn, vn, kp, vp, table, lens_dev)
            capi.attn_chunk_paged(qn, kp, vp, o, table, lens_dev, causal=True)
        outs.append(o)
        done += n
    torch.cuda.synchronize()
    out = torch.cat(outs, dim=2)
    assert torch.isfinite(out).all()
    if kv8:      # the cache as the pool holds it
        kc = gather(dl.dequant(kp.cpu(), ks.cpu()), table.cpu())[:, :, :N].contiguous()
        vc = gather(dl.dequant(vp.cpu(), vs.cpu()), table.cpu())[:, :, :N].contiguous()
        assert torch.isfinite(kc).all() and torch.isfinite(vc).all()
    else:
        kc, vc = k, v
        assert torch.equal(gather(kp.cpu(), table.cpu())[:, :, :N], k)
    truth, nks = decode_truth(_oracle(), q, kc, vc, (N,) * B, True)
    assert [int(x) for x in nks[0]] == list(range(1, N + 1))
    worst = check_decode(out.float().cpu().numpy(), truth, nks, "chunked prefill")
    qg, kg, vg = _cuda(q, kc, vc)
    fwd = torch.full_like(qg, float("nan"))
    capi.attn_fwd_gqa(qg, kg, vg, fwd, causal=True)
    torch.cuda.synchronize()
    check_decode(fwd.float().cpu().numpy(), truth, nks, "attn_fwd_gqa(causal)")
    agree = check_decode(out.float().cpu().numpy(), fwd.float().cpu().numpy(), nks, "chunked prefill against attn_fwd_gqa(causal)")
    print(f"[chunk] prefill in chunks kv8={kv8}: worst |err| / bound {worst:.3f} (oracle), {agree:.3f} (attn_fwd_gqa)")


# ---- 10. one model-sized shape

def test_one_model_sized_shape():
    """(B, H, Hkv, Nq, L, D) = (2, 32, 8, 512, 4096, 128) in pages of 16 keys, causal, auto split: the first and the last row of every row
    block of two K / V heads against the oracle (R = 2048: 32 row blocks per K / V head)"""
    capi = _capi()
    B, H, Hkv, Nq, Ncap, D, ps = 2, 32, 8, 512, 4096, 128, 16
    G, lens = H // Hkv, (4096, 2500)
    name = capi.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, Ncap // ps, D, causal=True)
    assert name.startswith("attn_chunk_paged_kernel<128>"), name
    q, k, v = decode_inputs(B, H, Hkv, Nq, Ncap, D, seed=4096)
    kp, vp, table = paginate(k, v, lens, ps, seed=12)
    out = cl.run_paged(q, kp, vp, table, lens, True).cpu()
    assert torch.isfinite(out).all()
    orc, worst, rows = _oracle(), 0.0, 0
    for b in range(B):
        for kvh in (0, Hkv - 1):
            for rb in range(cl.rb_of(H, Hkv, Nq)):
                for r in (64 * rb, 64 * rb + 63):
                    h, i = kvh * G + r // Nq, r % Nq
                    nk = dl.visible(lens[b], Nq, Ncap, True, i)
                    t = orc.attn_rows(q[b, h, i].view(1, 1, D), k[b, kvh, :nk].contiguous().view(1, nk, D), v[b, kvh, :nk].contiguous().view(1, nk, D),
                                      1, 1, nk, D)[0, 0]
                    o = out[b, h, i].float().numpy()
                    ok, err, excess = tol.attn_close(o, t, N=nk)
                    bound = tol.attn_max_abs(nk) + tol.ATTN_RTOL_F16 * np.abs(t.astype(np.float64))
                    worst = max(worst, float((np.abs(o.astype(np.float64) - t) / bound).max()))
                    rows += 1
                    assert ok, (name, f"batch {b} head {h} token {i} nk {nk}: max |err| {err:.3e}, excess {excess:.3e}")
    assert rows == B * 2 * 32 * 2
    print(f"[chunk] {name}: {rows} rows, worst |err| / bound {worst:.3f}")
