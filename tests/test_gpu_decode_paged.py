"""Decode attention over a PAGED KV cache on the GPU (lc_attn_decode_paged_f16 / capi.attn_decode_paged).  Correctness is (a) every row against
the CPU oracle on the logical cache (tests/decode_lib.py decode_truth / check_decode, tol.attn_close with N = the row's visible keys)
and (b) BIT equality with capi.attn_decode — an existing, separately tested call — on the gathered contiguous cache of Ncap = max_pages x
page_size under the same split.  Ncap = 1024 throughout; pools come from tests/decode_lib.py `paginate`: scattered pages, NaN in
every pool row of a position >= L_b and in the spare page every unused table entry names.  No test feeds an out-of-range page id."""
import functools

import numpy as np
import pytest
import torch

from tests.decode_lib import NCAP_POW2 as NCAP
from tests.decode_lib import (GRID_SHAPES, _capi, _cuda, _dev_lens, _lens_of, _oracle, check_decode, decode_inputs, decode_truth, forced_split, gather,
                              paginate, rt_of, seam_inputs)
from tests.decode_lib import run_flat as _run_flat
from tests.decode_lib import run_paged as _run_paged

pytestmark = pytest.mark.gpu


def _names(capi, B, H, Hkv, Nq, ps, D, split):
    return forced_split(split, lambda: (capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, NCAP // ps, D),
                                        capi.attn_decode_kernel_name(B, H, Hkv, Nq, NCAP, D)))


@functools.lru_cache(maxsize=4)
def _grid_case(D, shape, Nq, causal):
    B, H, Hkv = shape
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=D * 1000 + H * 100 + Hkv * 10 + Nq)
    lens = _lens_of(B, Hkv)
    truth, nks = decode_truth(_oracle(), q, k, v, lens, causal)
    return q, k, v, lens, truth, nks


@functools.lru_cache(maxsize=4)
def _grid_pool(D, shape, Nq, causal, ps):
    q, k, v, lens, _, _ = _grid_case(D, shape, Nq, causal)
    kp, vp, table = paginate(k, v, lens, ps, seed=ps + Nq)
    return _cuda(kp, vp, table, gather(kp, table), gather(vp, table))


@pytest.mark.parametrize("split", [0, 1, 3, 8])
@pytest.mark.parametrize("ps", [16, 64, 256])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Nq", [1, 5, 16])
@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", [64, 128])
def test_grid_against_the_oracle_and_the_contiguous_call(D, shape, Nq, causal, ps, split):
    capi = _capi()
    B, H, Hkv = shape
    name, flat_name = _names(capi, B, H, Hkv, Nq, ps, D, split)
    assert name.startswith(f"attn_decode_paged_kernel<{D},{rt_of(H, Hkv, Nq)}>") and name.replace("_paged", "") == flat_name
    if split == 1:
        assert " x" not in name
    elif split > 1:
        assert name.endswith(f" x{split}")
    q, k, v, lens, truth, nks = _grid_case(D, shape, Nq, causal)
    kp, vp, table, kflat, vflat = _grid_pool(D, shape, Nq, causal, ps)
    out = _run_paged(capi, q, kp, vp, table, lens, causal, split)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, name)
    assert torch.equal(out, _run_flat(capi, q, kflat, vflat, lens, causal, split)), name
    print(f"[decode paged] {name} {shape} Nq={Nq} page={ps} causal={causal}: worst |err| / bound {worst:.3f}")


EDGE_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024)


@functools.lru_cache(maxsize=2)
def _edge_case(D, causal):
    B, H, Hkv, Nq = len(EDGE_LENS), 4, 2, 5
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=177 + D)
    truth, nks = decode_truth(_oracle(), q, k, v, EDGE_LENS, causal)
    return q, k, v, truth, nks


@pytest.mark.parametrize("split", [1, 8])
@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_length_edges_in_one_launch(D, causal, ps, split):
    """one batch entry per L, around every page and tile seam: L = 0 uses no table entry at all, L = 1024 every one"""
    capi = _capi()
    q, k, v, truth, nks = _edge_case(D, causal)
    kp, vp, table = paginate(k, v, EDGE_LENS, ps, seed=5)
    out = _run_paged(capi, q, kp, vp, table, EDGE_LENS, causal, split)
    check_decode(out.float().cpu().numpy(), truth, nks, f"edges D={D} page={ps} S={split}")
    assert torch.equal(out, _run_flat(capi, q, gather(kp, table), gather(vp, table), EDGE_LENS, causal, split))


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
def test_a_contiguous_cache_is_a_pool_without_a_copy(D, split):
    """[B,Hkv,1024,D] handed over as a pool of B pages of 1024 keys: table [[0],[1],[2]] is the contiguous call; [[2],[1],[0]] the contiguous
    call on the batch-flipped cache"""
    capi = _capi()
    B, H, Hkv, Nq = 3, 8, 2, 4
    lens = (700, 129, 1000)
    q, k, v = _cuda(*decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=41 + D))
    ident = torch.arange(B, dtype=torch.int32, device="cuda").view(B, 1)
    assert capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, NCAP, 1, D).startswith(f"attn_decode_paged_kernel<{D},1>")
    for causal in (False, True):
        flat = _run_flat(capi, q, k, v, lens, causal, split)
        assert torch.isfinite(flat).all()
        assert torch.equal(_run_paged(capi, q, k, v, ident, lens, causal, split), flat)
        flipped = _run_flat(capi, q, k.flip(0).contiguous(), v.flip(0).contiguous(), lens, causal, split)
        assert torch.equal(_run_paged(capi, q, k, v, ident.flip(0).contiguous(), lens, causal, split), flipped)
        assert not torch.equal(flipped, flat)


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("ps", [16, 64])
def test_placement_invariance(ps, split):
    """the same logical cache under two pool permutations and with 3 or 40 spare pages: the same bits"""
    capi = _capi()
    B, H, Hkv, Nq, D = 3, 8, 2, 5, 128
    lens = (1000, 129, 65)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=51)
    outs = []
    tables = []
    for seed, spare in ((1, 3), (2, 3), (3, 40)):
        kp, vp, table = paginate(k, v, lens, ps, seed=seed, spare=spare)
        tables.append(table)
        outs.append(_run_paged(capi, q, kp, vp, table, lens, True, split))
    assert not torch.equal(tables[0], tables[1])
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
def test_shared_prefix(D, split):
    """two batch entries whose first n table entries name the SAME physical pages (prefix sharing): the contiguous call on a cache into which
    the prefix was copied"""
    capi = _capi()
    B, H, Hkv, Nq, ps, n = 2, 8, 2, 2, 16, 19
    lens = (500, 777)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=61 + D)
    kp, vp, table = paginate(k, v, lens, ps, seed=6)
    table[1, :n] = table[0, :n]
    k2, v2 = k.clone(), v.clone()
    k2[1, :, :n * ps] = k[0, :, :n * ps]
    v2[1, :, :n * ps] = v[0, :, :n * ps]
    for causal in (False, True):
        out = _run_paged(capi, q, kp, vp, table, lens, causal, split)
        assert torch.equal(out, _run_flat(capi, q, k2, v2, lens, causal, split))
        truth, nks = decode_truth(_oracle(), q, k2, v2, lens, causal)
        check_decode(out.float().cpu().numpy(), truth, nks, "shared prefix")
        assert not torch.equal(out[1], _run_flat(capi, q, k, v, lens, causal, split)[1])


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("ps", [16, 128])
def test_tail_and_unused_entries_never_matter(ps, causal, split):
    """pool rows of positions >= L_b and the spare page behind every unused table entry hold NaN, then zeros, then +-Inf: the same bits"""
    capi = _capi()
    B, H, Hkv, Nq, D = 3, 8, 2, 5, 128
    lens = (999, 129, 65)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=71)
    kp, vp, table = paginate(k, v, lens, ps, seed=7, fill=0.0)
    ref = _run_paged(capi, q, kp, vp, table, lens, causal, split)
    assert torch.isfinite(ref).all()
    for fill in (float("nan"), float("inf"), -float("inf")):
        kp, vp, table2 = paginate(k, v, lens, ps, seed=7, fill=fill)
        assert torch.equal(table2, table) and not torch.isfinite(kp).all()
        assert torch.equal(_run_paged(capi, q, kp, vp, table, lens, causal, split), ref), fill


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("ps", [16, 64])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_pinned_page_seam_inputs(D, causal, ps, split):
    """one key per row, next to a page seam, outweighs the rest: a kernel that ignores the table, is off by one page, reads another batch
    entry's table row, ignores the K / V head in the page base or wraps the in-page offset moves the row by >= 20 x the bound
    (tests/test_abi_cpu_decode_paged.py)"""
    capi = _capi()
    q, k, v, lens = seam_inputs(D, causal)
    truth, nks = _seam_truth(D, causal)
    kp, vp, table = paginate(k, v, lens, ps, seed=17 + D)
    out = _run_paged(capi, q, kp, vp, table, lens, causal, split)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, f"pinned seams D={D} page={ps} S={split}")
    print(f"[decode paged] pinned seams D={D} page={ps} causal={causal} S={split}: worst |err| / bound {worst:.3f}")


@functools.lru_cache(maxsize=4)
def _seam_truth(D, causal):
    q, k, v, lens = seam_inputs(D, causal)
    return decode_truth(_oracle(), q, k, v, lens, causal)


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("Nq", [5, 20], ids=["R5", "R20"])
@pytest.mark.parametrize("D", [64, 128])
def test_output_guard(D, Nq, split):
    """O is a view in the middle of a NaN-filled buffer (R = 5 and R = 20: padded row tiles): everything outside stays NaN, O is all finite"""
    capi = _capi()
    B, H, Hkv = 2, 2, 2                       # G = 1: R = Nq
    lens = (129, 1000)
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=9 + D + Nq)
    kp, vp, table = paginate(k, v, lens, 16, seed=8)
    n = B * H * Nq * D
    guard = 64 * D
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.half, device="cuda")
    o = buf[guard:guard + n].view(B, H, Nq, D)
    _run_paged(capi, q, kp, vp, table, lens, True, split, o=o)
    assert torch.isfinite(o).all()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    truth, nks = decode_truth(_oracle(), q, k, v, lens, True)
    check_decode(o.float().cpu().numpy(), truth, nks, "guard")


def _graph_state(D, ps):
    B, H, Hkv, Nq = 3, 8, 2, 2
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=33 + D)
    lens = (500, 129, 64)
    kp, vp, table = paginate(k, v, lens, ps, seed=9, spare=40)
    return B, H, Hkv, Nq, q.cuda(), k, v, lens, kp.cuda(), vp.cuda(), table.cuda(), _dev_lens(lens)


@pytest.mark.parametrize("split", [4, 0], ids=["S4", "auto"])
def test_graph_capture_with_a_caller_workspace(split):
    """captured once with a caller workspace and replayed: the eager bits.  Then one decode step: a new K / V row per sequence, every page moved
    to another pool slot, block_table and kv_len rewritten IN PLACE; the replay has the bits of an eager call on the new state (only the kernel
    reads the table and kv_len)"""
    capi = _capi()
    D, ps = 128, 16
    B, H, Hkv, Nq, q, k, v, lens, kp, vp, table, dl = _graph_state(D, ps)
    mp = NCAP // ps
    capi.tune("attn_decode_split", split)
    try:
        name = capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D)
        ws = torch.empty(max(capi.attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D), 16), dtype=torch.uint8, device="cuda")
        if split == 4:
            assert name.endswith(" x4") and ws.numel() == 4 * B * H * Nq * (D + 1) * 4
        eager = torch.full_like(q, float("nan"))
        capi.attn_decode_paged(q, kp, vp, eager, table, dl, causal=True, workspace=ws)
        o = torch.full_like(q, float("nan"))
        st = torch.cuda.Stream()                 # (a non-default stream: capture needs one)
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            capi.attn_decode_paged(q, kp, vp, o, table, dl, causal=True, workspace=ws)      # warm-up on the capture stream
            torch.cuda.synchronize()
            o.fill_(float("nan"))
            with torch.cuda.graph(g, stream=st):
                capi.attn_decode_paged(q, kp, vp, o, table, dl, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.isnan(o).all()               # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager)
        # ---- the next decode step, in place: one more row per sequence, pages moved, table and kv_len rewritten
        gen = torch.Generator().manual_seed(4)
        for b in range(B):
            k[b, :, lens[b]] = torch.randn(Hkv, D, generator=gen).half()
            v[b, :, lens[b]] = torch.randn(Hkv, D, generator=gen).half()
        new_lens = tuple(x + 1 for x in lens)
        kp2, vp2, table2 = paginate(k, v, new_lens, ps, seed=10, spare=40)
        assert not torch.equal(table2.cuda(), table)
        kp.copy_(kp2)
        vp.copy_(vp2)
        table.copy_(table2)
        dl += 1
        q.copy_(torch.randn(q.shape, generator=gen).half())
        g.replay()
        torch.cuda.synchronize()
        assert tuple(int(x) for x in dl.cpu()) == (501, 130, 65)
        again = torch.full_like(q, float("nan"))
        capi.attn_decode_paged(q, kp, vp, again, table, dl, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(o, again)
        truth, nks = decode_truth(_oracle(), q.cpu(), k, v, new_lens, True)
        check_decode(o.float().cpu().numpy(), truth, nks, f"replay {name}")
    finally:
        capi.tune("attn_decode_split", 0)


def test_graph_capture_without_a_workspace_runs_one_range():
    """no caller buffer while the stream is being captured: the S = 1 kernel runs and matches the eager S = 1 call bit for bit"""
    capi = _capi()
    D, ps = 64, 64
    B, H, Hkv, Nq, q, k, v, lens, kp, vp, table, dl = _graph_state(D, ps)
    s1 = _run_paged(capi, q, kp, vp, table, dl, False, 1)
    s4 = _run_paged(capi, q, kp, vp, table, dl, False, 4)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    o = torch.full_like(q, float("nan"))
    o2 = torch.full_like(q, float("nan"))
    capi.tune("attn_decode_split", 4)
    try:
        with torch.cuda.stream(st):
            capi.attn_decode_paged(q, kp, vp, o2, table, dl)            # a non-default stream, split through the stream's cached workspace
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                capi.attn_decode_paged(q, kp, vp, o, table, dl)
        g.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    assert torch.equal(o2, s4)
    assert torch.equal(o, s1)


def test_one_model_sized_shape():
    """(4, 32 / 8, Nq 1, Ncap 8192, D 128) in pages of 16 keys — a 2051-page pool, a [4, 512] table — lengths {8192, 8191, 4097, 1}, auto split:
    all 128 rows against the oracle, and the bits of the contiguous call"""
    capi = _capi()
    B, H, Hkv, Nq, Ncap, D, ps = 4, 32, 8, 1, 8192, 128, 16
    lens = (8192, 8191, 4097, 1)
    q, k, v = decode_inputs(B, H, Hkv, Nq, Ncap, D, seed=8192)
    name = capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, Ncap // ps, D)
    assert name.startswith("attn_decode_paged_kernel<128,1> x"), name      # 32 head groups do not fill the GPU: split
    kp, vp, table = paginate(k, v, lens, ps, seed=12)
    assert kp.shape[0] == 2051
    truth, nks = decode_truth(_oracle(), q, k, v, lens, False)
    out = _run_paged(capi, q, kp, vp, table, lens, False)
    worst = check_decode(out.float().cpu().numpy(), truth, nks, name)
    assert torch.equal(out, _run_flat(capi, q, k, v, lens, False))
    print(f"[decode paged] {name}: worst |err| / bound {worst:.3f}")
