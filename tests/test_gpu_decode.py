"""Decode attention over a KV cache on the GPU (lc_attn_decode_f16 / capi.attn_decode): every row of every case against the CPU oracle
(tests/decode_lib.py decode_truth) under tol.attn_close with N = the row's visible keys; rows without a visible key exactly 0.
The shapes are small (Ncap = 1000) so that every row is checked; the split path is reached through "attn_decode_split" (ranges may be
empty).  Inputs, truth and the pinned construction (tests/decode_lib.py) are shared with tests/test_abi_cpu_decode.py, which proves on the CPU
that the pinned inputs have teeth."""
import functools

import numpy as np
import pytest
import torch

from tests.decode_lib import NCAP_RAGGED as NCAP
from tests.decode_lib import (GRID_NQ, GRID_SHAPES, PLACES, _capi, _lens_of, _oracle, check_decode, decode_inputs, decode_truth, forced_split,
                              pinned_inputs, rt_of)
from tests.decode_lib import run_flat as _run

pytestmark = pytest.mark.gpu


def _want(capi, B, H, Hkv, Nq, Ncap, D, split):
    return forced_split(split, lambda: capi.attn_decode_kernel_name(B, H, Hkv, Nq, Ncap, D))


@functools.lru_cache(maxsize=8)
def _grid_case(D, shape, Nq, causal):
    B, H, Hkv = shape
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=D * 1000 + H * 100 + Hkv * 10 + Nq)
    lens = _lens_of(B, Hkv)
    truth, nks = decode_truth(_oracle(), q, k, v, lens, causal)
    return q, k, v, lens, truth, nks


@pytest.mark.parametrize("split", [0, 1, 3, 8])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Nq", GRID_NQ)
@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", [64, 128])
def test_grid_against_the_oracle(D, shape, Nq, causal, split):
    capi = _capi()
    B, H, Hkv = shape
    name = _want(capi, B, H, Hkv, Nq, NCAP, D, split)
    assert name.startswith(f"attn_decode_kernel<{D},{rt_of(H, Hkv, Nq)}>")
    if split == 1:
        assert " x" not in name
    elif split > 1:
        assert name.endswith(f" x{split}")
    q, k, v, lens, truth, nks = _grid_case(D, shape, Nq, causal)
    out = _run(capi, q, k, v, lens, causal, split).float().cpu().numpy()
    worst = check_decode(out, truth, nks, name)
    print(f"[decode] {name} {shape} Nq={Nq} causal={causal}: worst |err| / bound {worst:.3f}")


EDGE_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=4)
def _edge_case(D, causal):
    B, H, Hkv, Nq = len(EDGE_LENS), 4, 2, 5
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=77 + D)
    truth, nks = decode_truth(_oracle(), q, k, v, EDGE_LENS, causal)
    return q, k, v, truth, nks


@pytest.mark.parametrize("split", [1, 8])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_length_edges_in_one_launch(D, causal, split):
    """one batch entry per L: causal rows straddle the 64-key seam at L = 65 ... 68 (here 65), L < Nq gives zero rows, S = 8 gives empty
    ranges whenever ceil(L / 64) < 8"""
    capi = _capi()
    q, k, v, truth, nks = _edge_case(D, causal)
    if causal:
        assert (nks[EDGE_LENS.index(2)] == [0, 0, 0, 1, 2]).all() and (nks[EDGE_LENS.index(65)] == [61, 62, 63, 64, 65]).all()
    out = _run(capi, q, k, v, EDGE_LENS, causal, split).float().cpu().numpy()
    check_decode(out, truth, nks, f"edges D={D} S={split}")


@pytest.mark.parametrize("split", [1, 3, 8])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("D", [64, 128])
def test_pinned_inputs(D, place, causal, split):
    """one key per row outweighs the rest: a key masked wrongly, a tile or a range skipped, walked twice or taken from another head or batch
    entry moves the row by >= 20 x the bound (tests/test_abi_cpu_decode.py)"""
    capi = _capi()
    q, k, v, lens = pinned_inputs(D, place, causal, split if (place == "range_seam" and split > 1) else 3)
    truth, nks = decode_truth(_oracle(), q, k, v, lens, causal)
    out = _run(capi, q, k, v, lens, causal, split).float().cpu().numpy()
    worst = check_decode(out, truth, nks, f"pinned {place} D={D} S={split}")
    print(f"[decode] pinned {place} D={D} causal={causal} S={split}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("D", [64, 128])
def test_cache_tail_never_matters(D, causal, split):
    """positions >= L_b of K and V filled with NaN, then +-Inf: the same bits as with a zero tail; and K / V / Q at the front and the back
    of NaN-filled larger allocations"""
    capi = _capi()
    B, H, Hkv, Nq = 3, 8, 2, 5
    lens = (1000 - 1, 129, 65)
    q, k, v = (x.cuda() for x in decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=5 + D))
    tail = torch.arange(NCAP, device="cuda").view(1, 1, NCAP, 1) >= torch.tensor(lens, device="cuda").view(B, 1, 1, 1)
    ref = _run(capi, q, k.masked_fill(tail, 0.0), v.masked_fill(tail, 0.0), lens, causal, split)
    assert torch.isfinite(ref).all()
    for fill in (float("nan"), float("inf"), -float("inf")):
        got = _run(capi, q, k.masked_fill(tail, fill), v.masked_fill(tail, fill), lens, causal, split)
        assert torch.equal(got, ref), fill
    # front and back of larger NaN-filled allocations (a read before the first or past the last element meets a NaN)
    pad = 4096
    for front in (True, False):
        views = []
        for x in (q, k.masked_fill(tail, 0.0), v.masked_fill(tail, 0.0)):
            buf = torch.full((x.numel() + pad,), float("nan"), dtype=torch.half, device="cuda")
            sl = buf[:x.numel()] if front else buf[pad:]
            sl.copy_(x.reshape(-1))
            views.append(sl.view(x.shape))
        got = _run(capi, *views, lens, causal, split)
        assert torch.equal(got, ref), front


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("Nq", [5, 20], ids=["R5", "R20"])
@pytest.mark.parametrize("D", [64, 128])
def test_output_guard(D, Nq, split):
    """O is a view in the middle of a NaN-filled buffer (R = 5 and R = 20: padded row tiles): everything outside stays NaN — padding rows
    are not stored — and O itself, prefilled with NaN, is all finite afterwards"""
    capi = _capi()
    B, H, Hkv = 2, 2, 2                       # G = 1: R = Nq
    q, k, v = decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=9 + D + Nq)
    n = B * H * Nq * D
    guard = 64 * D                            # more than the padding rows of the last row tile would write
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.half, device="cuda")
    o = buf[guard:guard + n].view(B, H, Nq, D)
    _run(capi, q, k, v, (129, 1000), True, split, o=o)
    assert torch.isfinite(o).all()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    truth, nks = decode_truth(_oracle(), q, k, v, (129, 1000), True)
    check_decode(o.float().cpu().numpy(), truth, nks, "guard")


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_batch_invariance(causal, split):
    """entry b of a B = 3 call has the bits of the B = 1 call on its slice under the same S, whatever the other entries' lengths are"""
    capi = _capi()
    B, H, Hkv, Nq, D = 3, 8, 2, 4, 128
    q, k, v = (x.cuda() for x in decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=21))
    lens = (700, 129, 1000)
    whole = _run(capi, q, k, v, lens, causal, split)
    other = _run(capi, q, k, v, (65, 129, 3), causal, split)
    assert torch.equal(other[1], whole[1])
    for b in range(B):
        one = _run(capi, q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), lens[b:b + 1], causal, split)
        assert torch.equal(one[0], whole[b]), b


def _graph_state(D):
    B, H, Hkv, Nq = 3, 8, 2, 2
    q, k, v = (x.cuda() for x in decode_inputs(B, H, Hkv, Nq, NCAP, D, seed=33 + D))
    return B, H, Hkv, Nq, q, k, v, torch.tensor([500, 129, 64], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("split", [4, 0], ids=["S4", "auto"])
def test_graph_capture_with_a_caller_workspace(split):
    """captured once with a caller workspace and replayed: the eager bits; then one more K / V row at position L_b, kv_len incremented in
    place, new Q in place, replay: the oracle of the new state (the kernel reads kv_len, the host never does)"""
    capi = _capi()
    D = 128
    B, H, Hkv, Nq, q, k, v, lens = _graph_state(D)
    capi.tune("attn_decode_split", split)
    try:
        name = capi.attn_decode_kernel_name(B, H, Hkv, Nq, NCAP, D)
        ws = torch.empty(max(capi.attn_decode_workspace_bytes(B, H, Hkv, Nq, NCAP, D), 16), dtype=torch.uint8, device="cuda")
        if split == 4:
            assert name.endswith(" x4") and ws.numel() == 4 * B * H * Nq * (D + 1) * 4
        eager = torch.full_like(q, float("nan"))
        capi.attn_decode(q, k, v, eager, lens, causal=True, workspace=ws)
        o = torch.full_like(q, float("nan"))
        st = torch.cuda.Stream()                 # (a non-default stream: capture needs one)
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            capi.attn_decode(q, k, v, o, lens, causal=True, workspace=ws)      # warm-up on the capture stream
            torch.cuda.synchronize()
            o.fill_(float("nan"))
            with torch.cuda.graph(g, stream=st):
                capi.attn_decode(q, k, v, o, lens, causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.isnan(o).all()               # captured, not run
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager)
        # ---- the next decode step, in place
        gen = torch.Generator().manual_seed(4)
        for b in range(B):
            L = int(lens[b])
            k[b, :, L] = torch.randn(Hkv, D, generator=gen).half().cuda()
            v[b, :, L] = torch.randn(Hkv, D, generator=gen).half().cuda()
        lens += 1
        q.copy_(torch.randn(q.shape, generator=gen).half())
        g.replay()
        torch.cuda.synchronize()
        new_lens = tuple(int(x) for x in lens.cpu())
        assert new_lens == (501, 130, 65)
        truth, nks = decode_truth(_oracle(), q.cpu(), k.cpu(), v.cpu(), new_lens, True)
        check_decode(o.float().cpu().numpy(), truth, nks, f"replay {name}")
    finally:
        capi.tune("attn_decode_split", 0)


def test_graph_capture_without_a_workspace_runs_one_range():
    """no caller buffer while the stream is being captured: the S = 1 kernel runs (no allocation inside a capture) and matches the eager
    S = 1 call bit for bit; the same call on a non-default stream outside a capture"""
    capi = _capi()
    D = 64
    B, H, Hkv, Nq, q, k, v, lens = _graph_state(D)
    s1 = _run(capi, q, k, v, lens, False, 1)
    s4 = _run(capi, q, k, v, lens, False, 4)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    o = torch.full_like(q, float("nan"))
    o2 = torch.full_like(q, float("nan"))
    capi.tune("attn_decode_split", 4)
    try:
        with torch.cuda.stream(st):
            capi.attn_decode(q, k, v, o2, lens)            # a non-default stream, split through the stream's cached workspace
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                capi.attn_decode(q, k, v, o, lens)
        g.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    assert torch.equal(o2, s4)
    assert torch.equal(o, s1)


def test_agreement_with_prefill():
    """Nq = Ncap = 64, kv_len = NULL, causal: the decode entry and the causal prefill entry are both within the bound of the oracle"""
    capi = _capi()
    B, H, N, D = 2, 2, 64, 128
    q, k, v = decode_inputs(B, H, H, N, N, D, seed=64)
    truth, nks = decode_truth(_oracle(), q, k, v, None, True)
    assert (nks == np.arange(1, N + 1)).all()
    assert capi.attn_decode_kernel_name(B, H, H, N, N, D, causal=True) == "attn_decode_kernel<128,4>"
    out = _run(capi, q, k, v, None, True).float().cpu().numpy()
    check_decode(out, truth, nks, "decode vs oracle")
    o = torch.full((B, H, N, D), float("nan"), dtype=torch.half, device="cuda")
    capi.attn_fwd(q.cuda(), k.cuda(), v.cuda(), o, causal=True)
    torch.cuda.synchronize()
    check_decode(o.float().cpu().numpy(), truth, nks, "prefill vs oracle")


def test_one_model_sized_shape():
    """(4, 32 / 8, Nq 1, Ncap 8192, D 128), lengths {8192, 8191, 4097, 1}, auto split: all 128 rows against the oracle"""
    capi = _capi()
    B, H, Hkv, Nq, Ncap, D = 4, 32, 8, 1, 8192, 128
    lens = (8192, 8191, 4097, 1)
    q, k, v = decode_inputs(B, H, Hkv, Nq, Ncap, D, seed=8192)
    name = capi.attn_decode_kernel_name(B, H, Hkv, Nq, Ncap, D)
    assert name.startswith("attn_decode_kernel<128,1> x"), name      # 32 head groups do not fill the GPU: split
    truth, nks = decode_truth(_oracle(), q, k, v, lens, False)
    out = _run(capi, q, k, v, lens, False).float().cpu().numpy()
    worst = check_decode(out, truth, nks, name)
    print(f"[decode] {name}: worst |err| / bound {worst:.3f}")
