"""GPU tests of ragged-batch attention and rotary embedding + append over the paged caches (lc_attn_varlen_paged_f16 / _kv8,
lc_rope_append_varlen_f16 / _kv8).

1. A uniform ragged call (all Nq_b = max_nq) is the rectangular local / chunk / decode call on the same tokens, bit for bit, at equal S.
2. A sequence's bits do not depend on its neighbours: every sequence of a mixed batch equals the B = 1 ragged call on it alone; every row is
   within tol.attn_close(N = visible keys + 1) of the float64 reference.
3. window = 1: every row is its own key's V row, bit for bit — the position of every row of every block shape; and local_lib's pinned low edge
   on a sequence of 70 tokens, whose row blocks straddle head boundaries.
4. Rows nobody owns keep a sentinel, with one KV range and with three (the varlen combine kernel).
5. The clamps: cu_q with a negative entry, a decreasing pair, Nq_b > max_nq and an entry past T, on buffers with sentinel guard rows behind row T.
6. The ragged rope call against rope_append_paged (LC_ROPE_PACKED_SRC) called once per sequence: pools and Qout byte for byte.
7. One step [rope_append_varlen, attn_varlen_paged] captured once and replayed on three different ragged batches.

Inputs, truth and plan restatement: tests/varlen_lib.py on top of tests/local_lib.py and tests/decode_lib.py."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_lib as dl
from tests import local_lib as ll
from tests import varlen_lib as vl
from tests.decode_lib import _capi, _cuda

pytestmark = pytest.mark.gpu
NCAP = vl.NCAP
H, HKV = 8, 2
HEADS = torch.arange(H) // (H // HKV)


def bits(x):
    return x.view(torch.int16)


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


@functools.lru_cache(maxsize=None)
def cache(D, lens, seed=0):
    """ll.Cache of randn k, v [B,HKV,NCAP,D] (shared, never written to)"""
    _, k, v = dl.decode_inputs(len(lens), H, HKV, 1, NCAP, D, seed=11 * D + sum(lens) + seed)
    return ll.Cache(k, v, lens, ps=16, seed=D + len(lens))


@functools.lru_cache(maxsize=None)
def tokens(D, T, seed=0):
    return torch.randn(T, H, D, generator=torch.Generator().manual_seed(3 * D + T + seed)).half()


# ---- 1. a uniform ragged call is the rectangular call

@pytest.mark.parametrize("D", vl.DS)
@pytest.mark.parametrize("kind", vl.KINDS)
@pytest.mark.parametrize("Nq", (1, 5, 10, 20))                 # R = 4, 20, 40, 80: RT 1, 2, 4 and RB 2
def test_a_uniform_ragged_call_is_the_rectangular_call_bit_for_bit(D, kind, Nq):
    lens = (1000, 129, 65)
    B = len(lens)
    c = cache(D, lens)
    q = tokens(D, B * Nq)
    rect = vl.from_tokens(q, B, Nq)
    sinks = torch.randn(H, generator=torch.Generator().manual_seed(D + Nq))
    for window, sk in ((0, None), (33, None), (200, sinks), (0, sinks)):
        for split in (1, 3):
            got = vl.run(kind, c, q, vl.cu_of([Nq] * B), lens, Nq, window=window, sinks=sk, split=split)
            want = c.run(kind, rect, lens, True, window=window, sinks=sk, split=split)      # (window 0, no sinks: the chunk / decode call)
            assert torch.isfinite(want).all()
            assert same(vl.from_tokens(got, B, Nq), want), (window, sk is not None, split)


# ---- 2. neighbours

MIX_NQ = (1, 0, 37, 1, 130, 5)
MIX_LENS = (1000, 500, 129, 65, 577, 3)                        # (the last: more tokens than keys — two rows at negative positions)


@pytest.mark.parametrize("D", vl.DS)
@pytest.mark.parametrize("kind", vl.KINDS)
def test_a_sequences_bits_do_not_depend_on_its_neighbours(D, kind):
    c = cache(D, MIX_LENS)
    cu = vl.cu_of(MIX_NQ)
    T, max_nq = cu[-1], 130
    q = tokens(D, T)
    k64, v64 = c.logical(kind)
    sinks = torch.randn(H, generator=torch.Generator().manual_seed(D))
    for window, sk, split in ((0, None, 1), (0, None, 3), (100, sinks, 1), (100, sinks, 3)):
        got = vl.run(kind, c, q, cu, MIX_LENS, max_nq, window=window, sinks=sk, split=split)
        for b, n in enumerate(MIX_NQ):
            if n == 0:
                continue
            alone = vl.run(kind, c, q, cu[b:b + 2], MIX_LENS, max_nq, window=window, sinks=sk, split=split, seqs=[b])
            assert same(got[cu[b]:cu[b + 1]], alone[cu[b]:cu[b + 1]]), (b, window, split)
            rest = torch.cat([alone[:cu[b]], alone[cu[b + 1]:]])
            assert (rest == vl.SENTINEL).all(), (b, "the B = 1 call wrote a row of another sequence")
        truth, nvis = vl.ragged64(q, k64, v64, cu, MIX_LENS, max_nq, True, window=window, sinks=sk)
        assert (nvis >= 0).all() and (nvis == 0).sum() == 2
        vl.check_rows(got.float().cpu().numpy(), truth, nvis, extra=1, what=(kind, window, split))


# ---- 3. the position of every row

@pytest.mark.parametrize("D", vl.DS)
@pytest.mark.parametrize("kind", vl.KINDS)
def test_window_one_is_the_rows_own_value_row(D, kind):
    c = cache(D, MIX_LENS)
    cu = vl.cu_of(MIX_NQ)
    T = cu[-1]
    q = tokens(D, T)
    v = c.v if kind != "kv8" else dl.dequant(c.v8, dl.scales(dl.V_SCALES, HKV))      # powers of two: v_scale x code is exact in fp16
    want = torch.zeros(T, H, D, dtype=torch.half)
    for b, n in enumerate(MIX_NQ):
        for i in range(n):
            p = MIX_LENS[b] - n + i
            if p >= 0:
                want[cu[b] + i] = v[b, HEADS, p]
    want = want + 0.0                                           # (an e4m3 code of -0: the accumulator 0 + 1 x -0 is +0)
    for max_nq in (130, T):                                     # RB = 9 and RB = 11: the grid's RB is the host's, the rows are the sequence's
        for split in (1, 4):
            assert same(vl.run(kind, c, q, cu, MIX_LENS, max_nq, window=1, split=split), want), (max_nq, split)
    # RB = 1 kernels: sequences of at most 16 tokens
    nqs = (1, 16, 0, 7, 3, 2)
    cu2 = vl.cu_of(nqs)
    want2 = torch.zeros(cu2[-1], H, D, dtype=torch.half)
    for b, n in enumerate(nqs):
        for i in range(n):
            p = MIX_LENS[b] - n + i
            if p >= 0:
                want2[cu2[b] + i] = v[b, HEADS, p]
    want2 = want2 + 0.0
    for max_nq in (16, 8, 4):                                   # RT = 4, 2, 1 (a longer sequence is cut to its first max_nq tokens' worth of rows)
        got = vl.run(kind, c, q[:cu2[-1]], cu2, MIX_LENS, max_nq, window=1, split=1)
        for b, (q0, n) in enumerate(vl.owned(cu2, cu2[-1], max_nq)):
            if n == nqs[b]:
                assert same(got[q0:q0 + n], want2[q0:q0 + n]), (max_nq, b)


@pytest.mark.parametrize("D", vl.DS)
def test_the_low_edge_on_a_sequence_whose_blocks_straddle_heads(D):
    """local_lib.edge_inputs at Nq = 70 (R = 280: blocks start at rows 0, 64, 128, 192, 256 — tokens 0, 64, 58, 52, 46 of heads 0, 0, 1, 2, 3):
    the dominant key one below the window leaves the row alone, the one ON the edge is the row; sequence 1 holds the last 3 tokens of entry 1"""
    shape = (H, HKV, 70)
    for place in ("inside", "tile_straddle", "range_straddle", "clipped"):
        for below in (True, False):
            q, k, v, w, split = ll.edge_inputs(D, shape, place, below)
            c = ll.Cache(k, v, ll.EDGE_LENS, ps=16, seed=3, k_scales=dl.PIN_K_SCALES, v_scales=dl.PIN_V_SCALES)
            qt = torch.cat([q[0].permute(1, 0, 2), q[1, :, 67:].permute(1, 0, 2)]).contiguous()
            cu = [0, 70, 73]
            for kind in vl.KINDS:
                k64, v64 = c.logical(kind)
                truth, nvis = vl.ragged64(qt, k64, v64, cu, ll.EDGE_LENS, 70, True, window=w)
                out = vl.run(kind, c, qt, cu, ll.EDGE_LENS, 70, window=w, split=split).float().cpu().numpy()
                vl.check_rows(out, truth, nvis, what=(D, place, below, kind))


# ---- 4. rows nobody owns

@pytest.mark.parametrize("D", vl.DS)
@pytest.mark.parametrize("kind", vl.KINDS)
def test_rows_nobody_owns_are_not_written(D, kind):
    c = cache(D, MIX_LENS)
    nqs = (3, 0, 20, 1, 0, 2)
    cu = vl.cu_of(nqs)
    T = cu[-1] + 9
    q = tokens(D, T)
    for max_nq in (20, 8):                                      # RB = 2, and RB = 1 with sequence 2 cut to 8 tokens: rows 11 .. 22 are nobody's
        for split in (1, 3):
            got = vl.run(kind, c, q, cu, MIX_LENS, max_nq, split=split).cpu()
            assert (got[cu[-1]:] == vl.SENTINEL).all(), (max_nq, split)
            for q0, n in vl.owned(cu, T, max_nq):
                assert torch.isfinite(got[q0:q0 + n]).all() and (got[q0:q0 + n] != vl.SENTINEL).any(dim=-1).all(), (max_nq, split)
        if max_nq == 8:
            assert (vl.run(kind, c, q, cu, MIX_LENS, max_nq, split=1).cpu()[11:23] == vl.SENTINEL).all()
    # nobody owns anything
    for split in (1, 3):
        assert (vl.run(kind, c, q, [0] * 7, MIX_LENS, 20, split=split) == vl.SENTINEL).all()


# ---- 5. the clamps

CLAMP_CU = (-4, 5, 30, 28, 48, 900)
CLAMP_T, CLAMP_MAX, GUARD = 60, 20, 8


@pytest.mark.parametrize("D", vl.DS)
@pytest.mark.parametrize("kind", vl.KINDS)
def test_no_value_in_cu_q_leaves_the_T_rows(D, kind):
    """cu_q = (-4, 5, 30, 28, 48, 900) at T = 60, max_nq = 20: sequence 0 owns rows 0 .. 4 (a negative start), 1 rows 5 .. 24 (25 > max_nq),
    2 nothing (a decreasing pair), 3 rows 28 .. 47, 4 rows 48 .. 59 (an end past T).  Q and O have 8 sentinel rows behind row T."""
    lens = MIX_LENS[:5]
    c = cache(D, MIX_LENS)
    want_owned = [(0, 5), (5, 20), (30, 0), (28, 20), (48, 12)]
    assert vl.owned(CLAMP_CU, CLAMP_T, CLAMP_MAX) == want_owned
    qfull = tokens(D, CLAMP_T + GUARD).cuda()
    q = qfull[:CLAMP_T]
    for split in (1, 3):
        ofull = torch.full_like(qfull, vl.SENTINEL)
        vl.run(kind, c, q, CLAMP_CU, lens, CLAMP_MAX, split=split, o=ofull[:CLAMP_T], seqs=range(5))
        assert (ofull[CLAMP_T:] == vl.SENTINEL).all() and same(qfull[CLAMP_T:], tokens(D, CLAMP_T + GUARD)[CLAMP_T:]), split
        if split == 1:
            assert (ofull[25:28] == vl.SENTINEL).all()
        for b, (q0, n) in enumerate(want_owned):
            if n:
                alone = vl.run(kind, c, q, [q0, q0 + n], lens, CLAMP_MAX, split=split, seqs=[b])
                assert same(ofull[q0:q0 + n], alone[q0:q0 + n]), (b, split)


@pytest.mark.parametrize("kind", vl.KINDS)
def test_the_rope_call_under_a_hostile_cu_q_stays_inside_its_buffers(kind):
    capi = _capi()
    D = 64
    lens = MIX_LENS[:5]
    c = cache(D, MIX_LENS)
    T = CLAMP_T
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(T, (H + 2 * HKV) * D, generator=g).half().cuda()
    qfull = torch.full((T + GUARD, H, D), vl.SENTINEL, dtype=torch.half, device="cuda")
    P = c.kp.shape[0]
    if kind == "paged":
        pools = [torch.full((P + 2,) + tuple(c.kp.shape[1:]), vl.SENTINEL, dtype=torch.half, device="cuda") for _ in range(2)]
    else:
        pools = [torch.full((P + 2,) + tuple(c.kp8.shape[1:]), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
    table = (c.table if kind == "paged" else c.table8)[:5].contiguous().cuda()
    cs = capi.rope_table(NCAP, D).cuda()
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)
    fn = capi.rope_append_varlen if kind == "paged" else capi.rope_append_varlen_kv8
    fn(qv, kv, vv, pools[0][:P], pools[1][:P], cs, vl.dev_i32(CLAMP_CU), table, vl.dev_i32(lens), CLAMP_MAX, q_out=qfull[:T])
    torch.cuda.synchronize()
    assert (qfull[T:] == vl.SENTINEL).all()
    for pool in pools:
        assert (pool[P:] == (vl.SENTINEL if kind == "paged" else 0x5A)).all()
    assert (qfull[:5] != vl.SENTINEL).any()                    # sequence 0 was served


# ---- 6. the ragged rope call

ROPE_NQ = (3, 0, 10, 7, 40, 1)
ROPE_LENS = (1000, 500, 129, 5, 577, 65)                      # (sequence 3: 7 tokens on 5 keys — two rows at negative positions)


def rope_reference(capi, qkv, cu, lens, table, pools, cs, interleaved, scales):
    """rope_append_paged_qkv (LC_ROPE_PACKED_SRC) once per sequence, B = 1, on `pools`; returns Qout token-major (SENTINEL where nobody wrote)"""
    T = qkv.shape[0]
    D = pools[0].shape[-1]
    qout = torch.full((T, H, D), vl.SENTINEL, dtype=torch.half, device="cuda")
    for b in range(len(lens)):
        n = cu[b + 1] - cu[b]
        if n == 0:
            continue
        one = capi.rope_append_paged_qkv(qkv[cu[b]:cu[b + 1]].unsqueeze(0), H, HKV, pools[0], pools[1], cs, table[b:b + 1].contiguous(),
                                         vl.dev_i32(lens[b:b + 1]), interleaved=interleaved, **scales)
        qout[cu[b]:cu[b + 1]] = one[0].permute(1, 0, 2)
    torch.cuda.synchronize()
    return qout


@pytest.mark.parametrize("D", vl.DS)
@pytest.mark.parametrize("kind", vl.KINDS)
@pytest.mark.parametrize("interleaved", (False, True), ids=("neox", "gptj"))
def test_the_ragged_rope_call_is_the_rectangular_call_per_sequence(D, kind, interleaved):
    capi = _capi()
    c = cache(D, ROPE_LENS)
    cu = vl.cu_of(ROPE_NQ)
    T = cu[-1] + 3                                              # three tokens past cu_q[B]; D = 64: token block 0 straddles sequences 0, 2, 3, 4
    g = torch.Generator().manual_seed(D + int(interleaved))
    wide = torch.randn(T, (H + 2 * HKV) * D + 8, generator=g).half().cuda()
    qkv = wide[:, :(H + 2 * HKV) * D]                           # a row-strided view of a wider buffer: row stride (H + 2 Hkv) D + 8
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)
    table = (c.table if kind == "paged" else c.table8).cuda()
    kv8 = kind == "kv8"
    scales = {"k_scale": c.ks.cuda(), "v_scale": c.vs.cuda()} if kv8 else {}
    fn = capi.rope_append_varlen_kv8 if kv8 else capi.rope_append_varlen

    def fresh():
        src = (c.kp8, c.vp8) if kv8 else (c.kp, c.vp)
        return [torch.full(x.shape, 0x5A if kv8 else vl.SENTINEL, dtype=x.dtype, device="cuda") for x in src]

    for rot in (D, D // 2):
        cs = capi.rope_table(NCAP, rot).cuda()
        want_pools = fresh()
        want_q = rope_reference(capi, qkv, cu, ROPE_LENS, table, want_pools, cs, interleaved, scales)
        assert (want_q[cu[-1]:] == vl.SENTINEL).all() and (want_q[cu[3]:cu[3] + 2] == 0).all()
        # packed strides
        pools = fresh()
        got_q = fn(qv, kv, vv, pools[0], pools[1], cs, vl.dev_i32(cu), table, vl.dev_i32(ROPE_LENS), 40,
                   q_out=torch.full((T, H, D), vl.SENTINEL, dtype=torch.half, device="cuda"), interleaved=interleaved, **scales)
        torch.cuda.synchronize()
        assert same(got_q, want_q), ("packed", rot)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(pools, want_pools)), ("packed", rot)
        # dense sources, in place
        pools = fresh()
        qd, kd, vd = qv.contiguous(), kv.contiguous(), vv.contiguous()
        tail = qd[cu[-1]:].clone()
        assert fn(qd, kd, vd, pools[0], pools[1], cs, vl.dev_i32(cu), table, vl.dev_i32(ROPE_LENS), 40, q_out=qd, interleaved=interleaved,
                  **scales) is qd
        torch.cuda.synchronize()
        assert same(qd[:cu[-1]], want_q[:cu[-1]]) and same(qd[cu[-1]:], tail), ("in place", rot)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(pools, want_pools)), ("dense", rot)


# ---- 7. one step as a graph

def test_a_ragged_step_is_captured_once_and_replayed():
    """[rope_append_varlen, attn_varlen_paged with a window and sinks, split-KV on a caller workspace] captured as one chain; cu_q and kv_len are
    rewritten on the device between replays — three different ragged batches under one T and max_nq, one of them all-decode — and every replay
    equals the eager calls on the same state, bit for bit"""
    capi = _capi()
    D, ps, B, W, T, max_nq = 64, 16, 4, 128, 40, 24
    base = (500, 129, 65, 300)
    c = cache(D, (528, 151, 71, 317), seed=1)                  # the lengths after the three steps: every appended position lies in a page of its sequence
    gen = torch.Generator().manual_seed(77)
    sinks = torch.randn(H, generator=gen).cuda()
    cs = capi.rope_table(NCAP, D).cuda()
    tg, = _cuda(c.table)
    g_pools, e_pools = ([x.clone().cuda() for x in (c.kp, c.vp)] for _ in range(2))
    g_len, e_len = (torch.tensor(base, dtype=torch.int32, device="cuda") for _ in range(2))
    cu_dev = vl.dev_i32([0, 1, 2, 3, 4])
    qkv = torch.randn(T, (H + 2 * HKV) * D, generator=gen).half().cuda()
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)
    g_q, e_q, g_o, e_o = (torch.full((T, H, D), vl.SENTINEL, dtype=torch.half, device="cuda") for _ in range(4))
    capi.tune("attn_decode_split", 3)
    try:
        ws = torch.empty(capi.attn_varlen_paged_workspace_bytes(B, H, HKV, T, max_nq, ps, NCAP // ps, D, window=W), dtype=torch.uint8, device="cuda")
        assert ws.numel() == 3 * T * H * (D + 1) * 4

        def step(pools, lens_dev, out_q, out_o):
            capi.rope_append_varlen(qv, kv, vv, pools[0], pools[1], cs, cu_dev, tg, lens_dev, max_nq, q_out=out_q)
            capi.attn_varlen_paged(out_q, pools[0], pools[1], out_o, cu_dev, tg, lens_dev, max_nq, causal=True, window=W, sinks=sinks, workspace=ws)

        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            step([x.clone() for x in g_pools], g_len.clone(), torch.empty_like(g_q), torch.empty_like(g_o))      # warm-up on state of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                step(g_pools, g_len, g_q, g_o)
        torch.cuda.synchronize()
        assert (g_o == vl.SENTINEL).all()                                                     # captured, not run
        lens = list(base)
        for r, nqs in enumerate(((24, 1, 0, 15), (1, 1, 1, 1), (3, 20, 5, 1))):
            lens = [x + n for x, n in zip(lens, nqs)]                                         # kv_len is the length AFTER the step's append
            cu_dev.copy_(vl.dev_i32(vl.cu_of(nqs)))
            for x in (g_len, e_len):
                x.copy_(vl.dev_i32(lens))
            qkv.copy_(torch.randn(qkv.shape, generator=gen).half())
            for x in (g_q, e_q, g_o, e_o):
                x.fill_(vl.SENTINEL)
            g.replay()
            step(e_pools, e_len, e_q, e_o)
            torch.cuda.synchronize()
            n = sum(nqs)
            assert torch.isfinite(g_o[:n]).all() and (g_o[:n] != vl.SENTINEL).any(dim=-1).all() and (g_o[n:] == vl.SENTINEL).all(), r
            assert same(g_o, e_o) and same(g_q, e_q), r
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(g_pools, e_pools)), r
    finally:
        capi.tune("attn_decode_split", 0)
