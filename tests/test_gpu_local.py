"""GPU tests of sliding-window / attention-sink attention (lc_attn_local_f16 / _paged_f16 / _paged_kv8).

1. window = 0 without sinks is the chunk call, bit for bit.
2. A window whose low edge lies on a tile seam is, bit for bit, the decode call on the cache rows [L - W, L) with kv_len = W at equal S: this
   pins the start tile, the partition of the walked tiles into ranges and the low mask together.
3. window = 1: every row is its own key's V row, bit for bit.
4. The low edge on every row, with decode_lib's pinned construction: the dominant key one below the window leaves the row alone, the dominant
   key ON the edge is the row.
5. Random inputs against the float64 reference (tests/local_lib.py local64), per-row bound tol.attn_close(N = visible keys + 1).
6. Sink pins: half of V, -inf, a sink that outweighs everything, the head a sink belongs to, a range that holds the sink and no key.
7. Nothing below the start tile is read: NaN rows and out-of-range table entries there change no bit.
8. One decode step [rope_append_paged, attn_local_paged] captured once and replayed.

Inputs, truth and plan restatement: tests/local_lib.py on top of tests/decode_lib.py."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_lib as dl
from tests import local_lib as ll
from tests.decode_lib import _capi, _cuda, _dev_lens, forced_split

pytestmark = pytest.mark.gpu
NCAP = ll.NCAP


def bits(x):
    return x.view(torch.int16)


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


@functools.lru_cache(maxsize=None)
def grid(D, shape, lens, seed=0):
    """(q, Cache): randn inputs at NCAP = 1024 held the three ways (shared, never written to)"""
    H, Hkv, Nq = shape
    q, k, v = dl.decode_inputs(len(lens), H, Hkv, Nq, NCAP, D, seed=7 * D + 131 * H + 17 * Nq + sum(lens) + seed)
    return q, ll.Cache(k, v, lens, ps=16, seed=Nq + D)


def chunk_call(capi, kind, q, c, lens, causal, split):
    qg, = _cuda(q)
    o = torch.full_like(qg, float("nan"))
    L = _dev_lens(lens)
    if kind == "flat":
        k, v = _cuda(c.k, c.v)
        forced_split(split, lambda: capi.attn_chunk(qg, k, v, o, L, causal=causal))
    elif kind == "paged":
        kp, vp, t = _cuda(c.kp, c.vp, c.table)
        forced_split(split, lambda: capi.attn_chunk_paged(qg, kp, vp, o, t, L, causal=causal))
    else:
        kp, vp, t, ks, vs = _cuda(c.kp8, c.vp8, c.table8, c.ks, c.vs)
        forced_split(split, lambda: capi.attn_chunk_paged_kv8(qg, kp, vp, o, t, L, ks, vs, causal=causal))
    torch.cuda.synchronize()
    return o


# ---- 1. identity with the chunk call

@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("kind", ll.KINDS)
def test_no_window_and_no_sinks_is_the_chunk_call_bit_for_bit(D, kind):
    capi = _capi()
    lens = (1000, 129, 65)
    for shape in ((8, 2, 5), (4, 2, 40)):                      # R = 20 (decode-shaped) and R = 80 (row blocks)
        q, c = grid(D, shape, lens)
        for causal in (False, True):
            for split in (0, 3):
                assert same(c.run(kind, q, lens, causal, split=split), chunk_call(capi, kind, q, c, lens, causal, split)), (shape, causal, split)


# ---- 2. bit-identity on a cache slice

@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("H", (8, 24, 40))                     # Hkv = 1, Nq = 1: RT = 1, 2, 4
def test_a_tile_aligned_window_is_the_decode_call_on_the_cache_slice(D, H):
    capi = _capi()
    # (L, W): L - W = 640 and 512 (a multiple of 128) of 1000; 320 and 64 of 577 — multiples of both page sizes
    for L, W in ((1000, 360), (1000, 488), (577, 257), (577, 513)):
        lens = (L, L)
        q, c = grid(D, (H, 1, 1), lens, seed=L)
        lo = L - W
        assert lo % 64 == 0 and ll.tile_lo(L, 1, NCAP, W) == lo // 64
        wl = (W, W)
        ks, vs = c.k[:, :, lo:L].contiguous(), c.v[:, :, lo:L].contiguous()
        pools = {ps: (dl.paginate(c.k, c.v, lens, ps, seed=ps + H), dl.paginate(c.k8, c.v8, lens, ps, seed=ps + H + 1, fill=dl.NAN_BYTE))
                 for ps in (16, 64)}
        for split in (1, 3, 8):
            want = dl.run_flat(capi, q, ks, vs, wl, True, split=split)
            assert torch.isfinite(want).all()
            assert same(c.run("flat", q, lens, True, window=W, split=split), want), (L, W, split)
            for ps, ((kp, vp, table), (kp8, vp8, table8)) in pools.items():
                want_p = dl.run_paged(capi, q, kp, vp, table[:, lo // ps:].contiguous(), wl, True, split=split)
                assert same(ll.run_paged(q, kp, vp, table, lens, True, window=W, split=split), want_p), (L, W, split, ps)
                want_8 = dl.run_kv8(capi, q, kp8, vp8, table8[:, lo // ps:].contiguous(), wl, c.ks, c.vs, True, split=split)
                assert same(ll.run_kv8(q, kp8, vp8, table8, lens, c.ks, c.vs, True, window=W, split=split), want_8), (L, W, split, ps)


# ---- 3. window = 1

@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("shape", ((8, 2, 1), (8, 2, 5), (2, 2, 17), (4, 2, 40)), ids=lambda s: "x".join(map(str, s)))
def test_window_one_is_the_rows_own_value_row(D, shape):
    H, Hkv, Nq = shape
    lens = (1000, 129, 65, Nq - 1 if Nq > 1 else 0, 1)         # (a left-padded entry with kv_len < Nq; one with a single key)
    q, c = grid(D, shape, lens)
    vs2 = dl.scales(dl.V_SCALES, Hkv)                           # powers of two: v_scale x code is exact in fp16
    for kind in ll.KINDS:
        v = c.v if kind != "kv8" else dl.dequant(c.v8, vs2)
        want = torch.zeros(len(lens), H, Nq, D, dtype=torch.half)
        for b, L in enumerate(lens):
            for i in range(Nq):
                p = L - Nq + i
                if p >= 0:
                    want[b, :, i] = v[b, torch.arange(H) // (H // Hkv), p]
        want = want + 0.0                                       # (an e4m3 code of -0: the accumulator 0 + 1 x -0 is +0)
        for split in (0, 1, 4):
            assert same(c.run(kind, q, lens, True, window=1, split=split), want), (kind, split)


# ---- 4. the low edge, every row

EDGE_SHAPES = dl.ROW_SHAPES + ((2, 1, 48),)                     # R = 96: block 1 starts at token 16 of head 1 (i_min = 16, no straddle)


@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_low_edge_on_every_row(D, shape):
    """below: the dominant key is p - W, the first key under the window, with a V row of +-8 — the row stays within the bound of the truth
    without it (a kernel that lets it in is off by ~8).  on: the dominant key is p - W + 1 — the row is that key's V row within the bound."""
    H, Hkv, Nq = shape
    for place in ll.EDGE_PLACES:
        for below in (True, False):
            q, k, v, w, split = ll.edge_inputs(D, shape, place, below)
            c = ll.Cache(k, v, ll.EDGE_LENS, ps=16, seed=3, k_scales=dl.PIN_K_SCALES, v_scales=dl.PIN_V_SCALES)
            assert torch.equal(dl.dequant(c.k8, c.ks), k)                                    # +-1 is exact in e4m3: the dominant score stays
            for kind in ll.KINDS:
                k64, v64 = c.logical(kind)
                truth, nvis = ll.local64(q, k64, v64, ll.EDGE_LENS, True, window=w)
                assert (nvis == min(w, 1000)).any()
                if not below:                                                                # the truth IS the edge key's V row, to ~3 W e^-12 |V|
                    lo = ll.span(ll.EDGE_LENS[0], Nq, NCAP, True, w, Nq - 1)[0]
                    assert np.abs(truth[0, 0, Nq - 1] - v64[0, 0, lo].numpy()).max() < 0.25
                out = c.run(kind, q, ll.EDGE_LENS, True, window=w, split=split).float().cpu().numpy()
                ll.check_rows(out, truth, nvis, what=(D, shape, place, below, kind))


# ---- 5. random inputs against the float64 reference

RANDOM_LENS = (1000, 129, 65, 5, 0)


@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("kind", ll.KINDS)
@pytest.mark.parametrize("shape", ((8, 2, 5), (4, 2, 40)), ids=lambda s: "x".join(map(str, s)))
def test_random_inputs_against_the_float64_reference(D, kind, shape):
    H = shape[0]
    q, c = grid(D, shape, RANDOM_LENS)
    k64, v64 = c.logical(kind)
    g = torch.Generator().manual_seed(D + H)
    for sinks in (None, torch.randn(H, generator=g), torch.full((H,), -float("inf"))):
        for w in (1, 33, 64, 200, 4096):
            truth, nvis = ll.local64(q, k64, v64, RANDOM_LENS, True, window=w, sinks=sinks)
            for split in (0, 4):
                out = c.run(kind, q, RANDOM_LENS, True, window=w, sinks=sinks, split=split).float().cpu().numpy()
                ll.check_rows(out, truth, nvis, extra=1, what=(kind, shape, w, split, sinks is not None))
        if sinks is not None:                                                                 # sinks without a window, causal or not
            for causal in (False, True):
                truth, nvis = ll.local64(q, k64, v64, RANDOM_LENS, causal, sinks=sinks)
                out = c.run(kind, q, RANDOM_LENS, causal, sinks=sinks, split=4).float().cpu().numpy()
                ll.check_rows(out, truth, nvis, extra=1, what=(kind, shape, "no window", causal))


# ---- 6. sink pins

@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("kind", ll.KINDS)
def test_sink_pins(D, kind):
    shape = (8, 2, 5)                                           # G = 4, Nq = 5: r / Nq, r % Nq and kvh G all differ
    H, Hkv, Nq = shape
    lens = (1000, 129, 65)
    q, c = grid(D, shape, lens)
    G = H // Hkv
    heads = torch.arange(H) // G
    v = c.v if kind != "kv8" else dl.dequant(c.v8, c.vs)
    # K = 0, window = 1, a sink of 0: two equal terms in the denominator — half the row's own V row, bit for bit
    zk = ll.Cache(torch.zeros_like(c.k), c.v, lens, ps=16, seed=9)
    half = torch.zeros(len(lens), H, Nq, D, dtype=torch.half)
    for b, L in enumerate(lens):
        for i in range(Nq):
            half[b, :, i] = (v[b, heads, L - Nq + i].float() / 2).half() + 0.0      # (+ 0: an e4m3 code of -0 accumulates to +0)
    for split in (1, 8):
        assert same(zk.run(kind, q, lens, True, window=1, sinks=torch.zeros(H), split=split), half), split
        # a sink of 80 outweighs the one key of score 0 by e^80
        big = zk.run(kind, q, lens, True, window=1, sinks=torch.full((H,), 80.0), split=split).float().cpu()
        assert big.abs().max().item() <= 2.0 ** -20 * v.float().abs().max().item()
    # -inf is no sink, bit for bit
    for w, split in ((0, 1), (33, 1), (200, 4), (0, 8)):
        none = c.run(kind, q, lens, True, window=w, split=split)
        assert same(c.run(kind, q, lens, True, window=w, sinks=torch.full((H,), -float("inf")), split=split), none), (w, split)
        assert torch.isfinite(none).all()
    # the head a sink belongs to: swapping ONE head's value moves that head's rows and no other bit
    g = torch.Generator().manual_seed(D)
    sinks = torch.randn(H, generator=g) + 2.0
    for split in (1, 4):
        base = c.run(kind, q, lens, True, window=64, sinks=sinks, split=split).cpu()
        for h in (0, 3, 5, 7):
            other = sinks.clone()
            other[h] += 3.0
            moved = c.run(kind, q, lens, True, window=64, sinks=other, split=split).cpu()
            rest = [x for x in range(H) if x != h]
            assert torch.equal(bits(moved[:, rest]), bits(base[:, rest])), (h, split)
            assert (moved[:, h].float() - base[:, h].float()).abs().amax(dim=-1).min().item() > 0, (h, split)      # every row of the head
    # forced split 8 at L = 65 (two tiles): range 0 holds the sink and, like most ranges, no key
    short = (65, 65, 64)
    truth, nvis = ll.local64(q, *c.logical(kind), short, True, sinks=sinks)
    out = c.run(kind, q, short, True, sinks=sinks, split=8).float().cpu().numpy()
    ll.check_rows(out, truth, nvis, extra=1, what="split 8 at L = 65")
    truth, nvis = ll.local64(q, *c.logical(kind), (3, 0, 1), True, sinks=sinks)              # rows with a sink and no visible key: exactly 0
    out = c.run(kind, q, (3, 0, 1), True, sinks=sinks, split=8).float().cpu().numpy()
    assert (nvis == 0).any()
    ll.check_rows(out, truth, nvis, extra=1, what="sink and no key")


# ---- 7. unread cache

@pytest.mark.parametrize("D", ll.DS)
@pytest.mark.parametrize("shape", ((8, 1, 1), (8, 2, 5), (2, 1, 48)), ids=lambda s: "x".join(map(str, s)))
def test_nothing_below_the_start_tile_is_read(D, shape):
    H, Hkv, Nq = shape
    L, W, ps = 1000, 64, 16
    lens = (L, L)
    q, c = grid(D, shape, lens)
    low = 64 * ll.tile_lo(L, Nq, NCAP, W)                      # (a row block that starts mid-head begins later still)
    assert low == 64 * ((L - Nq + 1 - W) // 64) and low >= 832
    for kind in ll.KINDS:
        for split in (1, 3):
            want = c.run(kind, q, lens, True, window=W, split=split)
            if kind == "flat":
                k, v = c.k.clone(), c.v.clone()
                k[:, :, :low] = float("nan")
                v[:, :, :low] = float("nan")
                got = ll.run_flat(q, k, v, lens, True, window=W, split=split)
            else:
                kp, vp, table = (x.clone() for x in ((c.kp, c.vp, c.table) if kind == "paged" else (c.kp8, c.vp8, c.table8)))
                for b in range(len(lens)):
                    for p in range(low // ps):
                        kp[int(table[b, p])] = float("nan") if kind == "paged" else dl.NAN_BYTE
                        vp[int(table[b, p])] = float("nan") if kind == "paged" else dl.NAN_BYTE
                        table[b, p] = (-7, 1 << 30, kp.shape[0])[p % 3]
                got = (ll.run_paged(q, kp, vp, table, lens, True, window=W, split=split) if kind == "paged" else
                       ll.run_kv8(q, kp, vp, table, lens, c.ks, c.vs, True, window=W, split=split))
            assert torch.isfinite(want).all() and same(got, want), (kind, split)


# ---- 8. graph capture

def test_a_windowed_decode_step_is_captured_once_and_replayed():
    """[kv_len += 1 on the device, rope_append_paged, attn_local_paged with a window and sinks, split-KV on a caller workspace] captured as one
    chain and replayed three times: O equals the eager calls on the same state each time, bit for bit"""
    capi = _capi()
    D, ps, B, H, Hkv, W = 64, 16, 3, 8, 1, 128
    lens = (500, 129, 65)                                       # (the three appended positions of every entry lie in a page of its own)
    _, c = grid(D, (H, Hkv, 1), lens)
    gen = torch.Generator().manual_seed(77)
    sinks = torch.randn(H, generator=gen).cuda()
    cs = capi.rope_table(NCAP, D).cuda()
    tg, = _cuda(c.table)
    g_pools, e_pools = ([x.clone().cuda() for x in (c.kp, c.vp)] for _ in range(2))
    g_len, e_len = (torch.tensor(lens, dtype=torch.int32, device="cuda") for _ in range(2))
    q = torch.randn(B, H, 1, D, generator=gen).half().cuda()
    kn, vn = (torch.randn(B, Hkv, 1, D, generator=gen).half().cuda() for _ in range(2))
    g_o, e_o = (torch.full_like(q, float("nan")) for _ in range(2))
    g_q, e_q = torch.empty_like(q), torch.empty_like(q)
    capi.tune("attn_decode_split", 4)
    try:
        ws = torch.empty(capi.attn_local_paged_workspace_bytes(B, H, Hkv, 1, ps, NCAP // ps, D, window=W), dtype=torch.uint8, device="cuda")
        assert ws.numel() > 0

        def step(pools, lens_dev, out_q, out_o):
            lens_dev.add_(1)
            capi.rope_append_paged(q, kn, vn, pools[0], pools[1], cs, tg, lens_dev, q_out=out_q)
            capi.attn_local_paged(out_q, pools[0], pools[1], out_o, tg, lens_dev, causal=True, window=W, sinks=sinks, workspace=ws)

        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            step([x.clone() for x in g_pools], g_len.clone(), torch.empty_like(q), torch.empty_like(q))      # warm-up on state of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                step(g_pools, g_len, g_q, g_o)
        torch.cuda.synchronize()
        assert torch.isnan(g_o).all() and [int(x) for x in g_len.cpu()] == list(lens)        # captured, not run
        for r in range(3):
            for x in (q, kn, vn):
                x.copy_(torch.randn(x.shape, generator=gen).half())
            if r == 1:
                sinks.copy_(torch.randn(H, generator=gen))                                    # read by the kernel at replay time
            g.replay()
            step(e_pools, e_len, e_q, e_o)
            torch.cuda.synchronize()
            assert torch.equal(g_len.cpu(), e_len.cpu()) and [int(x) for x in g_len.cpu()] == [x + r + 1 for x in lens]
            assert torch.isfinite(g_o).all() and same(g_o, e_o) and same(g_q, e_q), r
    finally:
        capi.tune("attn_decode_split", 0)
