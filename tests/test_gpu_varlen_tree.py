"""GPU tests of the tree-speculation entries: the look-back visibility mask on the ragged attention calls and the per-token rotary positions on
the ragged rope + append calls (lc_attn_varlen_paged_tree_*, lc_rope_append_varlen_pos_*).

1. All ones is the twin: O and lse equal the LSE entry's bit for bit, with one KV range and with three, with and without window and sinks;
   rows nobody owns keep their sentinels.
2. Every bit, alone: integer Q and K, window = 64, row t carries the single bit d — all d in 0 .. 63 — at RT = 1, 2, 4 and RB = 2, with one and
   two ranges: the row sees exactly key p - d, O is that V row bit for bit and lse its score within 4 fp32 ulp; p - d < 0: O = 0, lse = -inf.
3. The edge at 64: a zero word without a window sees exactly the keys j <= p - 64.  Q = 0, 2^k such keys, small-integer V: lse = k ln 2 within
   one ulp and O the exact mean; p < 64: nothing; with a sink: the sink alone.
4. Random trees of 1, 5, 16, 17 and 64 tokens next to a decoding sequence and a 70-token chunk, against the float64 reference built from the
   parent arrays, under the project's bounds; the visible keys of every row are asserted; the worst err / bound is printed.
5. pos_ids: the slots give the twin's bytes; the quarter-turn table is exact; random ids stay under rope_lib's bound; ids outside the table use
   rows 0 and max_pos - 1; dropped and unowned tokens write nothing.
6. Tree equals path: rope_append_varlen_pos + tree attention on a branching tree against the plain causal calls on caches that hold one
   root-to-leaf path each.
7. [rope_append_varlen_pos, tree attention] captured once and replayed after cu_q, kv_len, tree_mask and pos_ids changed in place.

Inputs, references and bounds: tests/tree_lib.py on top of tests/lse_lib.py, varlen_lib.py, bf16_lib.py, local_lib.py, rope_lib.py, decode_lib.py."""
import math

import numpy as np
import pytest
import torch

from tests import bf16_lib as bl
from tests import decode_lib as dl
from tests import local_lib as ll
from tests import lse_lib as sl
from tests import rope_lib as rl
from tests import tree_lib as tl
from tests import varlen_lib as vl
from tests.decode_lib import _capi, _cuda
from tests.lse_lib import H, HKV, LENS, MAX_NQ, NCAP, NQS, SINKS, T_RAGGED, cache, el_of, tokens

pytestmark = pytest.mark.gpu
CASES = [(D, bf16, kind) for D in sl.DS for bf16 in (False, True) for kind in sl.KINDS]
IDS = [f"{D}-{'bf16' if b else 'f16'}-{k}" for D, b, k in CASES]
G = H // HKV


def f64(x):
    return x.float().cpu().double().numpy()


# ---- 1. all ones is the twin

@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_all_ones_is_the_twin_bit_for_bit(D, bf16, kind):
    _capi()
    c, q, cu = cache(D, bf16, LENS), tokens(D, bf16, T_RAGGED), vl.cu_of(NQS)
    n = sum(NQS)
    ones = torch.full((T_RAGGED,), tl.ONES, dtype=torch.int64)
    for split in (1, 3):
        for window, sinks in ((0, None), (45, SINKS)):
            want_o, want_l = sl.run(kind, bf16, c, q, cu, LENS, MAX_NQ, causal=True, window=window, sinks=sinks, split=split)
            o, lse = tl.run(kind, bf16, c, q, cu, LENS, MAX_NQ, ones, window=window, sinks=sinks, split=split)
            assert bl.same(o, want_o) and torch.equal(lse.view(torch.int32), want_l.view(torch.int32)), (split, window)
            assert (o[n:] == sl.o_sentinel(o.dtype)).all() and (lse[n:] == sl.LSE_SENTINEL).all(), (split, window)
            assert torch.isfinite(lse[:n]).all(), (split, window)


# ---- 2. every bit, alone

@pytest.mark.parametrize("max_nq", (4, 8, 16, 20), ids=("rt1", "rt2", "rt4", "rb2"))
@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_every_bit_alone_shows_exactly_its_key(D, bf16, kind, max_nq):
    capi = _capi()
    B = 64 // max_nq + 2                                               # >= 64 + max_nq tokens: every d, and d = t mod 64 meets several row places
    nqs = (max_nq,) * (B - 1) + (max_nq // 2 + 1,)
    lens = tuple(64 + max_nq + (57 * b) % 900 for b in range(B - 2)) + (max_nq + 2, 3)      # (the last two: p - d < 0, and tokens in front of key 0)
    g = torch.Generator().manual_seed(3 * D + max_nq)
    k = torch.randint(-3, 4, (B, HKV, NCAP, D), generator=g).to(el_of(bf16))
    v = torch.randn(B, HKV, NCAP, D, generator=g).to(el_of(bf16))
    c = ll.Cache(k, v, lens, ps=16, seed=7)
    klog, vlog = c.logical(kind)
    assert torch.equal(klog, k.double())                               # (kv8: small integers over a power-of-two scale — the codes are exact)
    T = sum(nqs)
    q = torch.randint(-3, 4, (T, H, D), generator=g).to(el_of(bf16))
    cu = vl.cu_of(nqs)
    name = capi.attn_varlen_paged_tree_kernel_name(B, H, HKV, T, max_nq, 16, NCAP // 16, D, window=64, kv8=kind == "kv8", bf16=bf16)
    assert name.startswith("attn_varlen_chunk_") == (max_nq == 20) and (max_nq == 20 or f",{dl.rt_of(H, HKV, max_nq)}>" in name), name
    seq, pos = bl.token_positions(cu, lens, T, max_nq)
    heads = torch.arange(H) // G
    seen = set()
    for shift, split in ((0, 1), (37, 2)):
        d = (torch.arange(T) + shift) % 64
        seen |= set(d.tolist())
        mask = tl.words([1 << int(x) for x in d])
        o, lse = tl.run(kind, bf16, c, q, cu, lens, max_nq, mask, window=64, split=split)
        key = pos - d
        empty = key < 0
        assert 0 < int(empty.sum()) < T
        got_o, got_l = o.cpu(), f64(lse)
        assert (got_o[empty] == 0).all() and (got_l[empty.numpy()] == -np.inf).all(), split
        for t in torch.nonzero(~empty).flatten().tolist():
            b, j = int(seq[t]), int(key[t])
            assert torch.equal(got_o[t].double(), vlog[b, heads, j]), (split, t, int(d[t]))
            want = (klog[b, heads, j] * q[t].double()).sum(-1).numpy() / math.sqrt(D)
            assert (np.abs(got_l[t] - want) <= 4 * sl.ulp32(want)).all(), (split, t, int(d[t]))
    assert seen == set(range(64))


# ---- 3. the edge at 64

@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_the_edge_at_64(D, bf16, kind):
    _capi()
    ks = tuple(range(8))
    nq = 2                                                             # token 0 at p = 63 + 2^k sees the 2^k keys 0 .. p - 64; token 1 one more
    lens = tuple(63 + 2 ** k + nq for k in ks) + (50, 65)              # (p < 64: nothing; the last: token 0 at p = 63 nothing, token 1 key 0)
    B = len(lens)
    g = torch.Generator().manual_seed(D + 5)
    k = torch.randn(B, HKV, NCAP, D, generator=g).to(el_of(bf16))
    v = torch.randint(-4, 5, (B, HKV, NCAP, D), generator=g).to(el_of(bf16))
    c = ll.Cache(k, v, lens, ps=16, seed=9)
    _, vlog = c.logical(kind)
    assert torch.equal(vlog, v.double())
    q = torch.zeros(nq * B, H, D, dtype=el_of(bf16))
    cu = vl.cu_of([nq] * B)
    zero = torch.zeros(nq * B, dtype=torch.int64)
    rows = [nq * i for i in range(len(ks))]
    heads = torch.arange(H) // G
    ln2 = np.float32(math.log(2.0))
    for split in (1, 2):
        o, lse = tl.run(kind, bf16, c, q, cu, lens, nq, zero, split=split)
        got = f64(lse)
        want = np.array([np.float32(x) * ln2 for x in ks], np.float64)[:, None]
        assert (np.abs(got[rows] - want) <= sl.ulp32(want)).all(), (split, got[rows, 0])
        nv1 = np.array([2 ** x + 1 for x in ks], np.float64)[:, None]                         # token 1: 2^k + 1 keys, under the derived bound
        assert (np.abs(got[[r + 1 for r in rows]] - np.log(nv1)) <= sl.lse_bound(0.0, np.log(nv1), nv1, D)).all(), split
        nothing = [nq * len(ks), nq * len(ks) + 1, nq * len(ks) + 2]                          # L = 50: both tokens; L = 65: token 0
        assert (got[nothing] == -np.inf).all() and (o[nothing] == 0).all(), split
        assert (got[nothing[-1] + 1] == 0).all(), split                                        # one key: ln 1
        if split == 1:                                                                         # (one range: the sum, the count and the quotient are exact)
            for i, x in enumerate(ks):
                mean = vlog[i, heads, :2 ** x].mean(dim=1)
                assert torch.equal(o[rows[i]].cpu().double(), mean.to(el_of(bf16)).double()), x
        sinks = torch.tensor([1.5, -2.0, 0.0, 0.25, 3.0, -0.5, 0.75, 1.0])
        o, lse = tl.run(kind, bf16, c, q, cu, lens, nq, zero, sinks=sinks, split=split)
        got = f64(lse)
        alone = sinks.double().numpy()[None, :]
        # fl(fl(s log2 e) ln 2): two roundings of a product, under two ulp of s (s = 0: exactly 0)
        assert (np.abs(got[nothing] - alone) <= 2 * sl.ulp32(alone) * (alone != 0)).all() and (o[nothing] == 0).all(), split
        want = np.log(np.array([2.0 ** x for x in ks])[:, None] + np.exp(alone))
        nv = np.array([2 ** x for x in ks])[:, None]
        assert (np.abs(got[rows] - want) <= sl.lse_bound(0.0, want, nv, D, float(sinks.abs().max()))).all(), split


# ---- 4. random trees

TREE_SIZES = (1, 5, 16, 17, 64)
TREE_NQS = TREE_SIZES + (1, 70)                                        # ... one all-ones decoding sequence and one all-ones 70-token chunk
TREE_LENS = (333, 100, 16, 90, 700, 260, 70)                           # (16 on 16: a tree without a prefix; 70 on 70: a first chunk)
TREE_T = sum(TREE_NQS) + 3


def forest(seed):
    rng = np.random.default_rng(seed)
    return [tl.random_parents(n, rng, chain=0.6) for n in TREE_SIZES] + [None, None]


@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_random_trees_against_the_float64_reference(D, bf16, kind):
    capi = _capi()
    c, q, cu = cache(D, bf16, TREE_LENS, seed=11), tokens(D, bf16, TREE_T, seed=11), vl.cu_of(TREE_NQS)
    klog, vlog = c.logical(kind)
    parents = forest(D + int(bf16))
    assert max(len(tl.ancestors(parents[4], i)) for i in range(64)) > 4 and len({p for p in parents[4]}) < 60      # deep, and it branches
    mask = torch.cat([capi.tree_mask(parents, cu), torch.full((3,), 12345, dtype=torch.int64)])                      # (nobody's rows: any word)
    depth_pos = tl.brute_positions(parents, cu, TREE_LENS)
    worst_o = worst_l = 0.0
    for window, sinks, splits in ((0, None, (1, 3)), (10, SINKS, (3,))):                                             # (10: cuts into the trees)
        truth, want_l, A, nvis = tl.tree64(q, klog, vlog, cu, TREE_LENS, MAX_NQ, parents, window=window, sinks=sinks)
        assert (nvis[cu[-1]:] == -1).all() and nvis[:cu[-1]].min() >= 1
        if window == 0:      # the prefix, the ancestors and the token itself: its rotary position + 1
            assert nvis[:cu[-1]].tolist() == [p + 1 for p in depth_pos]
        else:
            assert (nvis[:cu[-1]] <= 10).all() and (nvis[cu[4] + 10:cu[5]] < 10).any()
        for split in splits:
            o, lse = tl.run(kind, bf16, c, q, cu, TREE_LENS, MAX_NQ, mask, window=window, sinks=sinks, split=split)
            assert (o[cu[-1]:] == sl.o_sentinel(o.dtype)).all() and (lse[cu[-1]:] == sl.LSE_SENTINEL).all()
            worst_o = max(worst_o, sl.check_o(bf16, f64(o), truth, nvis, extra=0 if sinks is None else 1, what=(window, split)))
            worst_l = max(worst_l, sl.check_lse(f64(lse), want_l, A, nvis, D, sink=float(SINKS.abs().max()) if sinks is not None else 0.0,
                                                what=(window, split)))
    print(f"tree, D = {D} {'bf16' if bf16 else 'f16'} {kind}: worst O err / bound {worst_o:.3f}, worst lse err / bound {worst_l:.4f}")


# ---- 5. pos_ids

ROPE_NQ = (3, 0, 10, 7, 40, 1)
ROPE_LENS = (1000, 500, 129, 5, 577, 65)                               # (sequence 3: 7 tokens on 5 keys — two rows at negative positions)
MAX_POS = 512


def rope_setup(D, bf16, kind, seed):
    el = el_of(bf16)
    c = cache(D, bf16, ROPE_LENS, seed=12)
    cu = vl.cu_of(ROPE_NQ)
    T = cu[-1] + 3                                                     # three tokens past cu_q[B]
    g = torch.Generator().manual_seed(seed)
    q, kn, vn = (torch.randn(T, h, D, generator=g).to(el) for h in (H, HKV, HKV))
    kv8 = kind == "kv8"
    table = c.table8 if kv8 else c.table
    scales = {"k_scale": c.ks.cuda(), "v_scale": c.vs.cuda()} if kv8 else {}
    src = (c.kp8, c.vp8) if kv8 else (c.kp, c.vp)
    sent = 0x5A if kv8 else sl.o_sentinel(el)

    def fresh():
        return [torch.full(x.shape, sent, dtype=x.dtype, device="cuda") for x in src]

    def qout():
        return torch.full((T, H, D), sl.o_sentinel(el), dtype=el, device="cuda")

    return dict(c=c, cu=cu, T=T, q=q.cuda(), kn=kn.cuda(), vn=vn.cuda(), q_cpu=q, kn_cpu=kn, kv8=kv8, table=table, scales=scales, fresh=fresh,
                qout=qout, sent=sent, el=el)


def rope_run(s, bf16, cs, pos_ids, interleaved=False):
    pools = s["fresh"]()
    out = tl.rope_call(s["kv8"], bf16, s["q"], s["kn"], s["vn"], pools, cs, s["cu"], pos_ids, s["table"].cuda(), ROPE_LENS, 40, s["qout"](),
                       interleaved=interleaved, scales=s["scales"])
    return out, pools


def same_bytes(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("interleaved", (False, True), ids=("neox", "gptj"))
@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_pos_ids(D, bf16, kind, interleaved):
    _capi()
    s = rope_setup(D, bf16, kind, seed=D + int(interleaved))
    T, cu, el = s["T"], s["cu"], s["el"]
    n = cu[-1]
    seq, slot = bl.token_positions(cu, ROPE_LENS, T, 40)
    owned = seq >= 0
    live = owned & (slot >= 0)
    assert int((owned & (slot < 0)).sum()) == 2 and int((~owned).sum()) == 3
    # the slots are the twin: Q and pool bytes (rows nobody owns hold any id: never read)
    cs = rl.random_table(D // 2, 1024).cuda()
    want_q, want_pools = rope_run(s, bf16, cs, None, interleaved)
    ids = torch.where(owned, slot, torch.full_like(slot, 7 << 20)).int().cuda()
    got_q, got_pools = rope_run(s, bf16, cs, ids, interleaved)
    assert bl.same(got_q, want_q) and same_bytes(got_pools, want_pools)
    # dropped and unowned tokens write nothing: Qout past cu_q[B], every pool row no live token names; a token in front of key 0: Q = 0
    assert (got_q[n:] == sl.o_sentinel(el)).all() and (got_q.cpu()[owned & (slot < 0)] == 0).all()
    wrote = bl.written_mask(got_pools[0].cpu(), s["table"], seq, slot)
    for pool in got_pools:
        assert (pool.cpu()[~wrote] == s["sent"]).all() and (pool.cpu()[wrote] != s["sent"]).any()
    # random ids: exact on the quarter-turn table, under the derived bound on the base-10000 table; the slot still decides where a row goes
    g = torch.Generator().manual_seed(3 * D + 1)
    pos = torch.randint(0, MAX_POS, (T,), generator=g)
    for name, table in (("quarter", rl.pinned_table(D, MAX_POS)), ("random", rl.random_table(D // 2, MAX_POS))):
        got_q, got_pools = rope_run(s, bf16, table.cuda(), pos.int().cuda(), interleaved)
        assert bl.written_mask(got_pools[0].cpu(), s["table"], seq, slot).equal(wrote) and (got_pools[0].cpu()[~wrote] == s["sent"]).all()
        assert same_bytes(got_pools[1:], want_pools[1:])                                       # V does not know the position
        qe, qerr = tl.rope_exact(s["q_cpu"], pos, table, interleaved)
        ke, kerr = tl.rope_exact(s["kn_cpu"], pos, table, interleaved)
        krows = bl.pool_rows(got_pools[0].cpu(), s["table"], seq, slot)                        # [T,Hkv,D]
        if name == "quarter":
            assert torch.equal(got_q.cpu()[live].double(), qe[live]), name
            if s["kv8"]:
                want_codes = dl.quantize(ke.to(el).permute(1, 0, 2).unsqueeze(0), s["c"].ks)[0].permute(1, 0, 2)
                assert torch.equal(rl.zero_codes(krows[live]), rl.zero_codes(want_codes[live])), name
            else:
                assert torch.equal(krows[live].double(), ke[live]), name
        else:
            assert not tl.rope_violations(bf16, got_q.cpu()[live], qe[live], qerr[live]).any(), name
            if not s["kv8"]:
                assert not tl.rope_violations(bf16, krows[live], ke[live], kerr[live]).any(), name
    # ids outside the table use rows 0 and max_pos - 1
    table = rl.random_table(D // 2, MAX_POS).cuda()
    wild = pos.clone()
    wild[::3] = -1 - wild[::3]
    wild[1::3] = MAX_POS + 1000 * wild[1::3]
    got = rope_run(s, bf16, table, wild.int().cuda(), interleaved)
    want = rope_run(s, bf16, table, wild.clamp(0, MAX_POS - 1).int().cuda(), interleaved)
    assert bl.same(got[0], want[0]) and same_bytes(got[1], want[1])
    assert not bl.same(got[0], got_q)                                                          # (and they differ from the unclamped ids' rows)


# ---- 6. tree equals path

PATH_PARENTS = [-1, 0, 0, 1, 1, 2, 5, 5, 3]                            # leaves 4, 6, 7, 8
PREFIX = 40


@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_a_tree_equals_its_root_to_leaf_paths(D, bf16, kind):
    capi = _capi()
    el, kv8 = el_of(bf16), kind == "kv8"
    n = len(PATH_PARENTS)
    leaves = [i for i in range(n) if i not in PATH_PARENTS]
    paths = [sorted(tl.ancestors(PATH_PARENTS, i)) for i in leaves]
    assert leaves == [4, 6, 7, 8] and paths[1] == [0, 2, 5, 6]
    ps, mp = 16, 4
    nseq = 1 + len(leaves)
    g = torch.Generator().manual_seed(17 * D + int(bf16))
    table = torch.randperm(nseq * mp, generator=g).int().view(nseq, mp)
    ks_, vs_ = dl.scales(dl.K_SCALES, HKV), dl.scales(dl.V_SCALES, HKV)
    pk, pv = (torch.randn(1, HKV, PREFIX, D, generator=g).to(el) for _ in range(2))
    if kv8:
        pk, pv = dl.quantize(pk, ks_), dl.quantize(pv, vs_)
    pools = [torch.zeros(nseq * mp, HKV, ps, D, dtype=torch.uint8 if kv8 else el) for _ in range(2)]
    for b in range(nseq):                                               # the same prefix in every cache
        for j in range(PREFIX):
            for pool, src in zip(pools, (pk, pv)):
                pool[int(table[b, j // ps]), :, j % ps] = src[0, :, j]
    pools = [x.cuda() for x in pools]
    q, kn, vn = (torch.randn(n, h, D, generator=g).to(el).cuda() for h in (H, HKV, HKV))
    cs = capi.rope_table(256, D).cuda()
    scales = {"k_scale": ks_.cuda(), "v_scale": vs_.cuda()} if kv8 else {}
    # the tree: one sequence, PREFIX + n keys
    cu_t, len_t = [0, n], [PREFIX + n]
    mask = capi.tree_mask([PATH_PARENTS], cu_t)
    ids = capi.tree_positions([PATH_PARENTS], cu_t, len_t)
    assert ids.tolist() == [PREFIX + len(tl.ancestors(PATH_PARENTS, i)) - 1 for i in range(n)]
    qt = tl.rope_call(kv8, bf16, q, kn, vn, pools, cs, cu_t, ids.cuda(), table[:1].contiguous().cuda(), len_t, n,
                      torch.empty(n, H, D, dtype=el, device="cuda"), scales=scales)
    o_t = torch.empty_like(qt)
    fn = tl.fn_of(kind, bf16)
    _, lse_t = fn(qt, pools[0], pools[1], o_t, vl.dev_i32(cu_t), table[:1].contiguous().cuda(), vl.dev_i32(len_t), n, mask.cuda(), **scales)
    # the paths: one sequence per leaf on a cache of its own, the plain rope call (slot = position) and the plain causal call
    idx = [i for p in paths for i in p]
    cu_p, len_p = vl.cu_of([len(p) for p in paths]), [PREFIX + len(p) for p in paths]
    mq = max(len(p) for p in paths)
    tab_p = table[1:].contiguous().cuda()
    qp = tl.rope_call(kv8, bf16, q[idx].contiguous(), kn[idx].contiguous(), vn[idx].contiguous(), pools, cs, cu_p, None, tab_p, len_p, mq,
                      torch.empty(len(idx), H, D, dtype=el, device="cuda"), scales=scales)
    o_p = torch.empty_like(qp)
    lse_fn = {("paged", False): capi.attn_varlen_paged_lse, ("paged", True): capi.attn_varlen_paged_lse_bf16,
              ("kv8", False): capi.attn_varlen_paged_kv8_lse, ("kv8", True): capi.attn_varlen_paged_kv8_lse_bf16}[(kind, bf16)]
    _, lse_p = lse_fn(qp, pools[0], pools[1], o_p, vl.dev_i32(cu_p), tab_p, vl.dev_i32(len_p), mq, causal=True, **scales)
    torch.cuda.synchronize()
    # the rotated Q rows and the pool rows of a token are the same bits on its path's cache and on the tree's
    assert bl.same(qp, qt[idx])
    host = [x.cpu() for x in pools]
    seq_t, slot_t = bl.token_positions(cu_t, len_t, n, n)
    seq_p, slot_p = bl.token_positions(cu_p, len_p, len(idx), mq)
    for pool in host:
        assert bl.same(bl.pool_rows(pool, table[1:], seq_p, slot_p), bl.pool_rows(pool, table[:1], seq_t, slot_t)[idx])
    # the float64 attention of every path row over what its cache holds; the tree's leaf rows against the SAME truth
    def logical(pool, scale):
        rows = torch.stack([torch.cat([pool[int(table[b, j])] for j in range(mp)], dim=1) for b in range(1, nseq)])      # [leaves,Hkv,64,D]
        return dl.dequant64(rows, scale) if kv8 else rows.double()
    k64, v64 = logical(host[0], ks_), logical(host[1], vs_)
    truth, want_l, A, nvis = tl.tree64(qp.cpu(), k64, v64, cu_p, len_p, mq, [None] * len(paths))
    assert nvis.tolist() == [PREFIX + 1 + i for p in paths for i in range(len(p))]
    r1 = sl.check_o(bf16, f64(o_p), truth, nvis, what="paths")
    r2 = sl.check_lse(f64(lse_p), want_l, A, nvis, D, what="paths lse")
    last = [cu_p[i + 1] - 1 for i in range(len(paths))]                 # the leaf's row of every path
    nv_t = np.full((n,), -1, np.int64)
    truth_t, want_lt, A_t = np.zeros((n, H, D)), np.zeros((n, H)), np.zeros((n, H))
    for leaf, row in zip(leaves, last):
        nv_t[leaf], truth_t[leaf], want_lt[leaf], A_t[leaf] = nvis[row], truth[row], want_l[row], A[row]
    r3 = sl.check_o(bf16, f64(o_t), truth_t, nv_t, what="tree leaves")
    r4 = sl.check_lse(f64(lse_t), want_lt, A_t, nv_t, D, what="tree leaves lse")
    print(f"tree = path, D = {D} {'bf16' if bf16 else 'f16'} {kind}: paths O {r1:.3f} lse {r2:.4f}, tree leaves O {r3:.3f} lse {r4:.4f} of the bound")


# ---- 7. one verification step as a graph

@pytest.mark.parametrize("bf16", (False, True), ids=("f16", "bf16"))
def test_a_verification_step_is_captured_once_and_replayed(bf16):
    """[rope_append_varlen_pos, tree attention] captured as one chain on one stream (one KV range: no workspace); cu_q, kv_len, tree_mask and
    pos_ids are rewritten on the device between replays — trees of other shapes and sizes, a step without any tree — and every replay equals
    the eager calls on the same state, bit for bit"""
    capi = _capi()
    D, T, max_nq, B = 128, 48, 32, 3
    el = el_of(bf16)
    c = cache(D, bf16, (400, 160, 90), seed=13)
    tg, = _cuda(c.table)
    g_pools, e_pools = ([x.clone().cuda() for x in (c.kp, c.vp)] for _ in range(2))
    gen = torch.Generator().manual_seed(23)
    cs = capi.rope_table(NCAP, D).cuda()
    q, kn, vn = (torch.randn(T, h, D, generator=gen).to(el).cuda() for h in (H, HKV, HKV))
    cu_dev, len_dev = vl.dev_i32([0, 1, 2, 3]), vl.dev_i32([300, 100, 50])
    mask_dev = torch.full((T,), tl.ONES, dtype=torch.int64, device="cuda")
    pos_dev = torch.zeros(T, dtype=torch.int32, device="cuda")
    g_q, e_q, g_o, e_o = (torch.full((T, H, D), sl.o_sentinel(el), dtype=el, device="cuda") for _ in range(4))
    g_l, e_l = (torch.full((T, H), sl.LSE_SENTINEL, device="cuda") for _ in range(2))
    rope, attn = tl.rope_fn(False, bf16, True), tl.fn_of("paged", bf16)
    capi.tune("attn_decode_split", 1)
    try:
        sinks_dev = SINKS.cuda()                                        # (allocated before the capture)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()

        def step_g(pools, out_q, out_o, out_l):
            rope(q, kn, vn, pools[0], pools[1], cs, cu_dev, pos_dev, tg, len_dev, max_nq, q_out=out_q)
            attn(out_q, pools[0], pools[1], out_o, cu_dev, tg, len_dev, max_nq, mask_dev, lse=out_l, window=200, sinks=sinks_dev)

        with torch.cuda.stream(st):
            step_g([x.clone() for x in g_pools], torch.empty_like(g_q), torch.empty_like(g_o), torch.empty_like(g_l))      # warm-up on state of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step_g(g_pools, g_q, g_o, g_l)
        torch.cuda.synchronize()
        assert (g_o == sl.o_sentinel(el)).all()                         # captured, not run
        rng = np.random.default_rng(4)
        lens = [300, 100, 50]
        for r, sizes in enumerate(((32, 1, 9), (1, 1, 1), (5, 17, 26))):
            parents = [None if s == 1 else tl.random_parents(s, rng, chain=0.5) for s in sizes]
            lens = [x + s for x, s in zip(lens, sizes)]                 # kv_len is the length AFTER the step's append
            cu = vl.cu_of(sizes)
            n = cu[-1]
            cu_dev.copy_(vl.dev_i32(cu))
            len_dev.copy_(vl.dev_i32(lens))
            mask_dev[:n].copy_(capi.tree_mask(parents, cu))
            pos_dev[:n].copy_(capi.tree_positions(parents, cu, lens))
            for x in (q, kn, vn):
                x.copy_(torch.randn(x.shape, generator=gen).to(el))
            for x in (g_q, e_q, g_o, e_o):
                x.fill_(sl.o_sentinel(el))
            for x in (g_l, e_l):
                x.fill_(sl.LSE_SENTINEL)
            graph.replay()
            step_g(e_pools, e_q, e_o, e_l)
            torch.cuda.synchronize()
            assert torch.isfinite(g_o[:n].float()).all() and (g_o[n:] == sl.o_sentinel(el)).all() and (g_l[n:] == sl.LSE_SENTINEL).all(), r
            assert torch.isfinite(g_l[:n]).all(), r
            assert bl.same(g_o, e_o) and bl.same(g_q, e_q) and torch.equal(g_l, e_l), r
            assert all(bl.same(a, b) for a, b in zip(g_pools, e_pools)), r
    finally:
        capi.tune("attn_decode_split", 0)
