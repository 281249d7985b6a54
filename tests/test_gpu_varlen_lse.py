"""GPU tests of the log-sum-exp ragged entries, the state merge and the shared-prefix (cascade) step built from them
(lc_attn_varlen_paged_lse_*, lc_attn_merge_states_*, capi.attn_cascade_paged).

1. O is the twin's: the LSE entry's O equals the non-LSE entry's, bit for bit, with one KV range and with three; nobody's rows keep their sentinels.
2. Q = 0 with 2^k visible keys: lse = k ln 2 within one fp32 ulp with 1, 2 and 4 ranges; with a sink ln(2^k + e^s); no key, no sink: -inf, O = 0.
3. One visible key (causal, window = 1), exact dot products: lse = q.k / sqrt(D) (x k_scale) within 4 fp32 ulp at RT = 1, 2, 4 and RB = 2.
4. Random inputs against the float64 log-sum-exp under the DERIVED bound lse_lib.lse_bound; the worst |err| / bound is printed.
5. lse with 2 and 4 ranges against one range under the same bound; O under the project's bound.
6. The merge on exact inputs: pass-through bit for bit, both empty, the exact mean, in place, cu_q.
7. The merge on random inputs against merge64.
8. The cascade against the float64 attention over prefix + suffix, against the single-level call, with one and two prefix groups.
9. [prefix call, suffix call, merge] captured once on one stream and replayed after cu_q and kv_len advanced.

Inputs, references and bounds: tests/lse_lib.py on top of tests/varlen_lib.py, bf16_lib.py, local_lib.py and decode_lib.py."""
import math

import numpy as np
import pytest
import torch

from tests import bf16_lib as bl
from tests import decode_lib as dl
from tests import local_lib as ll
from tests import lse_lib as sl
from tests import tol
from tests import varlen_lib as vl
from tests.decode_lib import _capi, _cuda
from tests.lse_lib import H, HKV, LENS, MAX_NQ, NCAP, NQS, SINKS, T_RAGGED, cache, el_of, tokens

pytestmark = pytest.mark.gpu
CASES = [(D, bf16, kind) for D in sl.DS for bf16 in (False, True) for kind in sl.KINDS]
IDS = [f"{D}-{'bf16' if b else 'f16'}-{k}" for D, b, k in CASES]
def f64(x):
    return x.float().cpu().double().numpy()


# ---- 1. O is the twin's

@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_o_is_the_twins_bit_for_bit_and_nobodys_rows_keep_their_sentinels(D, bf16, kind):
    _capi()
    c, q, cu = cache(D, bf16, LENS), tokens(D, bf16, T_RAGGED), vl.cu_of(NQS)
    n = sum(NQS)
    for split in (1, 3):
        for window, sinks in ((0, None), (45, SINKS)):
            want = sl.run_twin(kind, bf16, c, q, cu, LENS, MAX_NQ, causal=True, window=window, sinks=sinks, split=split)
            o, lse = sl.run(kind, bf16, c, q, cu, LENS, MAX_NQ, causal=True, window=window, sinks=sinks, split=split)
            assert bl.same(o, want), (split, window)
            assert (o[n:] == sl.o_sentinel(o.dtype)).all() and (lse[n:] == sl.LSE_SENTINEL).all(), (split, window)
            assert torch.isfinite(lse[:n]).all() and (lse[:n] != sl.LSE_SENTINEL).all(), (split, window)


# ---- 2. exact lse on uniform scores

@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_uniform_scores_give_k_ln2_within_one_ulp(D, bf16, kind):
    _capi()
    ks = tuple(range(8))
    ln2 = np.float32(math.log(2.0))
    for causal in (False, True):
        # non-causal: one token that sees all 2^k keys; causal: two tokens, the first sees 2^k of the 2^k + 1 keys
        nq = 2 if causal else 1
        lens = tuple(2 ** k + (1 if causal else 0) for k in ks)
        c = cache(D, bf16, lens, seed=2)
        q = torch.zeros(nq * len(ks), H, D, dtype=el_of(bf16))
        cu = vl.cu_of([nq] * len(ks))
        rows = [nq * k for k in ks]
        for split in (1, 2, 4):
            _, lse = sl.run(kind, bf16, c, q, cu, lens, nq, causal=causal, split=split)
            got = f64(lse)[rows]                                                        # [8, H]
            want = np.array([np.float32(k) * ln2 for k in ks], np.float64)[:, None]
            assert (np.abs(got - want) <= sl.ulp32(want)).all(), (causal, split, got[:, 0])
            assert (got[0] == 0).all(), (causal, split)                                 # one key: ln 1
            for s in (1.5, -2.0):
                sinks = torch.full((H,), s)
                _, lse = sl.run(kind, bf16, c, q, cu, lens, nq, causal=causal, sinks=sinks, split=split)
                got = f64(lse)[rows]
                want = np.log(np.array([2.0 ** k for k in ks]) + math.exp(s))[:, None]
                nv = np.array([2 ** k for k in ks])[:, None]
                assert (np.abs(got - want) <= sl.lse_bound(0.0, want, nv, D, s)).all(), (causal, split, s)
    # a row with no visible key and no sink: causal, three tokens on a cache of one key — tokens 0 and 1 sit in front of key 0
    c = cache(D, bf16, (1, 40), seed=3)
    q = tokens(D, bf16, 4)
    for split in (1, 2):
        o, lse = sl.run(kind, bf16, c, q, [0, 3, 4], (1, 40), 3, causal=True, split=split)
        assert (lse[:2] == -float("inf")).all() and (o[:2] == 0).all(), split
        assert torch.isfinite(lse[2:]).all(), split


# ---- 3. exact lse on one key

@pytest.mark.parametrize("max_nq", (4, 8, 16, 20), ids=("rt1", "rt2", "rt4", "rb2"))
@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_one_visible_key_gives_its_score_within_four_ulp(D, bf16, kind, max_nq):
    capi = _capi()
    lens, nqs = (130, 65, 3), (max_nq, 1, max_nq // 2 + 1)              # (sequence 2: its first tokens sit in front of key 0)
    g = torch.Generator().manual_seed(D + max_nq)
    k = torch.randint(-3, 4, (3, HKV, NCAP, D), generator=g).to(el_of(bf16))
    v = torch.randn(3, HKV, NCAP, D, generator=g).to(el_of(bf16))
    c = ll.Cache(k, v, lens, ps=16, seed=5)
    klog, _ = c.logical(kind)
    assert torch.equal(klog, k.double())                                  # (kv8: small integers over a power-of-two scale — the codes are exact)
    T = sum(nqs)
    q = torch.randint(-3, 4, (T, H, D), generator=g).to(el_of(bf16))
    cu = vl.cu_of(nqs)
    name = capi.attn_varlen_paged_lse_kernel_name(3, H, HKV, T, max_nq, 16, NCAP // 16, D, causal=True, window=1, kv8=kind == "kv8", bf16=bf16)
    assert name.startswith("attn_varlen_chunk_") == (max_nq == 20) and (max_nq == 20 or f",{dl.rt_of(H, HKV, max_nq)}>" in name), name
    want, _, nvis = sl.lse64(q, klog, cu, lens, max_nq, True, window=1)
    assert set(nvis.tolist()) <= {0, 1} and (nvis == 0).sum() == max(0, nqs[2] - 3)
    for split in (1, 2):
        o, lse = sl.run(kind, bf16, c, q, cu, lens, max_nq, causal=True, window=1, split=split)
        got = f64(lse)
        empty = nvis == 0
        assert (got[empty] == -np.inf).all() and (o.cpu()[torch.from_numpy(empty)] == 0).all(), split
        err = np.abs(got[~empty] - want[~empty])
        assert (err <= 4 * sl.ulp32(want[~empty])).all(), (split, float((err / sl.ulp32(want[~empty])).max()))


# ---- 4. random inputs under the derived bound

@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_random_inputs_stay_under_the_derived_bound(D, bf16, kind):
    _capi()
    c, q, cu = cache(D, bf16, LENS), tokens(D, bf16, T_RAGGED), vl.cu_of(NQS)
    klog, vlog = c.logical(kind)
    worst = 0.0
    for window, sinks in ((0, None), (45, SINKS)):
        want, A, nvis = sl.lse64(q, klog, cu, LENS, MAX_NQ, True, window=window, sinks=sinks)
        truth, nv2 = vl.ragged64(q, klog, vlog, cu, LENS, MAX_NQ, True, window=window, sinks=sinks)
        assert (nvis == nv2).all()
        for split in (0, 3):
            o, lse = sl.run(kind, bf16, c, q, cu, LENS, MAX_NQ, causal=True, window=window, sinks=sinks, split=split)
            r = sl.check_lse(f64(lse), want, A, nvis, D, sink=float(SINKS.abs().max()) if sinks is not None else 0.0, what=(window, split))
            sl.check_o(bf16, f64(o), truth, nvis, extra=0 if sinks is None else 1, what=(window, split))
            worst = max(worst, r)
    print(f"lse, D = {D} {'bf16' if bf16 else 'f16'} {kind}: worst |err| / bound {worst:.4f}")


# ---- 5. several ranges against one

@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_two_and_four_ranges_agree_with_one(D, bf16, kind):
    _capi()
    c, q, cu = cache(D, bf16, LENS), tokens(D, bf16, T_RAGGED), vl.cu_of(NQS)
    klog, vlog = c.logical(kind)
    want, A, nvis = sl.lse64(q, klog, cu, LENS, MAX_NQ, True, sinks=SINKS)
    truth, _ = vl.ragged64(q, klog, vlog, cu, LENS, MAX_NQ, True, sinks=SINKS)
    _, one = sl.run(kind, bf16, c, q, cu, LENS, MAX_NQ, causal=True, sinks=SINKS, split=1)
    for split in (2, 4):
        o, lse = sl.run(kind, bf16, c, q, cu, LENS, MAX_NQ, causal=True, sinks=SINKS, split=split)
        sl.check_lse(f64(lse), f64(one), A, nvis, D, sink=float(SINKS.abs().max()), what=("vs one range", split))
        sl.check_lse(f64(lse), want, A, nvis, D, sink=float(SINKS.abs().max()), what=("vs float64", split))
        sl.check_o(bf16, f64(o), truth, nvis, extra=1, what=split)


# ---- 6. the merge, exact

def merge(oa, la, ob, lb, **kw):
    capi = _capi()
    out = capi.attn_merge_states(*_cuda(oa, la, ob, lb), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D", sl.DS)
@pytest.mark.parametrize("bf16", (False, True), ids=("f16", "bf16"))
def test_merge_on_exact_inputs(D, bf16):
    el = el_of(bf16)
    g = torch.Generator().manual_seed(D + int(bf16))
    T = 37                                                                               # T H = 296 rows: more than one workgroup, a ragged last one
    oa, ob = (torch.randn(T, H, D, generator=g).to(el) for _ in range(2))
    oa[0, 0, :4] = torch.tensor([-0.0, 0.0, 65504.0 if not bf16 else 3.0e38, -1e-7]).to(el)      # signed zeros, the largest value, a tiny one
    la = torch.randn(T, H, generator=g) * 5
    ninf = torch.full((T, H), -float("inf"))
    # one side empty: the other passes through bit for bit, whatever the empty side's O holds — either way round
    for junk in (ob, torch.full_like(ob, float("nan"))):
        for out, lse in (merge(oa, la, junk, ninf), merge(junk, ninf, oa, la)):
            assert bl.same(out, oa) and torch.equal(lse.cpu(), la)
    # both empty
    out, lse = merge(oa, ninf, ob, ninf)
    assert (out == 0).all() and (lse == -float("inf")).all()
    # equal weights, small integers: the exact mean, lse + ln 2 within an ulp.  (la in +-[1, 30]: one fp32 ulp of la + ln 2 is attainable by an
    # fp32 sum only where it does not cancel — the error is half an ulp of the sum plus |fl(ln 2) - ln 2| = 1.9e-9, under one ulp from
    # |la + ln 2| >= 2^-5 on; here |la + ln 2| >= 0.3)
    ia, ib = (torch.randint(-8, 9, (T, H, D), generator=g).to(el) for _ in range(2))
    le = (1 + 29 * torch.rand(T, H, generator=g)) * (torch.randint(0, 2, (T, H), generator=g) * 2 - 1)
    out, lse = merge(ia, le, ib, le.clone())
    assert torch.equal(out.cpu().double(), (ia.double() + ib.double()) / 2)
    want = le.double().numpy() + math.log(2.0)
    assert (np.abs(f64(lse) - want) <= sl.ulp32(want)).all()
    # in place equals out of place, on either operand
    lb = la + torch.randn(T, H, generator=g)
    ref_o, ref_l = merge(oa, la, ob, lb)
    for first in (True, False):
        a, l1, b, l2 = _cuda(oa.clone(), la.clone(), ob.clone(), lb.clone())
        out, lse = merge(a, l1, b, l2, out=a if first else b, lse_out=l1 if first else l2)
        assert out.data_ptr() == (a if first else b).data_ptr()
        assert bl.same(out, ref_o) and torch.equal(lse, ref_l), first
    # cu_q: rows outside clamp(cu_q[0]) .. clamp(cu_q[B]) keep their sentinels, in O and in lse
    for cu, lo, hi in (([3, 10, 30], 3, 30), ([0, 5], 0, 5), ([-4, 9, 99], 0, T), ([12, 12], 12, 12)):
        out = torch.full((T, H, D), sl.o_sentinel(el), dtype=el, device="cuda")
        lse = torch.full((T, H), sl.LSE_SENTINEL, device="cuda")
        merge(oa, la, ob, lb, out=out, lse_out=lse, cu_q=vl.dev_i32(cu))
        keep = torch.ones(T, dtype=torch.bool)
        keep[lo:hi] = False
        assert (out.cpu()[keep] == sl.o_sentinel(el)).all() and (lse.cpu()[keep] == sl.LSE_SENTINEL).all(), cu
        assert bl.same(out[lo:hi], ref_o[lo:hi]) and torch.equal(lse[lo:hi], ref_l[lo:hi]), cu


# ---- 7. the merge, random

@pytest.mark.parametrize("D", sl.DS)
@pytest.mark.parametrize("bf16", (False, True), ids=("f16", "bf16"))
def test_merge_on_random_inputs_against_merge64(D, bf16):
    """O: the relative term of the project's bound (one 16-bit ulp of |truth|: the single rounding and headroom) plus half an ulp of the inputs —
    the fp32 arithmetic in between is orders below both.  lse: lse_lib.merge_lse_bound, 6 x 2^-24 + half an fp32 ulp of lse, derived there."""
    el = el_of(bf16)
    rtol = tol.ATTN_RTOL_BF16 if bf16 else tol.ATTN_RTOL_F16
    g = torch.Generator().manual_seed(5 * D + int(bf16))
    T = 61
    oa, ob = (torch.randn(T, H, D, generator=g).to(el) for _ in range(2))
    la = torch.randn(T, H, generator=g) * 6
    lb = la + torch.randn(T, H, generator=g) * torch.tensor([0.1, 1.0, 8.0, 40.0]).repeat(2)       # from equal weights to one side vanishing
    out, lse = merge(oa, la, ob, lb)
    want_o, want_l = sl.merge64(oa.double().numpy(), la.double().numpy(), ob.double().numpy(), lb.double().numpy())
    half_ulp_in = rtol / 2 * np.maximum(np.abs(oa.double().numpy()), np.abs(ob.double().numpy()))
    ro = np.abs(f64(out) - want_o) / (rtol * np.abs(want_o) + half_ulp_in)
    rl = np.abs(f64(lse) - want_l) / sl.merge_lse_bound(want_l)
    print(f"merge, D = {D} {'bf16' if bf16 else 'f16'}: worst O err / bound {ro.max():.3f}, worst lse err / bound {rl.max():.3f}")
    assert (ro <= 1).all() and (rl <= 1).all()


# ---- 8. the cascade

def cascade_setup(D, bf16, kind, groups):
    """three sequences with private suffixes of 5 / 40 / 70 keys and 1 / 1 / 7 new tokens behind shared prefixes.  groups: ((prefix keys,
    sequences), ...) — the logical cache holds the suffixes as entries 0 .. 2 and the prefixes behind them, in ONE pool"""
    suf, nqs = (5, 40, 70), (1, 1, 7)
    lens = suf + tuple(p for p, _ in groups)
    c = cache(D, bf16, lens, seed=4)
    klog, vlog = c.logical(kind)
    table = c.table8 if kind == "kv8" else c.table
    group_of = [gi for gi, (_, n) in enumerate(groups) for _ in range(n)]
    assert len(group_of) == 3
    kfull, vfull, tcat = [], [], []
    for b in range(3):
        P = groups[group_of[b]][0]
        assert P % 16 == 0                                                               # the prefix ends on a page boundary
        pb = 3 + group_of[b]
        kfull.append(torch.cat([klog[pb, :, :P], klog[b, :, :NCAP - P]], dim=1))
        vfull.append(torch.cat([vlog[pb, :, :P], vlog[b, :, :NCAP - P]], dim=1))
        tcat.append(torch.cat([table[pb, :P // 16], table[b, :NCAP // 16 - P // 16]]))
    cu = vl.cu_of(nqs)
    cu_groups = vl.cu_of([sum(nqs[b] for b in range(3) if group_of[b] == gi) for gi in range(len(groups))])
    return dict(c=c, klog=klog, vlog=vlog, table=table, kfull=torch.stack(kfull), vfull=torch.stack(vfull), tcat=torch.stack(tcat), cu=cu,
                cu_groups=cu_groups, suf=suf, nqs=nqs, full=tuple(groups[group_of[b]][0] + suf[b] for b in range(3)),
                plens=tuple(p for p, _ in groups), pseq=[3 + gi for gi in range(len(groups))],
                max_nq_prefix=max(cu_groups[i + 1] - cu_groups[i] for i in range(len(groups))))


def emulate_cascade(s, q, bf16, sinks):
    """the reference path on the CPU: float64 attention of each level, its O rounded to the 16-bit type, the merge in fp32, one more rounding"""
    el = el_of(bf16)
    T = q.shape[0]
    op, _ = vl.ragged64(q, s["klog"][s["pseq"]], s["vlog"][s["pseq"]], s["cu_groups"], s["plens"], s["max_nq_prefix"], False)
    lp, _, _ = sl.lse64(q, s["klog"][s["pseq"]], s["cu_groups"], s["plens"], s["max_nq_prefix"], False)
    os_, _ = vl.ragged64(q, s["klog"][:3], s["vlog"][:3], s["cu"], s["suf"], 7, True, sinks=sinks)
    ls, _, _ = sl.lse64(q, s["klog"][:3], s["cu"], s["suf"], 7, True, sinks=sinks)
    n = s["cu"][-1]
    r16 = lambda x: torch.from_numpy(x).to(el).float().numpy()
    a, b = r16(os_[:n]), r16(op[:n])
    la, lb = ls[:n].astype(np.float32), lp[:n].astype(np.float32)
    m = np.maximum(la, lb)
    wa, wb = np.exp(la - m, dtype=np.float32), np.exp(lb - m, dtype=np.float32)
    o = ((wa[..., None] * a + wb[..., None] * b) / (wa + wb)[..., None]).astype(np.float32)
    out = np.zeros((T,) + a.shape[1:])
    out[:n] = torch.from_numpy(o).to(el).double().numpy()
    return out


@pytest.mark.parametrize("groups", (((32, 3),), ((32, 2), (48, 1))), ids=("one_group", "two_groups"))
@pytest.mark.parametrize("D,bf16,kind", CASES, ids=IDS)
def test_cascade_against_float64_attention_over_prefix_and_suffix(D, bf16, kind, groups):
    capi = _capi()
    s = cascade_setup(D, bf16, kind, groups)
    c, cu = s["c"], s["cu"]
    n, T = cu[-1], cu[-1] + 2
    q = tokens(D, bf16, T, seed=8)
    sinks = SINKS if len(groups) == 2 else None
    extra = 0 if sinks is None else 1
    truth, nvis = vl.ragged64(q, s["kfull"], s["vfull"], cu, s["full"], 7, True, sinks=sinks)
    want_l, A, nv2 = sl.lse64(q, s["kfull"], cu, s["full"], 7, True, sinks=sinks)
    assert (nvis == nv2).all() and nvis[:n].min() >= groups[0][0] and (nvis[n:] == -1).all()
    # the reference path itself must sit inside the bound before the GPU is asked to
    frac = sl.check_o(bf16, emulate_cascade(s, q, bf16, sinks), truth, nvis, extra=extra, what="CPU emulation of the two-level path")
    assert frac < 1.0
    # the cascade
    qg, = _cuda(q)
    pools = _cuda(c.kp8, c.vp8) if kind == "kv8" else _cuda(c.kp, c.vp)
    scales = dict(k_scale=c.ks.cuda(), v_scale=c.vs.cuda()) if kind == "kv8" else {}
    o = torch.full_like(qg, sl.o_sentinel(qg.dtype))
    scratch = (torch.empty_like(qg), torch.empty(T, H, device="cuda"), torch.full((T, H), sl.LSE_SENTINEL, device="cuda"))
    out, lse = capi.attn_cascade_paged(qg, *pools, o, vl.dev_i32(s["cu_groups"]), s["table"][s["pseq"]].contiguous().cuda(), vl.dev_i32(s["plens"]),
                                       vl.dev_i32(cu), s["table"][:3].contiguous().cuda(), vl.dev_i32(s["suf"]), s["max_nq_prefix"], 7,
                                       sinks=None if sinks is None else sinks.cuda(), scratch=scratch, **scales)
    torch.cuda.synchronize()
    assert out.data_ptr() == o.data_ptr() and lse.data_ptr() == scratch[2].data_ptr()
    assert (o[n:] == sl.o_sentinel(o.dtype)).all() and (lse[n:] == sl.LSE_SENTINEL).all()
    r_o = sl.check_o(bf16, f64(o), truth, nvis, extra=extra, what="cascade")
    sink = float(SINKS.abs().max()) if sinks is not None else 0.0
    r_l = sl.check_lse(f64(lse), want_l, A, nvis, D, sink=sink, what="cascade lse")
    # the single-level call on the concatenated tables: the same bound, and the two agree under it
    o1, l1 = sl.run(kind, bf16, c, q, cu, s["full"], 7, causal=True, sinks=sinks, table=s["tcat"])
    sl.check_o(bf16, f64(o1), truth, nvis, extra=extra, what="single level")
    sl.check_lse(f64(l1), want_l, A, nvis, D, sink=sink, what="single level lse")
    sl.check_o(bf16, f64(o), f64(o1), nvis, extra=extra, what="cascade vs single level")
    print(f"cascade {len(groups)} group(s), D = {D} {'bf16' if bf16 else 'f16'} {kind}: CPU two-level path {frac:.3f} of the bound, "
          f"GPU O {r_o:.3f}, lse {r_l:.4f}")


# ---- 9. one cascade step as a graph

@pytest.mark.parametrize("bf16", (False, True), ids=("f16", "bf16"))
def test_a_cascade_step_is_captured_once_and_replayed(bf16):
    """[prefix call, suffix call, merge] captured as one chain on one stream (no parallel branches, no workspace: one KV range a level); cu_q
    and kv_len advance on the device between replays, and every replay equals the eager calls on the same state, bit for bit"""
    capi = _capi()
    D, T = 128, 16
    c = cache(D, bf16, (90, 140, 170, 32), seed=6)
    kp, vp, table = _cuda(c.kp, c.vp, c.table)
    ptab, stab = table[3:4].contiguous(), table[:3].contiguous()
    plen = vl.dev_i32([32])
    el = el_of(bf16)
    gen_ = torch.Generator().manual_seed(19)
    q = torch.randn(T, H, D, generator=gen_).to(el).cuda()
    cu_dev, cg_dev, len_dev = vl.dev_i32([0, 1, 2, 3]), vl.dev_i32([0, 3]), vl.dev_i32([5, 40, 70])
    g_o, e_o = (torch.full((T, H, D), sl.o_sentinel(el), dtype=el, device="cuda") for _ in range(2))
    g_s, e_s = ((torch.empty(T, H, D, dtype=el, device="cuda"), torch.empty(T, H, device="cuda"),
                 torch.full((T, H), sl.LSE_SENTINEL, device="cuda")) for _ in range(2))

    capi.tune("attn_decode_split", 1)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        sk = SINKS.cuda()

        def step(o, scratch):
            capi.attn_cascade_paged(q, kp, vp, o, cg_dev, ptab, plen, cu_dev, stab, len_dev, T, 8, scratch=scratch, sinks=sk)

        with torch.cuda.stream(st):
            step(torch.empty_like(g_o), tuple(torch.empty_like(x) for x in g_s))          # warm-up on buffers of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step(g_o, g_s)
        torch.cuda.synchronize()
        assert (g_o == sl.o_sentinel(el)).all()                                           # captured, not run
        lens = [5, 40, 70]
        for r, nqs in enumerate(((1, 1, 1), (8, 1, 5), (1, 2, 1))):
            lens = [x + n for x, n in zip(lens, nqs)]
            cu_dev.copy_(vl.dev_i32(vl.cu_of(nqs)))
            cg_dev.copy_(vl.dev_i32([0, sum(nqs)]))
            len_dev.copy_(vl.dev_i32(lens))
            q.copy_(torch.randn(q.shape, generator=gen_).to(el))
            for x in (g_o, e_o):
                x.fill_(sl.o_sentinel(el))
            for x in (g_s[2], e_s[2]):
                x.fill_(sl.LSE_SENTINEL)
            graph.replay()
            step(e_o, e_s)
            torch.cuda.synchronize()
            n = sum(nqs)
            assert torch.isfinite(g_o[:n].float()).all() and (g_o[n:] == sl.o_sentinel(el)).all() and (g_s[2][n:] == sl.LSE_SENTINEL).all(), r
            assert torch.isfinite(g_s[2][:n]).all(), r
            assert bl.same(g_o, e_o) and torch.equal(g_s[2], e_s[2]), r
    finally:
        capi.tune("attn_decode_split", 0)
