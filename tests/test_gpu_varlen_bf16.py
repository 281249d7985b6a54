"""GPU tests of the bfloat16 ragged-batch entries (lc_attn_varlen_paged_bf16 / _kv8_bf16, lc_rope_append_varlen_bf16 / _kv8_bf16; DESIGN.md
section 4.3m).

1. One visible key (causal, window = 1) is that key's V row, bit for bit — V holds bf16 values from 2^-40 to 2^40, which no fp16 decode survives.
2. Q = 0, small-integer V, power-of-two lengths: O is the mean of the visible V rows, bit for bit, with one KV range and with two and four.
3. Random inputs against the float64 definition under the project's bf16 bound, tol.attn_close(bf16=True); the worst ratio is printed.
4. The same with K entries around 1e5.
5. The fp8-cache call is the bf16 call on the dequantised pool, bit for bit.
6. A sequence's bits do not depend on its neighbours; rows nobody owns keep their sentinel.
7. Rotary embedding + append into bf16 pools: the derived bound, the quarter-turn table exactly, copies bit for bit, sentinels kept.
8. ... into fp8 pools: K codes are those of the bf16-rounded rotated row; V codes on all 65 536 bf16 bit patterns.
9. One step [rope_append_varlen_bf16, attn_varlen_paged_bf16] captured once on one stream and replayed after cu_q and kv_len advanced.

Inputs, truth and bounds: tests/bf16_lib.py on top of tests/varlen_lib.py, local_lib.py, rope_lib.py and decode_lib.py."""
import functools

import pytest
import torch

from tests import bf16_lib as bl
from tests import decode_lib as dl
from tests import rope_lib as rl
from tests import varlen_lib as vl
from tests.bf16_lib import BF, H, HEADS, HKV, NCAP, same
from tests.decode_lib import _capi, _cuda

pytestmark = pytest.mark.gpu
LENS = (1000, 129, 65)
# max_nq -> the plan with G = 4: RT = 1, 2, 4 and RB = 2 (R = 16, 32, 64, 80); the batch holds one sequence of max_nq tokens, one of one, one between
PLANS = (4, 8, 16, 20)


def nqs_of(max_nq):
    return (max_nq, 1, max_nq // 2 + 1)


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def cache(D, lens, seed=0):
    """bf16_cache of randn k, v [B,HKV,NCAP,D] (shared, never written to)"""
    g = gen(11, D, sum(lens), seed)
    k, v = (torch.randn(len(lens), HKV, NCAP, D, generator=g).to(BF) for _ in range(2))
    return bl.bf16_cache(k, v, lens, ps=16, seed=D + len(lens))


@functools.lru_cache(maxsize=None)
def tokens(D, T, seed=0):
    return torch.randn(T, H, D, generator=gen(3, D, T, seed)).to(BF)


def e4m3_grid(shape, scales, g):
    """bf16 [B,HKV,NCAP,D] of value(code) x scale[head] for random finite codes (exact), and the codes"""
    codes = dl.FINITE_CODES[torch.randint(0, len(dl.FINITE_CODES), shape, generator=g)]
    return bl.dequant_bf16(codes, scales), codes


# ---- 1. one visible key

@functools.lru_cache(maxsize=None)
def wide_cache(D, kind):
    """K randn; V: paged — sign x 2^e x (1 + m / 128) with e in [-40, 40]: values outside fp16's range and precision; kv8 — the e4m3 grid under
    decode_lib.V_SCALES, so that the codes of the cache are exact and O = value(code) x v_scale"""
    g = gen(17, D, len(kind))
    shape = (len(LENS), HKV, NCAP, D)
    k = torch.randn(shape, generator=g).to(BF)
    if kind == "kv8":
        v, codes = e4m3_grid(shape, dl.scales(dl.V_SCALES, HKV), g)
        c = bl.bf16_cache(k, v, LENS, ps=16, seed=D)
        assert torch.equal(c.v8, codes)
        return c
    e = torch.randint(-40, 41, shape, generator=g).double()
    m = torch.randint(0, 128, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    v64 = sign * torch.pow(torch.tensor(2.0, dtype=torch.float64), e) * (1 + m / 128)
    v = v64.to(BF)
    assert torch.equal(v.double(), v64) and float(v.double().abs().max()) > 65504 * 1e6 and float(v.double().abs().min()) < 1e-9
    return bl.bf16_cache(k, v, LENS, ps=16, seed=D)


@pytest.mark.parametrize("D", bl.DS)
@pytest.mark.parametrize("kind", bl.KINDS)
@pytest.mark.parametrize("max_nq", PLANS)
def test_one_visible_key_is_that_keys_value_row_bit_for_bit(D, kind, max_nq):
    c = wide_cache(D, kind)
    nqs = nqs_of(max_nq)
    cu = vl.cu_of(nqs)
    T = cu[-1]
    q = tokens(D, T)
    want = torch.zeros(T, H, D, dtype=BF)
    for b, n in enumerate(nqs):
        for i in range(n):
            want[cu[b] + i] = c.v[b, HEADS, LENS[b] - n + i]
    want = want + 0.0                                           # (an e4m3 code of -0: the accumulator 0 + 1 x -0 is +0)
    for split in (1, 3):
        got = bl.run(kind, c, q, cu, LENS, max_nq, window=1, split=split)
        assert same(got, want), (max_nq, split)


# ---- 2. the exact mean

MEAN_LENS = (1024, 128, 16)


@functools.lru_cache(maxsize=None)
def mean_cache(D):
    """K randn (Q = 0: every score is 0); V = integer in [-8, 8] x decode_lib.V_SCALES[head]: exact in bf16 and on the e4m3 grid"""
    g = gen(23, D)
    shape = (len(MEAN_LENS), HKV, NCAP, D)
    k = torch.randn(shape, generator=g).to(BF)
    vs = dl.scales(dl.V_SCALES, HKV)
    v64 = torch.randint(-8, 9, shape, generator=g).double() * vs.view(1, HKV, 1, 1).double()
    c = bl.bf16_cache(k, v64.to(BF), MEAN_LENS, ps=64, seed=D + 1)
    assert torch.equal(c.v.double(), v64) and torch.equal(bl.dequant_bf16(c.v8, vs).double(), v64)
    return c


@pytest.mark.parametrize("D", bl.DS)
@pytest.mark.parametrize("kind", bl.KINDS)
def test_zero_queries_give_the_exact_mean_with_one_two_and_four_ranges(D, kind):
    c = mean_cache(D)
    mean = torch.stack([c.v[b, :, :L].double().sum(dim=1) / L for b, L in enumerate(MEAN_LENS)])      # [B,HKV,D]: exact in float64
    for max_nq in (16, 20):                                    # RT = 4 and RB = 2
        nqs = nqs_of(max_nq)
        cu = vl.cu_of(nqs)
        T = cu[-1]
        want = torch.cat([mean[b][HEADS].unsqueeze(0).expand(n, H, D) for b, n in enumerate(nqs)]).float().to(BF)
        q = torch.zeros(T, H, D, dtype=BF)
        for split in (1, 2, 4):
            got = bl.run(kind, c, q, cu, MEAN_LENS, max_nq, causal=False, split=split)
            assert same(got, want), (max_nq, split)


# ---- 3. / 4. random inputs against the float64 definition

MIX_NQ = (1, 37, 1, 70, 5)
MIX_LENS = (1000, 129, 65, 577, 300)


def worst_ratio(kind, c, q, cu, lens, max_nq, cases):
    """the worst |err| / bound over the cases (window, sinks, split); every owned row is asserted under the bound on the way"""
    k64, v64 = c.logical(kind)
    worst = 0.0
    for window, sk, split in cases:
        truth, nvis = vl.ragged64(q, k64, v64, cu, lens, max_nq, True, window=window, sinks=sk)
        assert (nvis >= 1).all()
        got = bl.run(kind, c, q, cu, lens, max_nq, window=window, sinks=sk, split=split)
        worst = max(worst, bl.check_rows(got.float().cpu().numpy(), truth, nvis, what=(kind, window, split)))
    return worst


@pytest.mark.parametrize("D", bl.DS)
@pytest.mark.parametrize("kind", bl.KINDS)
def test_random_inputs_are_within_the_bf16_bound_of_the_float64_definition(D, kind):
    """Unit-variance randn Q, K, V; a step of prompts of 37, 70 and 5 tokens next to two sequences that decode one.  On an MI355X the worst
    |err| / bound of the four cases is printed (DESIGN.md section 4.3m records it); a CPU emulation of the kernel's roundings — bf16 P, fp32 sums,
    one bf16 rounding of O — stays at or below 0.26 of the bound on such inputs."""
    c = cache(D, MIX_LENS)
    cu = vl.cu_of(MIX_NQ)
    q = tokens(D, cu[-1])
    sinks = torch.randn(H, generator=gen(D))
    ratio = worst_ratio(kind, c, q, cu, MIX_LENS, 70, ((0, None, 0), (0, None, 3), (100, sinks, 0), (100, sinks, 3)))
    print(f"bf16 varlen {kind} D={D}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("kind", bl.KINDS)
def test_keys_around_1e5_are_not_decoded_as_fp16(kind):
    """K = 1e5 x randn — beyond fp16's 65504 — with Q scaled by 1e-5 so that the scores are those of test 3; the fp8 cache holds K under
    k_scale = 2^9, 2^10 (|K| / k_scale stays on the e4m3 grid's range; what is clamped is clamped in the reference's logical cache too)"""
    D = 128
    g = gen(29, len(kind))
    shape = (len(MIX_LENS), HKV, NCAP, D)
    k = (torch.randn(shape, generator=g) * 1e5).to(BF)
    v = torch.randn(shape, generator=g).to(BF)
    assert float(k.double().abs().max()) > 3e5
    c = bl.bf16_cache(k, v, MIX_LENS, ps=16, seed=9, k_scales=(2.0 ** 9, 2.0 ** 10))
    cu = vl.cu_of(MIX_NQ)
    q = (torch.randn(cu[-1], H, D, generator=g) * 1e-5).to(BF)
    ratio = worst_ratio(kind, c, q, cu, MIX_LENS, 70, ((0, None, 0), (0, None, 3)))
    print(f"bf16 varlen {kind} D={D}, |K| ~ 1e5: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ---- 5. the fp8 cache is the bf16 cache of the dequantised codes

@pytest.mark.parametrize("D", bl.DS)
def test_the_fp8_call_is_the_bf16_call_on_the_dequantised_pool_bit_for_bit(D):
    g = gen(31, D)
    shape = (len(LENS), HKV, NCAP, D)
    k, kc = e4m3_grid(shape, dl.scales(dl.K_SCALES, HKV), g)
    v, vc = e4m3_grid(shape, dl.scales(dl.V_SCALES, HKV), g)
    c = bl.bf16_cache(k, v, LENS, ps=16, seed=D + 2)
    assert torch.equal(c.k8, kc) and torch.equal(c.v8, vc)      # the bf16 pools hold value(code) x scale exactly
    sinks = torch.randn(H, generator=g)
    for max_nq in (4, 16, 20):                                  # RT = 1, RT = 4, RB = 2
        cu = vl.cu_of(nqs_of(max_nq))
        q = tokens(D, cu[-1], seed=1)
        for split in (1, 3):
            for window, sk in ((0, None), (100, sinks)):
                a = bl.run("kv8", c, q, cu, LENS, max_nq, window=window, sinks=sk, split=split)
                b = bl.run("paged", c, q, cu, LENS, max_nq, window=window, sinks=sk, split=split)
                assert torch.isfinite(b.float()).all() and same(a, b), (max_nq, split, window)


# ---- 6. neighbours

@pytest.mark.parametrize("D", bl.DS)
@pytest.mark.parametrize("kind", bl.KINDS)
def test_a_uniform_call_does_not_depend_on_its_neighbours(D, kind):
    c = cache(D, LENS)
    B = len(LENS)
    for Nq in (5, 20):                                          # RT = 2 and RB = 2
        cu = vl.cu_of([Nq] * B)
        T = cu[-1] + 3                                          # three rows at or past cu_q[B]
        q = tokens(D, T)
        for split in (1, 3):
            got = bl.run(kind, c, q, cu, LENS, Nq, split=split)
            assert (got[cu[-1]:] == bl.SENTINEL).all(), (Nq, split)
            assert torch.isfinite(got[:cu[-1]].float()).all() and (got[:cu[-1]] != bl.SENTINEL).any(dim=-1).all()
            for b in range(B):
                alone = bl.run(kind, c, q, cu[b:b + 2], LENS, Nq, split=split, seqs=[b])
                assert same(got[cu[b]:cu[b + 1]], alone[cu[b]:cu[b + 1]]), (Nq, split, b)
                rest = torch.cat([alone[:cu[b]], alone[cu[b + 1]:]])
                assert (rest == bl.SENTINEL).all(), (b, "the B = 1 call wrote a row of another sequence")


# ---- 7. rotary embedding + append, bf16 pools

ROPE_NQ = (3, 10, 40)
ROPE_LENS = (1000, 129, 65)


def sentinel_pools(c, kv8):
    src = (c.kp8, c.vp8) if kv8 else (c.kp, c.vp)
    if kv8:
        return [torch.full(x.shape, bl.SENT8, dtype=torch.uint8, device="cuda") for x in src]
    return [torch.full(x.shape, bl.SENT16, dtype=torch.int16, device="cuda").view(BF) for x in src]


def rope_sources(D, seed, strided):
    """(q [T,H,D], k_new, v_new [T,HKV,D]) bf16 on the GPU: views into a projection output whose rows are 8 elements longer, or dense"""
    T = vl.cu_of(ROPE_NQ)[-1] + 3                               # three tokens past cu_q[B]
    wide = torch.randn(T, (H + 2 * HKV) * D + 8, generator=gen(37, D, seed)).to(BF).cuda()
    qkv = wide[:, :(H + 2 * HKV) * D]
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)
    return (qv, kv, vv) if strided else (qv.contiguous(), kv.contiguous(), vv.contiguous())


def rope_truth(x, pos, table, interleaved):
    """rope_lib.rope_ref on token-major rows x [T,heads,D] at per-token positions: (exact, e) float64 [T,heads,D]"""
    exact, e = rl.rope_ref(x.cpu().permute(1, 0, 2).unsqueeze(0), pos.view(1, -1), table, interleaved)
    return exact[0].permute(1, 0, 2), e[0].permute(1, 0, 2)


@pytest.mark.parametrize("D", bl.DS)
@pytest.mark.parametrize("interleaved", (False, True), ids=("neox", "gptj"))
def test_rope_into_bf16_pools_obeys_the_derived_bound(D, interleaved):
    capi = _capi()
    c = cache(D, ROPE_LENS)
    cu = vl.cu_of(ROPE_NQ)
    n = cu[-1]
    table = c.table.cuda()
    for rot in (D, D // 2):
        for pinned in (False, True):
            cs = (rl.pinned_table(rot, NCAP) if pinned else rl.random_table(rot, NCAP))
            for strided in (True, False):
                qv, kv, vv = rope_sources(D, rot + int(pinned), strided)
                T = qv.shape[0]
                seq, pos = bl.token_positions(cu, ROPE_LENS, T, 40)
                assert (seq[:n] >= 0).all() and (seq[n:] < 0).all() and (pos >= 0).all()
                pools = sentinel_pools(c, False)
                q_src = qv.clone()
                in_place = not strided
                q_out = qv if in_place else torch.full((T, H, D), bl.SENTINEL, dtype=BF, device="cuda")
                tail = qv[n:].clone()
                got_q = capi.rope_append_varlen_bf16(qv, kv, vv, pools[0], pools[1], cs.cuda(), vl.dev_i32(cu), table, vl.dev_i32(ROPE_LENS), 40,
                                                     q_out=q_out, interleaved=interleaved)
                torch.cuda.synchronize()
                assert got_q is q_out
                what = (D, interleaved, rot, pinned, strided)
                got_q, kp, vp = got_q.cpu(), pools[0].cpu(), pools[1].cpu()
                # Qout: the bound on the owned rows, nothing written past cu_q[B]
                exact, e = rope_truth(q_src, pos, cs, interleaved)
                assert not bl.rope_violations(got_q[:n], exact[:n], e[:n]).any(), (what, "Qout")
                assert same(got_q[n:], tail.cpu() if in_place else torch.full((T - n, H, D), bl.SENTINEL, dtype=BF)), (what, "rows nobody owns")
                assert same(got_q[:n, :, rot:], q_src.cpu()[:n, :, rot:]), (what, "the tail of Q is not a copy")
                # the K rows gathered back from the pool, V and the tail bit for bit
                exact_k, e_k = rope_truth(kv, pos, cs, interleaved)
                got_k, got_v = bl.pool_rows(kp, c.table, seq, pos), bl.pool_rows(vp, c.table, seq, pos)
                assert not bl.rope_violations(got_k[:n], exact_k[:n], e_k[:n]).any(), (what, "K")
                assert same(got_k[:n, :, rot:], kv.cpu()[:n, :, rot:]), (what, "the tail of K is not a copy")
                assert same(got_v[:n], vv.cpu()[:n]), (what, "V is not a copy")
                if pinned:                                       # a signed permutation: exact
                    assert torch.equal(got_q[:n].double(), exact[:n]) and torch.equal(got_k[:n].double(), exact_k[:n]), (what, "quarter turns")
                # rows and pages the step does not own
                w = bl.written_mask(kp, c.table, seq, pos)
                assert int(w.sum()) == HKV * n
                for pool in (kp, vp):
                    assert (bl.bits(pool)[~w] == bl.SENT16).all(), (what, "a row nobody names was written")


# ---- 8. rotary embedding + append, fp8 pools

@pytest.mark.parametrize("D", bl.DS)
@pytest.mark.parametrize("interleaved", (False, True), ids=("neox", "gptj"))
def test_rope_into_fp8_pools_quantises_the_bf16_rounded_row(D, interleaved):
    """K codes = quantize(the K row the bf16-pool call stores, k_scale), byte for byte: the same rows through both calls, so that no rounding
    tie of the rotation is argued a second time; V codes = quantize(V, v_scale); Qout is the bf16-pool call's"""
    capi = _capi()
    c = cache(D, ROPE_LENS)
    cu = vl.cu_of(ROPE_NQ)
    n = cu[-1]
    ks, vs = torch.tensor([0.3, 2.0 ** -3]), torch.tensor([2.0 ** -2, 1.7 / 448])
    for rot in (D, D // 2):
        cs = rl.random_table(rot, NCAP).cuda()
        qv, kv, vv = rope_sources(D, rot, True)
        T = qv.shape[0]
        seq, pos = bl.token_positions(cu, ROPE_LENS, T, 40)
        args = (cs, vl.dev_i32(cu), c.table.cuda(), vl.dev_i32(ROPE_LENS), 40)
        p16, p8 = sentinel_pools(c, False), sentinel_pools(c, True)
        q16 = capi.rope_append_varlen_bf16(qv, kv, vv, p16[0], p16[1], *args, interleaved=interleaved)
        q8 = capi.rope_append_varlen_kv8_bf16(qv, kv, vv, p8[0], p8[1], *args, interleaved=interleaved, k_scale=ks.cuda(), v_scale=vs.cuda())
        torch.cuda.synchronize()
        assert same(q8[:n], q16[:n]), (rot, "Qout")
        w = bl.written_mask(c.kp, c.table, seq, pos)
        want_k, want_v = dl.quantize(p16[0].cpu(), ks), dl.quantize(p16[1].cpu(), vs)
        for got, want, name in ((p8[0].cpu(), want_k, "K"), (p8[1].cpu(), want_v, "V")):
            assert torch.equal(got[w], want[w]), (rot, name)
            assert (got[~w] == bl.SENT8).all(), (rot, name, "a row nobody names was written")
        assert same(bl.pool_rows(p16[1].cpu(), c.table, seq, pos)[:n], vv.cpu()[:n])


def test_fp8_codes_of_every_bf16_bit_pattern():
    """One call, one sequence of 512 tokens, D = 128, four K / V heads: every head of V holds all 65 536 bf16 bit patterns, shuffled, under the
    scales 1.0, 2^-3, 0.3 and 1.7 / 448.  code = (x.float() / scale).clamp(+-448).to(float8_e4m3fn), byte for byte; a NaN's code has 0x7F set.
    The table is the identity (cos 1, sin 0); K holds finite randn values."""
    capi = _capi()
    Hkv, T, D, ps = 4, 512, 128, 64
    g = gen(41)
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v_new = torch.stack([every[torch.randperm(65536, generator=g)] for _ in range(Hkv)]).view(Hkv, T, D).permute(1, 0, 2).contiguous().view(BF)
    k_new = torch.randn(T, Hkv, D, generator=g).to(BF)
    q = torch.randn(T, Hkv, D, generator=g).to(BF)
    cs = torch.cat([torch.ones(T, D // 2), torch.zeros(T, D // 2)], dim=1)
    mp = T // ps
    table = torch.randperm(mp + 3, generator=g)[:mp].view(1, mp).to(torch.int32)
    pools = [torch.full((mp + 3, Hkv, ps, D), bl.SENT8, dtype=torch.uint8, device="cuda") for _ in range(2)]
    ks, vs = torch.ones(Hkv), torch.tensor(bl.ALL_V_SCALES)
    capi.rope_append_varlen_kv8_bf16(q.cuda(), k_new.cuda(), v_new.cuda(), pools[0], pools[1], cs.cuda(), vl.dev_i32([0, T]), table.cuda(),
                                     vl.dev_i32([T]), T, k_scale=ks.cuda(), v_scale=vs.cuda())
    torch.cuda.synchronize()
    seq, pos = bl.token_positions([0, T], (T,), T, T)
    got = bl.pool_rows(pools[1].cpu(), table, seq, pos)                      # [T,Hkv,D] codes
    want = (v_new.float() / vs.view(1, Hkv, 1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    nan = torch.isnan(v_new.float())
    assert int(nan.sum()) == Hkv * 2 * 127 and ((want[nan] & 0x7F) == 0x7F).all()
    assert ((got[nan] & 0x7F) == 0x7F).all(), "a NaN's code is not a NaN"
    bad = (got != want) & ~nan
    assert not bad.any(), (int(bad.sum()), [hex(int(x) & 0xFFFF) for x in bl.bits(v_new)[bad][:8]], got[bad][:8].tolist(), want[bad][:8].tolist())
    # K under the identity table and scale 1.0: the codes of the rows themselves
    got_k = bl.pool_rows(pools[0].cpu(), table, seq, pos)
    assert torch.equal(got_k, dl.quantize(k_new, 1.0))


# ---- 9. one step as a graph

def test_a_bf16_step_is_captured_once_and_replayed():
    """[rope_append_varlen_bf16, attn_varlen_paged_bf16 with split-KV on a caller workspace] captured as one chain on one stream; cu_q and
    kv_len advance on the device between replays, and every replay equals the eager calls on the same state, bit for bit"""
    capi = _capi()
    D, ps, B, T, max_nq = 64, 16, 3, 32, 20
    base = (500, 129, 65)
    c = cache(D, (524, 151, 71), seed=1)                        # the lengths after the steps: every appended position lies in a page of its sequence
    gen_ = gen(43)
    cs = capi.rope_table(NCAP, D).cuda()
    tg, = _cuda(c.table)
    g_pools, e_pools = ([x.clone().cuda() for x in (c.kp, c.vp)] for _ in range(2))
    g_len, e_len = (torch.tensor(base, dtype=torch.int32, device="cuda") for _ in range(2))
    cu_dev = vl.dev_i32([0, 1, 2, 3])
    qkv = torch.randn(T, (H + 2 * HKV) * D, generator=gen_).to(BF).cuda()
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)
    g_q, e_q, g_o, e_o = (torch.full((T, H, D), bl.SENTINEL, dtype=BF, device="cuda") for _ in range(4))
    capi.tune("attn_decode_split", 3)
    try:
        ws = torch.empty(capi.attn_varlen_paged_workspace_bytes(B, H, HKV, T, max_nq, ps, NCAP // ps, D), dtype=torch.uint8, device="cuda")
        assert ws.numel() == 3 * T * H * (D + 1) * 4

        def step(pools, lens_dev, out_q, out_o):
            capi.rope_append_varlen_bf16(qv, kv, vv, pools[0], pools[1], cs, cu_dev, tg, lens_dev, max_nq, q_out=out_q)
            capi.attn_varlen_paged_bf16(out_q, pools[0], pools[1], out_o, cu_dev, tg, lens_dev, max_nq, causal=True, workspace=ws)

        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            step([x.clone() for x in g_pools], g_len.clone(), torch.empty_like(g_q), torch.empty_like(g_o))      # warm-up on state of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step(g_pools, g_len, g_q, g_o)
        torch.cuda.synchronize()
        assert (g_o == bl.SENTINEL).all()                                                     # captured, not run
        lens = list(base)
        for r, nqs in enumerate(((20, 1, 5), (1, 1, 1))):
            lens = [x + n for x, n in zip(lens, nqs)]                                         # kv_len is the length AFTER the step's append
            cu_dev.copy_(vl.dev_i32(vl.cu_of(nqs)))
            for x in (g_len, e_len):
                x.copy_(vl.dev_i32(lens))
            qkv.copy_(torch.randn(qkv.shape, generator=gen_).to(BF))
            for x in (g_q, e_q, g_o, e_o):
                x.fill_(bl.SENTINEL)
            graph.replay()
            step(e_pools, e_len, e_q, e_o)
            torch.cuda.synchronize()
            n = sum(nqs)
            assert torch.isfinite(g_o[:n].float()).all() and (g_o[:n] != bl.SENTINEL).any(dim=-1).all() and (g_o[n:] == bl.SENTINEL).all(), r
            assert same(g_o, e_o) and same(g_q, e_q), r
            assert all(same(a, b) for a, b in zip(g_pools, e_pools)), r
    finally:
        capi.tune("attn_decode_split", 0)
