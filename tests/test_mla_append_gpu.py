"""GPU tests of lc_mla_append_paged_f16 / _bf16 / _kv8 / _kv8_bf16 against float64 from the 16-bit inputs.

The latent bound: |got - exact| <= e + half_ulp(|exact| + e), e = 2^-15 |exact|.  An fp32 sum of 512 non-negative terms in any order is within
512 x 2^-24 = 2^-15 of exact, relatively; its reciprocal root carries half of that; one ulp of the hardware reciprocal root and the two rounded
products add <= 2^-21: 2^-15 covers the total, and the one rounding to the element type adds the half ulp.  k_pe and q_pe: rope_lib's bound."""
import functools

import pytest
import torch

from leetcuda_amd import capi
from tests import bf16_lib as bl
from tests import mla_lib as ml
from tests import rope_lib as rl
from tests.decode_lib import forced_split, quantize
from tests.test_mla_gpu import ELS, O_CANARY, cu_of, i32

pytestmark = pytest.mark.gpu
KV8 = pytest.mark.parametrize("kv8", (False, True), ids=("p16", "p8"))
CU, LENS, PAGE, T, MAX_NQ = [0, 1, 6, 6, 76], (33, 3, 7, 100), 16, 80, 70      # Nq = 1, 5 (> kv_len: p = -2 ..), 0, 70 (p = 30 .. 99); 4 canary rows
SCALE, EPS, SENT8, ZERO_ROW, EDGE_ROW = 0.0123, 1e-6, 0x5A, 20, 5     # no power of two; tokens whose sources are zeros (p = 44) / extremes (p = 2)


@functools.lru_cache(maxsize=None)
def geometry(el, edge=False):
    """(kv [T,584], q [T,H=32,192], gamma, table, P, seq, pos, written tokens, their pages and slots): rows scaled by 2^-12, 1 and 2^10, one
    latent row of zeros and (edge: the exact tests) one token of largest finite and subnormal values"""
    g = torch.Generator().manual_seed(76)
    rows = torch.tensor([2.0 ** -12, 1.0, 2.0 ** 10])[torch.arange(T) % 3]
    kv, q = (torch.randn(T, 584, generator=g) * rows[:, None]).to(el), (torch.randn(T, 32, 192, generator=g) * rows[:, None, None]).to(el)
    kv[ZERO_ROW, :512] = 0
    fi = torch.finfo(el)
    ext = torch.tensor([fi.max, fi.smallest_normal * fi.eps, -fi.max, -fi.smallest_normal * fi.eps * 3], dtype=torch.float64).to(el)
    if edge:
        kv[EDGE_ROW, :576], q[EDGE_ROW] = ext.repeat(144), ext.repeat(48)
    _, _, table = ml.paged(LENS, PAGE, seed=3, el=el)
    P = int(table.max()) + 1 + 3
    table[3, 3] = P + 5                                                         # a bad page id: p = 48 .. 63 of the long sequence are dropped
    seq, pos = bl.token_positions(CU, LENS, T, MAX_NQ)
    pid = torch.where((seq >= 0) & (pos >= 0), table[seq.clamp(min=0), pos.clamp(min=0) // PAGE].long(), torch.full_like(pos, -1))
    w = ((pid >= 0) & (pid < P)).nonzero().flatten()
    return kv, q, torch.randn(512, generator=g), table, P, seq, pos, w, pid[w], pos[w] % PAGE


def rotated(x, pos, tab, il):
    """(exact, e) float64 of x [T,heads,64] rotated at pos [T] (rope_lib.rope_ref on one batch entry of T tokens)"""
    exact, e = rl.rope_ref(x.transpose(0, 1)[None], pos[None], tab, il)
    return exact[0].transpose(0, 1), e[0].transpose(0, 1)


def call(el, kv8, H, il, gamma, tab, edge=False, inplace=False):
    """(ckv_pool, kpe_pool, q_pe_out) after one call from sentinel pools on views of [T,584] and [T,H,192] (inplace: a dense q_pe = q_pe_out)"""
    kv, q, _, table, P, *_ = geometry(el, edge)
    kvd, qd = kv.cuda(), q[:, :H].contiguous().cuda()
    q_pe = qd[:, :, 128:].contiguous() if inplace else qd[:, :, 128:]
    ckv = torch.full((P, PAGE, 512), SENT8, dtype=torch.uint8).cuda() if kv8 else torch.full((P, PAGE, 512), bl.SENT16, dtype=torch.int16).view(el).cuda()
    kpe = torch.full((P, PAGE, 64), bl.SENT16, dtype=torch.int16).view(el).cuda()
    out = q_pe if inplace else torch.full((T, H, 64), bl.SENT16, dtype=torch.int16).view(el).cuda()
    args = (kvd[:, :512], kvd[:, 512:576], q_pe, ckv, kpe, tab.cuda(), i32(CU), table.cuda(), i32(LENS), MAX_NQ)
    kw = dict(gamma=None if gamma is None else gamma.cuda(), eps=EPS, q_pe_out=out, interleaved=il)
    (capi.mla_append_paged_kv8 if kv8 else capi.mla_append_paged)(*args, **kw, **(dict(ckv_scale=torch.tensor([SCALE], device="cuda")) if kv8 else {}))
    torch.cuda.synchronize()
    return ckv.cpu(), kpe.cpu(), out.cpu()


def check_rest(el, ckv, kpe, out):  # (the geometry's table and positions are the same with and without the edge token)
    """what no token owns keeps its bits: pool rows, the rows behind cu_q[B]; p < 0 rows of Qpe_out are zero"""
    *_, P, seq, pos, w, pid, slot = geometry(el)
    free = torch.ones(P, PAGE, dtype=torch.bool)
    free[pid, slot] = False
    sent = SENT8 if ckv.dtype == torch.uint8 else bl.SENT16
    assert (bl.bits(ckv)[free] == sent).all() and (bl.bits(kpe)[free] == bl.SENT16).all(), "a pool row nobody names was written"
    assert (bl.bits(out)[seq < 0] == bl.SENT16).all() and (bl.bits(out)[(seq >= 0) & (pos < 0)] == 0).all()
    assert int(((seq >= 0) & (pos < 0)).sum()) == 2 and len(w) == 76 - 2 - 16 and int((seq < 0).sum()) == 4      # (what the geometry is meant to hold)


@ELS
@KV8
@pytest.mark.parametrize("H,il", ((3, False), (32, True), (32, False)), ids=("H3-neox", "H32-gptj", "H32-neox"))
def test_a_ragged_batch_stays_inside_the_derived_bounds(el, kv8, H, il):
    kv, q, gamma, table, P, seq, pos, w, pid, slot = geometry(el)
    tab = rl.random_table(64)
    ckv, kpe, out = call(el, kv8, H, il, gamma, tab)
    check_rest(el, ckv, kpe, out)
    viol = bl.rope_violations if el == torch.bfloat16 else rl.violations
    x = kv[:, :512].double()
    exact = x * torch.rsqrt((x * x).mean(1, keepdim=True) + float(torch.tensor(EPS))) * gamma.double()     # eps as the float the call passes
    e = exact.abs() * 2.0 ** -15
    if kv8:      # the code of SOME 16-bit value inside the bound: the rounded exact value or one of its two neighbours
        b = bl.bits(exact.to(el)).int()
        down = torch.where((b & 0x7fff) == 0, (b ^ 0x8000) + 1, b - 1)
        ok = torch.zeros(len(w), 512, dtype=torch.bool)
        for cand in (b, b + 1, down):
            c = cand.to(torch.int16).view(el)[w]
            ok |= (quantize(c, SCALE) == ckv[pid, slot]) & ~viol(c, exact[w], e[w])
        assert ok.all(), f"{int((~ok).sum())} codes are the code of no 16-bit value inside the bound"
    else:
        bad = viol(ckv[pid, slot], exact[w], e[w])
        assert not bad.any() and (ckv[pid, slot][w == ZERO_ROW] == 0).all(), f"{int(bad.sum())} latent elements leave the bound"
    own = (seq >= 0) & (pos >= 0)                                                # (a token on a bad page still has its Qpe_out rows)
    (ke, kee), (qe, qee) = rotated(kv[:, None, 512:576], pos, tab, il), rotated(q[:, :H, 128:], pos, tab, il)
    for what, got, ex, ee in (("k_pe", kpe[pid, slot], ke[w, 0], kee[w, 0]), ("q_pe", out[own], qe[own], qee[own])):
        bad = viol(got, ex, ee)
        assert not bad.any(), f"{int(bad.sum())} {what} elements leave the rope bound"


@ELS
@KV8
@pytest.mark.parametrize("il", (False, True), ids=("neox", "gptj"))
def test_without_gamma_on_the_quarter_turn_table_every_byte_is_the_reference(el, kv8, il):
    kv, q, gamma, table, P, seq, pos, w, pid, slot = geometry(el, True)
    tab, H = rl.pinned_table(64), 3
    ckv, kpe, out = call(el, kv8, H, il, None, tab, edge=True)
    check_rest(el, ckv, kpe, out)
    assert bl.same(ckv[pid, slot], quantize(kv[w, :512], SCALE) if kv8 else kv[w, :512])
    assert bl.same(kpe[pid, slot], rotated(kv[:, None, 512:576], pos, tab, il)[0][w, 0].to(el))
    own = (seq >= 0) & (pos >= 0)
    assert bl.same(out[own], rotated(q[:, :H, 128:], pos, tab, il)[0][own].to(el))
    # a zero row under a gamma and eps > 0 is zeros (0 x a negative gamma: -0, the code 0x80), not NaN; in place on a dense q_pe: the same bits
    ckv_g, _, out2 = call(el, kv8, H, il, gamma, tab, edge=True, inplace=True)
    zero = ckv_g[pid, slot][w == ZERO_ROW]
    assert (((zero & 0x7f) == 0).all() if kv8 else (zero == 0).all()) and bl.same(out2[own], out[own])


@ELS
@KV8
def test_a_captured_append_and_attention_step_is_replayed_on_new_lengths(el, kv8):
    """[mla_append_paged -> attn_mla_paged] captured once (one KV range) and replayed — twice: the step is idempotent — after cu_q, kv_len and
    block_table changed on the device: O is bit for bit attn_mla_paged on pools built in torch from the reference rows"""
    H, Tn, max_nq, scale = 16, 7, 2, 2.0 ** -5
    old, new = ((1, 1), (60, 30)), ((2, 1), (70, 31))
    g = torch.Generator().manual_seed(5)
    q_c, q_pe, kv = (torch.randn(*s, generator=g).to(el) for s in ((Tn, H, 512), (Tn, H, 64), (Tn, 576)))
    ckv0, kpe0, table_new = ml.paged(new[1], PAGE, seed=9, el=el)
    table_old = torch.cat([table_new[:, :2].flip(1), table_new[:, 2:]], 1)
    tab, pool0 = rl.pinned_table(64), quantize(ckv0, scale) if kv8 else ckv0
    kvd, qd, qcd, cs = kv.cuda(), q_pe.cuda(), q_c.cuda(), tab.cuda()
    kw8 = dict(ckv_scale=torch.tensor([scale], device="cuda")) if kv8 else {}
    append, attend = (capi.mla_append_paged_kv8, capi.attn_mla_paged_kv8) if kv8 else (capi.mla_append_paged, capi.attn_mla_paged)
    attn = lambda qp, c, k, o, *a: attend(qcd, qp, c, k, o, *a, max_nq, ml.SM_SCALE, causal=True, **kw8)   # noqa: E731
    cu_d, len_d, tab_d = i32(cu_of(old[0])), i32(old[1]), table_old.cuda()

    def step(ckv, kpe, qo, o):
        append(kvd[:, :512], kvd[:, 512:], qd, ckv, kpe, cs, cu_d, tab_d, len_d, max_nq, q_pe_out=qo, **kw8)
        attn(qo, ckv, kpe, o, cu_d, tab_d, len_d)
    ckv, kpe, qo, o = pool0.cuda(), kpe0.cuda(), torch.empty_like(qd), torch.full(q_c.shape, O_CANARY, dtype=el, device="cuda")
    cu_new, o_r = cu_of(new[0]), torch.full_like(o, O_CANARY)
    seq, pos = bl.token_positions(cu_new, new[1], Tn, max_nq)
    own = seq >= 0
    pid, slot = table_new[seq[own], pos[own] // PAGE].long(), pos[own] % PAGE
    ckv_r, kpe_r, q_r = pool0.clone(), kpe0.clone(), torch.zeros_like(q_pe)      # the new tokens' rows put where the rule says, in torch
    ckv_r[pid, slot] = quantize(kv[own, :512], scale) if kv8 else kv[own, :512]
    kpe_r[pid, slot] = rotated(kv[:, None, 512:], pos, tab, False)[0][own, 0].to(el)
    q_r[own] = rotated(q_pe, pos, tab, False)[0][own].to(el)

    def body():
        st, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            step(ckv.clone(), kpe.clone(), torch.empty_like(qd), torch.empty_like(o))      # warm-up on buffers of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step(ckv, kpe, qo, o)
        torch.cuda.synchronize()
        assert (o == O_CANARY).all()                                                       # captured, not run
        for dst, src in ((cu_d, i32(cu_new)), (len_d, i32(new[1])), (tab_d, table_new.cuda())):
            dst.copy_(src)
        attn(q_r.cuda(), ckv_r.cuda(), kpe_r.cuda(), o_r, cu_d, tab_d, len_d)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert bl.same(ckv, ckv_r) and bl.same(kpe, kpe_r) and bl.same(o, o_r) and not (o[:3] == O_CANARY).all()
    forced_split(1, body)
