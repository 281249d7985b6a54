"""GPU tests of the fp8 lightning indexer (lc_mla_index_logits_fp8, lc_mla_index_append_fp8_*, capi.mla_index_select_fp8)."""
import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import mla_lib as ml
from tests import test_mla_index_gpu as mi
from tests import test_mla_sparse_gpu as sp
from tests import tol

pytestmark = pytest.mark.gpu
F8, HI, DI, CANARY = torch.float8_e4m3fn, mi.HI, mi.DI, mi.CANARY
ELS = pytest.mark.parametrize("el", (torch.half, torch.bfloat16), ids=("f16", "bf16"))

# (Nq, kv_len): the boundaries of a 128-key tile and of 8- and 16-token blocks; one trailing token nobody owns.  "wave4": max_nq = 70, the
# 16-token kernel; "wave2": the sequences of at most 8 tokens (and a full 8-token block) on their own, the 8-token kernel
RAGGED = [(1, 1), (3, 127), (9, 128), (0, 129), (17, 128), (70, 260), (3, 129), (5, 3)]
BATCHES = {"wave4": RAGGED, "wave2": [c for c in RAGGED if c[0] <= 8] + [(8, 131)]}
C_BOUND = 2.0 ** -17


codes = lambda x: x.to(F8).view(torch.uint8)   # noqa: E731


def logits_rows(batch, page, causal, q8, w, k8, ks):
    """runs the entry (unmapped slots: NaN codes and scales), checks the canary behind n_t, yields (got, float64 formula, A) per visible token"""
    nq, lens = [q for q, _ in batch], [L for _, L in batch]
    T = sum(nq) + 1
    num_pages, table = mi.table_for(lens, page, seed=page)
    owner, n = mi.visible(nq, lens, T, causal)
    used = torch.zeros(num_pages * page, dtype=torch.bool)
    for b, L in enumerate(lens):
        if nq[b]:
            used[mi.slot_ref(table, num_pages, page, b, np.arange(L))] = True
    k8, ks = k8[:num_pages * page].clone(), ks[:num_pages * page].clone()
    k8[~used], ks[~used] = 0x7F, float("nan")
    logits = torch.full((T, table.shape[1] * page + 4), CANARY, device="cuda")
    cu = torch.tensor(np.concatenate([[0], np.cumsum(nq)]), dtype=torch.int32)
    capi.mla_index_logits_fp8(*mi.dev(q8[:T], w[:T], k8.view(num_pages, page, DI), ks.view(num_pages, page)), logits,
                              *mi.dev(cu, table, torch.tensor(lens, dtype=torch.int32)), max(nq), causal=causal)
    got = logits.cpu().double()
    qv, kv = q8.view(F8).double(), k8.view(F8).double()
    for t in range(T):
        assert (got[t, n[t]:] == CANARY).all(), t
        if n[t]:
            at = mi.slot_ref(table, num_pages, page, owner[t], np.arange(n[t]))
            prod = torch.einsum("hd,jd->hj", qv[t], kv[at])
            want = ks[at].double() * (w[t].double()[:, None] * prod.clamp(min=0)).sum(0)
            A = ks[at].double().abs() * torch.einsum("h,hj->j", w[t].double().abs(), torch.einsum("hd,jd->hj", qv[t].abs(), kv[at].abs()))
            yield got[t, :n[t]], want, A


GRID = pytest.mark.parametrize("causal,page,batch", [(c, p, b) for b in BATCHES for p in (16, 64) for c in (True, False)])
TMAX, SLOTS = sum(q for q, _ in RAGGED) + 1, 1600   # (more than any batch and table here needs)


@GRID
def test_logits_are_exact_on_integer_sums(causal, page, batch):
    """codes in [-4, 4], w in [-3, 3], power-of-two scales: every partial sum is an integer below 2^24, exact under any internal alignment"""
    g = torch.Generator().manual_seed(11 + page)
    q8, k8 = codes(torch.randint(-4, 5, (TMAX, HI, DI), generator=g).float()), codes(torch.randint(-4, 5, (SLOTS, DI), generator=g).float())
    w, ks = torch.randint(-3, 4, (TMAX, HI), generator=g).float(), torch.exp2(torch.randint(-3, 3, (SLOTS,), generator=g).float())
    rows = list(logits_rows(BATCHES[batch], page, causal, q8, w, k8, ks))
    assert rows and all(torch.equal(got, want) for got, want, _ in rows)


@GRID
def test_logits_match_float64_on_random_inputs(causal, page, batch):
    """randn rows quantised at amax / 448, the query scale folded into w: within C_BOUND A[t, j], A = |ks| sum_h |w_h| sum_d |q_hd k_d|.  The
    instruction's internal alignment is narrower than fp32 (tol.fp8_atol), so the bound is measured: the worst err / A of these 16 cases on an
    MI355X is 2^-19.61, C_BOUND = 2^-17 the power of two at or above four times that; the ceiling 2^-12 (a dropped scale costs 2^-3)"""
    g = torch.Generator().manual_seed(5 + page)
    q, k = torch.randn(TMAX, HI, DI, generator=g), torch.randn(SLOTS, DI, generator=g)
    sq, ks = q.abs().amax(-1) / 448, k.abs().amax(-1) / 448
    w = torch.randn(TMAX, HI, generator=g) * sq
    worst = max((got - want).abs().div(A).max().item() for got, want, A in logits_rows(BATCHES[batch], page, causal, codes(q / sq[..., None]), w,
                                                                                     codes(k / ks[:, None]), ks))
    print(f"fp8 logits {batch} page {page} causal {causal}: worst err / A = 2^{np.log2(worst):.2f}")
    assert C_BOUND <= 2.0 ** -12 and worst <= C_BOUND


def quantise_ref(x, pow2):
    s = x.float().abs().amax(-1).clamp_min(1e-4) / 448
    if pow2:
        m, e = torch.frexp(s)
        s = torch.ldexp(torch.ones_like(s), e - (m == 0.5).int())
    return codes(x.float() / s[:, None]), s


@ELS
@pytest.mark.parametrize("pow2", (True, False), ids=("pow2", "exact"))
def test_append_quantises_and_scatters(pow2, el):
    """a strided view, a zero row, a row at +-65504; dropped: a token without a position, one on a bad page id, an unowned one; canaries stay"""
    nq, lens, page = [3, 1, 6, 2], [40, 17, 5, 65], 16
    T = sum(nq) + 1
    g = torch.Generator().manual_seed(7)
    wide = (torch.randn(T, DI + 8, generator=g) * torch.exp2(torch.randint(-12, 9, (T, 1), generator=g).float())).to(el)
    x = wide[:, 8:]
    x[0], x[1, ::2], x[1, 1::2] = 0, 65504.0, -65504.0
    num_pages, table = mi.table_for(lens, page, seed=2)
    table[3, 4] = num_pages + 3                                                  # position 64, the last token of the last sequence
    want8, want_s = torch.full((num_pages * page, DI), 0xAB, dtype=torch.uint8), torch.full((num_pages * page,), CANARY)
    c8, s = quantise_ref(x, pow2)
    t = 0
    for b, (q, L) in enumerate(zip(nq, lens)):
        for i in range(q):
            p, pid = L - q + i, int(table[b, max(L - q + i, 0) // page])
            if p >= 0 and 0 <= pid < num_pages:
                want8[pid * page + p % page], want_s[pid * page + p % page] = c8[t], s[t]
            t += 1
    pool, scale = torch.full((num_pages, page, DI), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((num_pages, page), CANARY, device="cuda")
    cu = torch.tensor(np.concatenate([[0], np.cumsum(nq)]), dtype=torch.int32)
    capi.mla_index_append_fp8(wide.cuda()[:, 8:], pool, scale, *mi.dev(cu, table, torch.tensor(lens, dtype=torch.int32)), max(nq), pow2=pow2)
    assert (want_s != CANARY).sum() == sum(nq) - 2
    assert torch.equal(scale.cpu().view(-1), want_s) and torch.equal(pool.cpu().view(-1, DI), want8)


def digit_rows(values, el):   # [n] integers < 512 -> rows [n,128] holding their three base-8 digits: exact in e4m3 under a power-of-two scale
    rows = torch.zeros(len(values), DI)
    rows[:, 0], rows[:, 1], rows[:, 2] = values // 64, values // 8 % 8, values % 8
    return rows.to(el)


@ELS
def test_a_captured_step_appends_selects_and_attends(el):
    """[append -> select -> attn_mla_sparse] captured once, replayed twice on rewritten kv_len and keys.  exact_step's construction in e4m3's
    four bits: a key is three base-8 digits, Qi (64, 8, 1) in one head, w one-hot at a power of two — all exact, so the slots EQUAL the 16-bit
    mla_index_select's on the dequantised pool and queries; the appended rows dequantise to their sources"""
    nq, page, topk, H = [2, 1], 16, 64, 16
    lens = [[150, 90], [155, 250], [157, 251]]
    T = sum(nq)
    num_pages, table = mi.table_for(lens[-1], page, seed=4)
    g = torch.Generator().manual_seed(1)
    q, w = torch.zeros(T, HI, DI), torch.zeros(T, HI)
    for t in range(T):
        w[t, (7 * t + 3) % HI], q[t, (7 * t + 3) % HI, :3] = 2.0 ** (t % 5 - 2), torch.tensor([64.0, 8.0, 1.0])
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
    ckv, kpe = torch.randn(num_pages * page, ml.DC, generator=g).to(el), torch.randn(num_pages * page, ml.DR, generator=g).to(el)
    cu_d, table_d = mi.dev(torch.tensor([0, 2, 3], dtype=torch.int32), table)
    pool, scale = torch.zeros(num_pages, page, DI, dtype=torch.uint8, device="cuda"), torch.ones(num_pages, page, device="cuda")
    for b, L in enumerate(lens[-1]):                                           # the cache so far: one eager append per sequence
        capi.mla_index_append_fp8(digit_rows(torch.randperm(512, generator=g)[:L], el).cuda(), pool, scale, *mi.dev(torch.tensor([0, L], dtype=torch.int32)),
                                  table_d[b:b + 1], *mi.dev(torch.tensor([L], dtype=torch.int32)), L)
    new_d, len_d = digit_rows(torch.zeros(T, dtype=torch.long), el).cuda(), torch.tensor(lens[0], dtype=torch.int32).cuda()
    q8_d, w_d, q16_d = codes(q).cuda(), w.cuda(), q.to(el).cuda()
    qc_d, qpe_d, ckv_d, kpe_d = mi.dev(q_c, q_pe, ckv, kpe)
    logits = torch.empty(T, table.shape[1] * page, device="cuda")
    slots = torch.full((T, topk), -7, dtype=torch.int32, device="cuda")
    o = torch.full(q_c.shape, 768.0, dtype=el, device="cuda")

    def step(slots_, o_):
        capi.mla_index_append_fp8(new_d, pool, scale, cu_d, table_d, len_d, max(nq))
        capi.mla_index_select_fp8(q8_d, w_d, pool, scale, logits, slots_, cu_d, table_d, len_d, max(nq))
        capi.attn_mla_sparse(qc_d, qpe_d, ckv_d, kpe_d, o_, slots_, ml.SM_SCALE)
    st, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step(torch.empty_like(slots), torch.empty_like(o))                     # warm-up on buffers of its own
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=st):
            step(slots, o)
    torch.cuda.synchronize()
    assert (slots == -7).all() and (o == 768.0).all()                          # captured, not run
    for L in lens[1:]:
        new = digit_rows(torch.randint(0, 512, (T,), generator=g), el)
        new_d.copy_(new.cuda())
        len_d.copy_(torch.tensor(L, dtype=torch.int32).cuda())
        graph.replay()
        torch.cuda.synchronize()
        deq = (pool.view(F8).float() * scale[..., None]).to(el)
        at = [mi.slot_ref(table, num_pages, page, b, L[b] - nq[b] + i) for b in range(2) for i in range(nq[b])]
        assert torch.equal(deq.view(-1, DI)[at].cpu(), new)
        want = capi.mla_index_select(q16_d, w_d, deq, torch.empty_like(logits), torch.empty_like(slots), cu_d, table_d, len_d, max(nq))
        assert torch.equal(slots, want) and (slots[:, :topk] >= 0).all()
        want_o, _, _, nvis = sp.ref64(q_c, q_pe, ckv, kpe, want.cpu(), ml.SM_SCALE)
        ok, mx, _ = tol.attn_close(o.float().cpu().numpy(), want_o, int(nvis.max()), bf16=el == torch.bfloat16)
        assert ok, mx
