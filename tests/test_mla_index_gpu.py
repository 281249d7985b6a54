"""GPU tests of the lightning indexer (lc_mla_index_logits_f16 / _bf16, lc_mla_index_topk, capi.mla_index_select): the
logits against float64 under a derived bound, the selection bit for bit against a stable sort in numpy."""
import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import mla_lib as ml
from tests import test_mla_sparse_gpu as sp
from tests import tol

pytestmark = pytest.mark.gpu
ELS = pytest.mark.parametrize("el", (torch.half, torch.bfloat16), ids=("f16", "bf16"))
HI, DI, CANARY = 64, 128, -7777.25


def table_for(lens, page, seed, spare=3):   # (num_pages, table [B,max_pages] int32): shuffled, unused entries -1
    g = torch.Generator().manual_seed(seed)
    need = [(L + page - 1) // page for L in lens]
    ids = torch.randperm(sum(need) + spare, generator=g).tolist()
    table = torch.full((len(lens), max(need + [1])), -1, dtype=torch.int32)
    for b, n in enumerate(need):
        table[b, :n] = torch.tensor([ids.pop() for _ in range(n)], dtype=torch.int32)
    return sum(need) + spare, table


def visible(nq, lens, T, causal):   # (owner [T], n_t [T]) for cu_q = cumsum(nq): owner -1 and n_t 0 for a token nobody owns
    owner, n, t = np.full(T, -1), np.zeros(T, int), 0
    for b, (q, L) in enumerate(zip(nq, lens)):
        for i in range(q):
            owner[t], n[t] = b, max(0, min(L, L - q + i + 1)) if causal else L
            t += 1
    return owner, n


def slot_ref(table, num_pages, page, b, j):
    return np.clip(table[b].numpy()[j // page], 0, num_pages - 1) * page + j % page


def dev(*xs):
    return [x.cuda() for x in xs]


# (Nq, kv_len): every kv_len boundary of a 64-key tile, Nq = 1, 3, one more than the 8-token block, 70, a sequence without a token, one whose
# leading tokens see nothing (kv_len < Nq); one trailing token nobody owns
RAGGED = [(1, 1), (3, 63), (9, 64), (0, 65), (70, 130), (3, 65), (5, 3)]


@ELS
@pytest.mark.parametrize("page", (16, 64))
@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
def test_logits_match_float64_and_nothing_else_is_written(causal, page, el):
    """every written element within (Di + Hi + 4) 2^-24 A[t, j], A = sum_h |w_h| sum_d |q_hd k_d|: the products are exact in fp32, at most
    128 + 64 fp32 additions and one multiply round once each, relu is 1-Lipschitz"""
    nq, lens = [q for q, _ in RAGGED], [L for _, L in RAGGED]
    T = sum(nq) + 1
    g = torch.Generator().manual_seed(3 + page)
    num_pages, table = table_for(lens, page, seed=page)
    q, w = torch.randn(T, HI, DI, generator=g).to(el), torch.randn(T, HI, generator=g)
    pool = torch.randn(num_pages, page, DI, generator=g).to(el)
    owner, n = visible(nq, lens, T, causal)
    used = torch.zeros(num_pages * page, dtype=torch.bool)
    for b, L in enumerate(lens):
        if nq[b]:
            used[slot_ref(table, num_pages, page, b, np.arange(L))] = True
    pool.view(-1, DI)[~used] = float("nan")                                   # a slot no visible key maps to
    ld = table.shape[1] * page + 4
    logits = torch.full((T, ld), CANARY, device="cuda")
    cu = torch.tensor(np.concatenate([[0], np.cumsum(nq)]), dtype=torch.int32)
    capi.mla_index_logits(*dev(q, w, pool), logits, *dev(cu, table, torch.tensor(lens, dtype=torch.int32)), max(nq), causal=causal)
    got, worst = logits.cpu().double().numpy(), 0.0
    for t in range(T):
        assert (got[t, n[t]:] == CANARY).all(), t
        if n[t]:
            k = pool.view(-1, DI)[slot_ref(table, num_pages, page, owner[t], np.arange(n[t]))].double()
            prod = torch.einsum("hd,jd->hj", q[t].double(), k)
            A = torch.einsum("h,hj->j", w[t].double().abs(), torch.einsum("hd,jd->hj", q[t].double().abs(), k.abs())).numpy()
            want = (w[t].double()[:, None] * prod.clamp(min=0)).sum(0).numpy()
            worst = max(worst, (np.abs(got[t, :n[t]] - want) / ((DI + HI + 4) * 2.0 ** -24 * A)).max())
    print(f"logits {el} page {page} causal {causal}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("topk", (1, 5, 64, 300))
def test_topk_is_the_stable_sort_bit_for_bit(topk):
    """rows of n_t = 0, 1, topk - 1, topk, topk + 1, two compaction chunks and a bit, 70 000, and a causal three-token sequence; the logits are
    a few hundred distinct patterns (the threshold is always tied) with +-0, +-inf and NaNs of both signs; columns >= n_t hold +inf"""
    page, chunk = 64, 4096
    lens = [0, 1, topk - 1, topk, topk + 1, 2 * chunk + 5, 70000, topk + 2]
    nq = [1] * 7 + [3]
    T = sum(nq) + 1                                                            # the last token is nobody's
    owner, n = visible(nq, lens, T, True)
    num_pages, table = table_for(lens, page, seed=topk)
    table[6, 2], table[6, 5] = num_pages + 7, -3                               # out-of-range page ids: clamped
    rng = np.random.default_rng(topk)
    vals = np.concatenate([rng.standard_normal(300).astype(np.float32).view(np.uint32),
                           np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc00000, 0x7f800123], dtype=np.uint32)])
    ld = table.shape[1] * page
    bits = vals[rng.integers(0, len(vals), size=(T, ld))]
    want = np.full((T, topk), -1, dtype=np.int32)
    for t in range(T):
        bits[t, n[t]:] = 0x7f800000
        row = bits[t, :n[t]]
        key = np.where(row >> 31 != 0, ~row, row | np.uint32(0x80000000)).astype(np.int64)      # order-preserving
        keep = np.sort(np.argsort(-key, kind="stable")[:topk])
        if len(keep):
            want[t, :len(keep)] = slot_ref(table, num_pages, page, owner[t], keep)
    slots = torch.full((T, topk), 12345, dtype=torch.int32, device="cuda")
    cu = torch.tensor(np.concatenate([[0], np.cumsum(nq)]), dtype=torch.int32)
    capi.mla_index_topk(torch.from_numpy(bits.view(np.float32)).cuda(), slots, *dev(cu, table, torch.tensor(lens, dtype=torch.int32)), max(nq),
                        causal=True, page_size=page, num_pages=num_pages)
    assert torch.equal(slots.cpu(), torch.from_numpy(want))


def exact_step(nq, lens, page, el, seed):
    """inputs whose logits are exact and distinct by construction: w one-hot at a power of two, Qi two non-zero dims — (256, 1), on odd tokens
    (1, 256) —, Ki[., 0:2] the two base-256 digits of a permutation of the key positions: integers <= 256, exact in bf16, sums exact in fp32.
    Returns (q, w, pool, table, num_pages, score) with score(t, b, n) the float64 logits of token t over the first n keys of sequence b"""
    g = torch.Generator().manual_seed(seed)
    T = sum(nq)
    num_pages, table = table_for(lens, page, seed=seed)
    q, w, pool = torch.zeros(T, HI, DI), torch.zeros(T, HI), torch.zeros(num_pages * page, DI)
    perms = [torch.randperm(L, generator=g) for L in lens]
    for t in range(T):
        w[t, (7 * t + 3) % HI] = 2.0 ** (t % 5 - 2)
        q[t, (7 * t + 3) % HI, :2] = torch.tensor([256.0, 1.0] if t % 2 == 0 else [1.0, 256.0])
    for b, L in enumerate(lens):
        at = slot_ref(table, num_pages, page, b, np.arange(L))
        pool[at, 0], pool[at, 1] = (perms[b] // 256).float(), (perms[b] % 256).float()

    def score(t, b, n):
        hi, lo = (perms[b][:n] // 256).double().numpy(), (perms[b][:n] % 256).double().numpy()
        return float(w[t].sum()) * (256 * hi + lo if t % 2 == 0 else hi + 256 * lo)
    return q.to(el), w, pool.view(num_pages, page, DI).to(el), table, num_pages, score


def select_ref(nq, lens, table, num_pages, page, topk, score):
    T = sum(nq)
    owner, n = visible(nq, lens, T, True)
    want = np.full((T, topk), -1, dtype=np.int32)
    for t in range(T):
        s = score(t, owner[t], n[t])
        assert len(np.unique(s)) == len(s)
        keep = np.sort(np.argsort(-s, kind="stable")[:topk])
        want[t, :len(keep)] = slot_ref(table, num_pages, page, owner[t], keep)
    return torch.from_numpy(want)


@ELS
def test_select_is_exact_end_to_end(el):
    nq, lens, page, topk = [5, 1, 9], [200, 700, 40], 16, 64
    q, w, pool, table, num_pages, score = exact_step(nq, lens, page, el, seed=9)
    T = sum(nq)
    logits = torch.empty(T, table.shape[1] * page, device="cuda")
    slots = torch.empty(T, topk, dtype=torch.int32, device="cuda")
    cu = torch.tensor(np.concatenate([[0], np.cumsum(nq)]), dtype=torch.int32)
    out = capi.mla_index_select(*dev(q, w, pool), logits, slots, *dev(cu, table, torch.tensor(lens, dtype=torch.int32)), max(nq))
    assert out is slots and torch.equal(slots.cpu(), select_ref(nq, lens, table, num_pages, page, topk, score))


@ELS
def test_a_captured_step_is_replayed_on_a_longer_cache(el):
    """[mla_index_select -> attn_mla_sparse] captured once; kv_len and the index-key pool are rewritten on the device, then the graph is replayed
    (three times: the same bits every time)"""
    nq, page, topk, H = [2, 1], 16, 64, 16
    old, new = [150, 90], [155, 250]
    T = sum(nq)
    q, w, pool_new, table, num_pages, score = exact_step(nq, new, page, el, seed=4)
    g = torch.Generator().manual_seed(1)
    pool_old = torch.randn(pool_new.shape, generator=g).to(el)
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
    ckv, kpe = torch.randn(num_pages * page, ml.DC, generator=g).to(el), torch.randn(num_pages * page, ml.DR, generator=g).to(el)
    cu = torch.tensor([0, 2, 3], dtype=torch.int32)
    q_d, w_d, pool_d, cu_d, table_d, len_d = dev(q, w, pool_old, cu, table, torch.tensor(old, dtype=torch.int32))
    qc_d, qpe_d, ckv_d, kpe_d = dev(q_c, q_pe, ckv, kpe)
    logits = torch.empty(T, table.shape[1] * page, device="cuda")
    slots = torch.full((T, topk), -7, dtype=torch.int32, device="cuda")
    o = torch.full(q_c.shape, 768.0, dtype=el, device="cuda")

    def step(slots_, o_):
        capi.mla_index_select(q_d, w_d, pool_d, logits, slots_, cu_d, table_d, len_d, max(nq))
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
    pool_d.copy_(pool_new.cuda())
    len_d.copy_(torch.tensor(new, dtype=torch.int32).cuda())
    want = select_ref(nq, new, table, num_pages, page, topk, score)
    want_o, _, _, nvis = sp.ref64(q_c, q_pe, ckv, kpe, want, ml.SM_SCALE)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(slots.cpu(), want)
        ok, mx, _ = tol.attn_close(o.float().cpu().numpy(), want_o, int(nvis.max()), bf16=el == torch.bfloat16)
        assert ok, mx
