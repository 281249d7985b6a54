"""GPU tests of lc_attn_mla_prefill_f16 / _bf16 against a float64 reference: per sequence the visible keys
cat(k_nope, k_pe) of a head, then softmax, lse and P @ V.  Operands are strided views whose gaps and foreign rows are NaN."""
import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import lse_lib as sl
from tests import tol

pytestmark = pytest.mark.gpu
ELS = pytest.mark.parametrize("el", (torch.half, torch.bfloat16), ids=("f16", "bf16"))
O_CANARY, LSE_CANARY = 768.0, -4321.5     # exact in fp16 and bf16; a value no log-sum-exp here reaches
SM_SCALE = 1.0 / 192 ** 0.5
PAD = 3                                   # spare key rows in front of cu_k[0]


def inputs(H, nqs, lks, el, seed):
    """q [Tq,H,192] of a [Tq,H,200] buffer, k_nope / v the halves of a [Tk,H,256] buffer, k_pe [Tk,64] of a [Tk,72] buffer; Tq = sum Nq + 4,
    Tk = PAD + sum Lk + 2.  The gaps, the rows nobody owns and the key rows outside [cu_k[0], cu_k[B]) are NaN."""
    g = torch.Generator().manual_seed(seed)
    nq, nk = sum(nqs), sum(lks)
    qb, kvb, kpb = (torch.full(s, float("nan"), dtype=el) for s in ((nq + 4, H, 200), (PAD + nk + 2, H, 256), (PAD + nk + 2, 72)))
    qb[:nq, :, :192] = torch.randn(nq, H, 192, generator=g).to(el)
    kvb[PAD:PAD + nk] = torch.randn(nk, H, 256, generator=g).to(el)
    kpb[PAD:PAD + nk, :64] = torch.randn(nk, 64, generator=g).to(el)
    cu_q = torch.tensor(np.cumsum((0,) + tuple(nqs)), dtype=torch.int32)
    cu_k = torch.tensor(np.cumsum((PAD,) + tuple(lks)), dtype=torch.int32)
    return qb[:, :, :192], kvb[:, :, :128], kpb[:, :64], kvb[:, :, 128:], cu_q, cu_k


def ref64(q, kn, kpe, v, cu_q, cu_k, causal):
    """(O [Tq,H,128], lse [Tq,H], A [Tq,H], nvis [Tq]) in float64; A = max over the visible keys of sm_scale sum_d |q_d k_d| (lse_lib.lse_bound);
    nvis = -1: a row nobody owns"""
    Tq, H, _ = q.shape
    O, lse, A, nvis = np.zeros((Tq, H, 128)), np.full((Tq, H), -np.inf), np.zeros((Tq, H)), np.full(Tq, -1)
    for b in range(len(cu_q) - 1):
        (q0, q1), (k0, k1) = cu_q[b:b + 2].tolist(), cu_k[b:b + 2].tolist()
        keys = torch.cat([kn[k0:k1], kpe[k0:k1, None, :].expand(-1, H, -1)], -1).double()      # [Lk,H,192]
        for i in range(q1 - q0):
            n = min(max(k1 - k0 - (q1 - q0) + i + 1, 0), k1 - k0) if causal else k1 - k0
            nvis[q0 + i] = n
            if n:
                prod = q[q0 + i].double()[None] * keys[:n]                                   # [n,H,192]
                s = prod.sum(-1) * SM_SCALE
                A[q0 + i] = (prod.abs().sum(-1) * SM_SCALE).max(0).values.numpy()
                lse[q0 + i] = torch.logsumexp(s, 0).numpy()
                O[q0 + i] = torch.einsum("nh,nhd->hd", torch.softmax(s, 0), v[k0:k0 + n].double()).numpy()
    return O, lse, A, nvis


def device_views(q, kn, kpe, v):
    """the same strided views of DEVICE copies of the three buffers"""
    qb, kvb, kpb = (x._base.cuda() for x in (q, kn, kpe))
    return qb[:, :, :192], kvb[:, :, :128], kpb[:, :64], kvb[:, :, 128:]


def run(q, kn, kpe, v, cu_q, cu_k, max_nq, causal):
    """the call on strided device views; O and lse canary-filled"""
    o = torch.full((q.shape[0], q.shape[1], 128), O_CANARY, dtype=q.dtype, device="cuda")
    lse = torch.full(q.shape[:2], LSE_CANARY, device="cuda")
    capi.attn_mla_prefill(*device_views(q, kn, kpe, v), o, cu_q.cuda(), cu_k.cuda(), max_nq, SM_SCALE, lse=lse, causal=causal)
    torch.cuda.synchronize()
    return o, lse


def check(o, lse, want, N, bf16, what, rtol=None, lse_extra=0.0):
    """owned rows under the project's bounds (printed first), rows that see nothing exactly 0 / -inf, rows nobody owns untouched"""
    want_o, want_lse, A, nvis = want
    got, got_lse, own = o.float().cpu().numpy(), lse.cpu().numpy().astype(np.float64), nvis >= 0
    ok, mx, exc = tol.attn_close(got[own], want_o[own], N, bf16=bf16, rtol=rtol)
    fin = np.isfinite(want_lse)
    rl = float((np.abs(got_lse[fin] - want_lse[fin]) / (sl.lse_bound(A, want_lse, nvis[:, None], 192) + lse_extra)[fin]).max()) if fin.any() else 0.0
    print(f"{what}: O max |err| {mx:.3e} (excess {exc:.3e}); lse worst err / bound {rl:.3f}")
    assert ok, (what, mx)
    assert rl <= 1.0 and np.isfinite(got_lse[fin]).all(), (what, rl)
    assert (got[nvis == 0] == 0).all() and (got_lse[nvis == 0] == -np.inf).all(), what
    assert (got[~own] == O_CANARY).all() and (got_lse[~own] == LSE_CANARY).all(), what


# H, Nq_b, Lk_b, causal
CASES = [
    (2, (1, 64, 3), (1, 64, 65), True),      # RS 1: one key, a full tile, one key into a second tile
    (3, (127, 0, 129), (127, 5, 129), True), # both sides of the 128-row block; keys without a query; an odd head count
    (2, (70, 5), (200, 261), True),          # the diagonal crosses tiles inside a chunk behind a prefix; a fifth tile of 5 keys
    (2, (40,), (17,), True),                 # RS 1: rows with p < 0
    (2, (33, 130), (100, 67), False),        # ragged last tiles, no mask
]


@ELS
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"H{c[0]}-q{'_'.join(map(str, c[1]))}-k{'_'.join(map(str, c[2]))}-{'c' if c[3] else 'n'}")
def test_random_inputs_match_the_float64_reference(case, el):
    H, nqs, lks, causal = case
    x = inputs(H, nqs, lks, el, seed=7 * H + sum(lks))
    o, lse = run(*x, max(nqs), causal)
    check(o, lse, ref64(*x, causal), max(lks), el == torch.bfloat16, f"{case} {el}")


@ELS
@pytest.mark.parametrize("L", (1, 3, 65))
def test_one_visible_key_is_that_value_row_bit_for_bit(L, el):
    """the first token of a causal Nq = Lk call sees key 0 alone.  A seventh of the value elements each are large, subnormal and negative zero;
    the accumulator starts at +0 and 0 + 1 x (-0) is +0, so the expected bits are those of `row + 0.0`."""
    big, sub = (60000.0, 2.0 ** -20) if el == torch.half else (2.0 ** 100, 2.0 ** -130)
    q, kn, kpe, v, cu_q, cu_k = inputs(2, (L,), (L,), el, seed=11 + L)
    idx = torch.arange(L * 2 * 128).view(L, 2, 128) % 7
    for k, val in ((0, big), (1, sub), (2, -0.0)):
        v[PAD:PAD + L][idx == k] = val
    assert (v[PAD:PAD + L].contiguous().view(torch.int16)[idx == 2] == -32768).all() and (v[PAD:PAD + L][idx == 1].float() == sub).all()
    o, _ = run(q, kn, kpe, v, cu_q, cu_k, L, True)
    assert torch.equal(o[0].cpu().view(torch.int16), (v[PAD] + 0.0).contiguous().view(torch.int16))


@ELS
def test_a_chunk_composes_through_the_merge(el):
    """the last 70 of 200 tokens: over the 130 context keys (no mask) and over their own 70 keys (causal), merged by attn_merge_states, against
    the float64 attention over all 200 keys.  O: two 16-bit roundings in sequence, so twice the element type's rtol; lse: both derived bounds."""
    q, kn, kpe, v, cu_q, cu_k = inputs(2, (70,), (200,), el, seed=3)
    ctx, own = (torch.tensor(c, dtype=torch.int32) for c in ((PAD, PAD + 130), (PAD + 130, PAD + 200)))
    oa, la = run(q, kn, kpe, v, cu_q, ctx, 70, False)
    ob, lb = run(q, kn, kpe, v, cu_q, own, 70, True)
    o, lse = capi.attn_merge_states(oa, la, ob, lb, cu_q=cu_q.cuda())
    torch.cuda.synchronize()
    want = ref64(q, kn, kpe, v, cu_q, cu_k, True)
    o[70:], lse[70:] = O_CANARY, LSE_CANARY                                       # (the merge allocates: rows nobody owns are its business)
    bf16 = el == torch.bfloat16
    check(o, lse, want, 200, bf16, f"merge {el}", rtol=2 * (tol.ATTN_RTOL_BF16 if bf16 else tol.ATTN_RTOL_F16), lse_extra=sl.merge_lse_bound(want[1]))


@ELS
def test_a_captured_call_is_replayed_on_new_offsets(el):
    """captured on (3, 60) tokens; cu_q / cu_k are rewritten on the device to (64, 5) tokens over (70, 9) keys, max_nq 64 for both"""
    x = inputs(2, (64, 5), (70, 9), el, seed=5)
    cu_q, cu_k = torch.tensor([0, 3, 63], dtype=torch.int32).cuda(), torch.tensor([PAD, PAD + 10, PAD + 70], dtype=torch.int32).cuda()
    o = torch.full((x[0].shape[0], 2, 128), O_CANARY, dtype=el, device="cuda")
    lse = torch.full((x[0].shape[0], 2), LSE_CANARY, device="cuda")
    views, st, graph = device_views(*x[:4]), torch.cuda.Stream(), torch.cuda.CUDAGraph()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(*x[:4], cu_q, cu_k, 64, True)                                        # warm-up on buffers of its own
        with torch.cuda.graph(graph, stream=st):
            capi.attn_mla_prefill(*views, o, cu_q, cu_k, 64, SM_SCALE, lse=lse, causal=True)
    torch.cuda.synchronize()
    assert (o == O_CANARY).all()                                                 # captured, not run
    cu_q.copy_(x[4].cuda()), cu_k.copy_(x[5].cuda())
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    check(o, lse, ref64(*x, True), 70, el == torch.bfloat16, f"replay {el}")
