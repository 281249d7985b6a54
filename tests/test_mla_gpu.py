"""GPU tests of lc_attn_mla_paged_f16 / _bf16 against the float64 reference of tests/mla_lib.py."""
import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import lse_lib as sl
from tests import mla_lib as ml
from tests import tol
from tests.decode_lib import forced_split

pytestmark = pytest.mark.gpu
ELS = pytest.mark.parametrize("el", (torch.half, torch.bfloat16), ids=("f16", "bf16"))
O_CANARY, LSE_CANARY = 768.0, -4321.5     # exact in fp16 and bf16; a value no log-sum-exp here reaches


i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device="cuda")   # noqa: E731
cu_of = lambda nqs: [0] + np.cumsum(nqs).tolist()                         # noqa: E731


def run(q_c, q_pe, ckv, kpe, table, cu, lens, max_nq, causal, split, workspace=None):
    o = torch.full(q_c.shape, O_CANARY, dtype=q_c.dtype, device="cuda")
    lse = torch.full(q_c.shape[:2], LSE_CANARY, device="cuda")
    forced_split(split, lambda: capi.attn_mla_paged(q_c.cuda(), q_pe.cuda(), ckv.cuda(), kpe.cuda(), o, i32(cu), table.cuda(), i32(lens), max_nq,
                                                    ml.SM_SCALE, lse=lse, causal=causal, workspace=workspace))
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def check(o, lse, want, bf16, n_own, N, what):
    """owned rows under the project's bounds (tol.attn_close at N = max kv_len, lse_lib.lse_bound at D = 576), the rows behind them intact"""
    want_o, want_lse, A, nvis = want
    assert (o[n_own:] == O_CANARY).all() and (lse[n_own:] == LSE_CANARY).all(), (what, "rows nobody owns were written")
    got = o[:n_own].float().numpy()
    ok, mx, _ = tol.attn_close(got, want_o[:n_own], N, bf16=bf16)
    bound = tol.attn_max_abs(N, bf16) + (tol.ATTN_RTOL_BF16 if bf16 else tol.ATTN_RTOL_F16) * np.abs(want_o[:n_own])
    ro = float((np.abs(got - want_o[:n_own]) / bound).max())
    rl = sl.check_lse(lse.numpy(), want_lse, A, nvis, ml.DC + ml.DR, what=what)
    print(f"{what}: O max |err| {mx:.3e}, worst err / bound {ro:.3f}; lse worst err / bound {rl:.3f}")
    assert ok, (what, mx, ro)


# H, Nq_b per sequence, kv_len per sequence, page, causal, forced S
CASES = [
    (16, (1, 1, 1), (1, 64, 65), 16, False, 1),     # one live wave; one key; a full tile; one key into the second tile; a tile over four pages
    (5, (3, 0, 2), (3, 7, 130), 16, True, 1),       # R = 15, 10: no multiples of 16; an empty sequence; L = Nq; a third tile with 2 keys
    (16, (5,), (300,), 32, True, 2),                # R = 80: the second row block has 16 rows; the causal limit differs per block
    (128, (1, 2), (200, 67), 64, True, 3),          # RB = 2 and 4; L = 67: two tiles over three ranges, one of them empty
    (128, (1,), (0,), 64, False, 1),                # no key: O = 0 and lse = -inf on every row
]


@ELS
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"H{c[0]}-L{'_'.join(map(str, c[2]))}-p{c[3]}-S{c[5]}")
def test_random_inputs_match_the_float64_reference(case, el):
    H, nqs, lens, page, causal, split = case
    cu, T = cu_of(nqs), sum(nqs) + 4
    g = torch.Generator().manual_seed(7 * H + sum(lens))
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
    ckv, kpe, table = ml.paged(lens, page, seed=H + page, el=el)
    want = ml.ref64(q_c, q_pe, ckv, kpe, cu, table, lens, max(nqs), ml.SM_SCALE, causal)
    o, lse = run(q_c, q_pe, ckv, kpe, table, cu, lens, max(nqs), causal, split)
    check(o, lse, want, el == torch.bfloat16, cu[-1], max(lens), f"{case} {el}")
    if max(lens) == 0:
        assert (o[:cu[-1]] == 0).all() and (lse[:cu[-1]] == -np.inf).all()


@ELS
@pytest.mark.parametrize("split", (1, 2))
def test_one_visible_key_is_that_keys_latent_row_bit_for_bit(split, el):
    """kv_len = 1 for three sequences, and the first token of a causal chunk with L = Nq = 3.  A seventh of the latent elements each are large,
    subnormal and negative zero; the accumulator starts at +0 and 0 + 1 x (-0) is +0, so the expected bits are those of `row + 0.0`."""
    H = 16
    big, sub = (60000.0, 2.0 ** -20) if el == torch.half else (2.0 ** 100, 2.0 ** -130)
    for nqs, lens, causal in (((1, 1, 1), (1, 1, 1), False), ((3,), (3,), True)):
        cu, T = cu_of(nqs), sum(nqs)
        g = torch.Generator().manual_seed(11 + T)
        q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
        ckv, kpe, table = ml.paged(lens, 16, seed=3, el=el)
        idx = torch.arange(ckv.numel()).view(ckv.shape) % 7
        for k, v in ((0, big), (1, sub), (2, -0.0)):
            ckv[idx == k] = v
        assert (ckv.view(torch.int16)[idx == 2] == -32768).all() and (ckv[idx == 1].float() == sub).all()
        o, _ = run(q_c, q_pe, ckv, kpe, table, cu, lens, max(nqs), causal, split)
        for b in range(len(lens)):
            row = ckv[table[b, 0].long(), 0] + 0.0
            assert torch.equal(o[cu[b]].view(torch.int16), row.expand(H, ml.DC).contiguous().view(torch.int16)), (nqs, b)


@ELS
def test_a_captured_split_step_is_replayed_on_new_lengths(el):
    """captured with a caller workspace under S = 2; cu_q, kv_len and block_table change on the device (Nq_b 1, 1 -> 2, 1, a tile boundary crossed)"""
    H, T, max_nq, page = 16, 7, 2, 16
    old, new = ((1, 1), (60, 30)), ((2, 1), (70, 31))
    g = torch.Generator().manual_seed(5)
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el).cuda(), torch.randn(T, H, ml.DR, generator=g).to(el).cuda()
    ckv, kpe, table_new = ml.paged(new[1], page, seed=9, el=el)
    table_old = table_new.clone()
    table_old[:, :2] = table_new[:, :2].flip(1)             # the same pages in another order: valid for the old lengths too
    cu_d, len_d, tab_d = i32(cu_of(old[0])), i32(old[1]), table_old.cuda()
    ckv_d, kpe_d = ckv.cuda(), kpe.cuda()
    o = torch.full(q_c.shape, O_CANARY, dtype=el, device="cuda")
    lse = torch.full((T, H), LSE_CANARY, device="cuda")
    capi.tune("attn_decode_split", 2)
    try:
        ws = torch.empty(capi.attn_mla_paged_workspace_bytes(2, H, T, max_nq, page, table_new.shape[1]), dtype=torch.uint8, device="cuda")
        def step(o_, lse_):
            capi.attn_mla_paged(q_c, q_pe, ckv_d, kpe_d, o_, cu_d, tab_d, len_d, max_nq, ml.SM_SCALE, lse=lse_, causal=True, workspace=ws)
        st, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            step(torch.empty_like(o), torch.empty_like(lse))     # warm-up on buffers of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step(o, lse)
        torch.cuda.synchronize()
        assert (o == O_CANARY).all()                             # captured, not run
        cu_d.copy_(i32(cu_of(new[0])))
        len_d.copy_(i32(new[1]))
        tab_d.copy_(table_new.cuda())
        graph.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    want = ml.ref64(q_c.cpu(), q_pe.cpu(), ckv, kpe, cu_of(new[0]), table_new, new[1], max_nq, ml.SM_SCALE, True)
    check(o.cpu(), lse.cpu(), want, el == torch.bfloat16, 3, max(new[1]), f"replay {el}")
