"""GPU tests of lc_attn_mla_sparse_f16 / _bf16 against a float64 reference: the valid entries of a row gathered from the
pools, then softmax, lse and P @ CKV."""
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
NSLOTS = 331                              # slot 0 and slot 330 are never selected


def ref64(q_c, q_pe, ckv, kpe, slots, sm_scale):
    """(O [T,H,512], lse [T,H], A [T,H], nvis [T]) in float64; A = max over the row's keys of sm_scale sum_d |q_d k_d| (lse_lib.lse_bound)"""
    T, H, _ = q_c.shape
    O, lse, A, nvis = np.zeros((T, H, ml.DC)), np.full((T, H), -np.inf), np.zeros((T, H)), np.zeros(T, int)
    q, kv = torch.cat([q_c, q_pe], -1).double(), torch.cat([ckv, kpe], -1)
    for t in range(T):
        idx = slots[t][(slots[t] >= 0) & (slots[t] < ckv.shape[0])].long()
        nvis[t] = len(idx)
        if len(idx):
            prod = q[t][:, None, :] * kv[idx].double()[None]
            s = prod.sum(-1) * sm_scale
            A[t] = (prod.abs().sum(-1) * sm_scale).max(-1).values.numpy()
            lse[t] = torch.logsumexp(s, -1).numpy()
            O[t] = (torch.softmax(s, -1) @ kv[idx, :ml.DC].double()).numpy()
    return O, lse, A, nvis


def inputs(H, T, topk, el, seed, holes=False, gap=False):
    """q_c, q_pe, flat randn pools and slots [T,topk] drawn per token without replacement from slots 1 .. NSLOTS - 2; every pool slot no row
    selects is NaN.  holes: every third entry invalid (-1, NSLOTS, 2^31 - 1 in turn), token 1 all invalid, token 2 with a slot listed twice;
    gap: entries 64 .. 127 of token 0 invalid"""
    g = torch.Generator().manual_seed(seed)
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
    ckv, kpe = torch.randn(NSLOTS, ml.DC, generator=g).to(el), torch.randn(NSLOTS, ml.DR, generator=g).to(el)
    slots = torch.stack([1 + torch.randperm(NSLOTS - 2, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    if holes:
        slots[:, ::3] = torch.tensor([-1, NSLOTS, 2 ** 31 - 1], dtype=torch.int32).repeat(topk)[:len(range(0, topk, 3))]
        slots[1] = -1
        slots[2, 5] = slots[2, 40]
    if gap:
        slots[0, 64:128] = -1
    unused = torch.ones(NSLOTS, dtype=torch.bool)
    unused[slots[(slots >= 0) & (slots < NSLOTS)].long()] = False
    assert unused[0] and unused[-1]
    ckv[unused], kpe[unused] = float("nan"), float("nan")
    return q_c, q_pe, ckv, kpe, slots


def check(o, lse, want, bf16, what):
    want_o, want_lse, A, nvis = want
    got = o.float().numpy()
    ok, mx, _ = tol.attn_close(got, want_o, int(nvis.max()), bf16=bf16)
    rl = sl.check_lse(lse.numpy(), want_lse, A, nvis, ml.DC + ml.DR, what=what)
    print(f"{what}: O max |err| {mx:.3e}; lse worst err / bound {rl:.3f}")
    assert ok, (what, mx)
    assert (got[nvis == 0] == 0).all()


def run(q_c, q_pe, ckv, kpe, slots, split):
    o = torch.full(q_c.shape, O_CANARY, dtype=q_c.dtype, device="cuda")
    lse = torch.full(q_c.shape[:2], LSE_CANARY, device="cuda")
    forced_split(split, lambda: capi.attn_mla_sparse(q_c.cuda(), q_pe.cuda(), ckv.cuda(), kpe.cuda(), o, slots.cuda(), ml.SM_SCALE, lse=lse))
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


# H, T, topk, forced S, what the slots hold
CASES = [
    (16, 3, 1, 1, {}),                     # one key
    (16, 3, 65, 1, {}),                    # one entry into a second tile; the tokens select different slots
    (5, 4, 70, 1, dict(holes=True)),       # H no multiple of 16; invalid entries between valid ones; a token without a key; a duplicate
    (80, 2, 130, 2, {}),                   # the second row block has 16 rows
    (128, 2, 67, 3, {}),                   # RB = 2; two tiles over three ranges: one range is empty
    (16, 2, 192, 1, dict(gap=True)),       # the middle tile of token 0 is entirely invalid
]


@ELS
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"H{c[0]}-T{c[1]}-k{c[2]}-S{c[3]}")
def test_random_inputs_match_the_float64_reference(case, el):
    H, T, topk, split, kind = case
    q_c, q_pe, ckv, kpe, slots = inputs(H, T, topk, el, seed=7 * H + topk, **kind)
    o, lse = run(q_c, q_pe, ckv, kpe, slots, split)
    check(o, lse, ref64(q_c, q_pe, ckv, kpe, slots, ml.SM_SCALE), el == torch.bfloat16, f"{case} {el}")


@ELS
@pytest.mark.parametrize("split", (1, 2))
def test_one_valid_entry_is_that_slots_latent_row_bit_for_bit(split, el):
    """the one valid entry of a topk = 130 row sits at position 0, 63, 64 and 129, a token each.  A seventh of the latent elements each are
    large, subnormal and negative zero; the accumulator starts at +0 and 0 + 1 x (-0) is +0, so the expected bits are those of `row + 0.0`."""
    H, topk, at = 16, 130, (0, 63, 64, 129)
    big, sub = (60000.0, 2.0 ** -20) if el == torch.half else (2.0 ** 100, 2.0 ** -130)
    q_c, q_pe, ckv, kpe, _ = inputs(H, len(at), topk, el, seed=11)
    ckv.masked_fill_(ckv.isnan(), 0.5), kpe.masked_fill_(kpe.isnan(), 0.5)
    idx = torch.arange(ckv.numel()).view(ckv.shape) % 7
    for k, v in ((0, big), (1, sub), (2, -0.0)):
        ckv[idx == k] = v
    assert (ckv.view(torch.int16)[idx == 2] == -32768).all() and (ckv[idx == 1].float() == sub).all()
    slots = torch.full((len(at), topk), -1, dtype=torch.int32)
    for t, j in enumerate(at):
        slots[t, j] = 17 + 71 * t
    o, _ = run(q_c, q_pe, ckv, kpe, slots, split)
    for t in range(len(at)):
        row = ckv[17 + 71 * t] + 0.0
        assert torch.equal(o[t].view(torch.int16), row.expand(H, ml.DC).contiguous().view(torch.int16)), (at[t], split)


@ELS
def test_a_captured_step_is_replayed_on_new_slots(el):
    """captured with a caller workspace under S = 2; slots is rewritten on the device: other slots, other positions of the invalid entries"""
    H, T, topk = 16, 4, 130
    q_c, q_pe, ckv, kpe, old = inputs(H, T, topk, el, seed=5)
    new = old.roll(1, 0).flip(1).contiguous()            # the selected set of slots stays: the NaN slots stay unselected
    old[:, 1::3], new[:, ::4], new[3] = -1, -1, -1
    q_d, qpe_d, ckv_d, kpe_d, slots_d = (x.cuda() for x in (q_c, q_pe, ckv, kpe, old))
    o = torch.full(q_c.shape, O_CANARY, dtype=el, device="cuda")
    lse = torch.full((T, H), LSE_CANARY, device="cuda")
    capi.tune("attn_decode_split", 2)
    try:
        ws = torch.empty(capi.attn_mla_sparse_workspace_bytes(T, H, topk), dtype=torch.uint8, device="cuda")
        def step(o_, lse_):
            capi.attn_mla_sparse(q_d, qpe_d, ckv_d, kpe_d, o_, slots_d, ml.SM_SCALE, lse=lse_, workspace=ws)
        st, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            step(torch.empty_like(o), torch.empty_like(lse))     # warm-up on buffers of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step(o, lse)
        torch.cuda.synchronize()
        assert ws.numel() > 0 and (o == O_CANARY).all()          # captured, not run
        slots_d.copy_(new.cuda())
        graph.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    check(o.cpu(), lse.cpu(), ref64(q_c, q_pe, ckv, kpe, new, ml.SM_SCALE), el == torch.bfloat16, f"replay {el}")
