"""GPU tests of lc_attn_mla_sparse_kv8 / _kv8_bf16 against float64 on the dequantised pool and against the 16-bit entry.
`inputs` fills every pool slot no row selects with NaN, which `quantise` turns into code 0x7f: an invalid or unselected entry that reached a
product would show."""
import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import mla_lib as ml
from tests.decode_lib import forced_split
from tests.test_mla_kv8_gpu import F8, SCALE, dequant64, quantise, scale_of
from tests.test_mla_sparse_gpu import CASES, ELS, LSE_CANARY, NSLOTS, O_CANARY, check, inputs, ref64
from tests.test_mla_sparse_gpu import run as run16

pytestmark = pytest.mark.gpu


def run(q_c, q_pe, codes, kpe, slots, split, scale):
    o = torch.full(q_c.shape, O_CANARY, dtype=q_c.dtype, device="cuda")
    lse = torch.full(q_c.shape[:2], LSE_CANARY, device="cuda")
    forced_split(split, lambda: capi.attn_mla_sparse_kv8(q_c.cuda(), q_pe.cuda(), codes.cuda(), kpe.cuda(), o, slots.cuda(), ml.SM_SCALE,
                                                         ckv_scale=scale_of(scale), lse=lse))
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


@ELS
@pytest.mark.parametrize("case,scale", [(c, SCALE) for c in CASES] + [(CASES[2], None)],
                         ids=lambda x: f"H{x[0]}-T{x[1]}-k{x[2]}-S{x[3]}" if isinstance(x, tuple) else f"scale{x}")
def test_random_inputs_match_the_float64_reference_on_the_dequantised_pool(case, scale, el):
    H, T, topk, split, kind = case
    q_c, q_pe, ckv, kpe, slots = inputs(H, T, topk, el, seed=7 * H + topk, **kind)
    codes = quantise(ckv, 1.0 if scale is None else scale)
    assert (codes[ckv.isnan()] == 0x7f).all()
    o, lse = run(q_c, q_pe, codes, kpe, slots, split, scale)
    want = ref64(q_c, q_pe, dequant64(codes, 1.0 if scale is None else scale), kpe, slots, ml.SM_SCALE)
    check(o, lse, want, el == torch.bfloat16, f"kv8 {case} scale {scale} {el}")
    assert (lse[want[3] == 0] == -np.inf).all()


@ELS
@pytest.mark.parametrize("case", (CASES[2], CASES[4]), ids=("holes", "RB2-S3"))
def test_a_power_of_two_scale_gives_the_16_bit_entrys_bits(case, el):
    """scale 2^-5: code x scale is exact and normal in fp16 and bf16, and the scale passes the fp32 score chain and the epilogue without a rounding"""
    H, T, topk, split, kind = case
    q_c, q_pe, ckv, kpe, slots = inputs(H, T, topk, el, seed=7 * H + topk, **kind)
    codes = quantise(ckv, 2.0 ** -5)
    o, lse = run(q_c, q_pe, codes, kpe, slots, split, 2.0 ** -5)
    o16, lse16 = run16(q_c, q_pe, (codes.view(F8).float() * 2.0 ** -5).to(el), kpe, slots, split)
    assert torch.equal(o.view(torch.int16), o16.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse16.view(torch.int32))


@ELS
@pytest.mark.parametrize("split", (1, 2))
def test_one_valid_entry_is_every_finite_code_times_the_scale_bit_for_bit(split, el):
    """the one valid entry of a topk = 130 row sits at position 0, 63, 64 and 129, a token each; its 512 bytes run through the 254 finite codes
    and every other slot of the pools is NaN.  P = 1 and l = 1 exactly, so O is fl_el(fl32(code x scale)); the accumulator starts at +0, so
    the code 0x80 gives +0: `row + 0.0`"""
    H, topk, at = 16, 130, (0, 63, 64, 129)
    finite = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=torch.uint8)
    q_c, q_pe, _, kpe, _ = inputs(H, len(at), topk, el, seed=11)
    codes = torch.full((NSLOTS, ml.DC), 0x7f, dtype=torch.uint8)
    kpe[:] = float("nan")
    slots = torch.full((len(at), topk), -1, dtype=torch.int32)
    for t, j in enumerate(at):
        slots[t, j] = 17 + 71 * t
        codes[17 + 71 * t] = finite.roll(37 * t).repeat(3)[:ml.DC]
        kpe[17 + 71 * t] = 0.5
    o, _ = run(q_c, q_pe, codes, kpe, slots, split, SCALE)
    for t in range(len(at)):
        row = (codes[17 + 71 * t].view(F8).float() * torch.tensor(SCALE, dtype=torch.float32)).to(el) + 0.0
        assert torch.equal(o[t].view(torch.int16), row.expand(H, ml.DC).contiguous().view(torch.int16)), (at[t], split)


@ELS
def test_a_captured_step_is_replayed_on_new_slots_and_a_new_scale(el):
    """captured with a caller workspace under S = 2; slots and the scale are rewritten on the device before the one replay"""
    H, T, topk = 16, 4, 130
    q_c, q_pe, ckv, kpe, old = inputs(H, T, topk, el, seed=5)
    codes = quantise(ckv, SCALE)
    new = old.roll(1, 0).flip(1).contiguous()            # the selected set of slots stays: the NaN slots stay unselected
    old[:, 1::3], new[:, ::4], new[3] = -1, -1, -1
    q_d, qpe_d, codes_d, kpe_d, slots_d, scale_d = (x.cuda() for x in (q_c, q_pe, codes, kpe, old, scale_of(0.5)))
    o = torch.full(q_c.shape, O_CANARY, dtype=el, device="cuda")
    lse = torch.full((T, H), LSE_CANARY, device="cuda")
    capi.tune("attn_decode_split", 2)
    try:
        ws = torch.empty(capi.attn_mla_sparse_workspace_bytes(T, H, topk), dtype=torch.uint8, device="cuda")
        def step(o_, lse_):
            capi.attn_mla_sparse_kv8(q_d, qpe_d, codes_d, kpe_d, o_, slots_d, ml.SM_SCALE, ckv_scale=scale_d, lse=lse_, workspace=ws)
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
        scale_d.copy_(scale_of(SCALE))
        graph.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    check(o.cpu(), lse.cpu(), ref64(q_c, q_pe, dequant64(codes, SCALE), kpe, new, ml.SM_SCALE), el == torch.bfloat16, f"kv8 replay {el}")
