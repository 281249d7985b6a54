"""GPU tests of lc_attn_mla_paged_kv8 / _kv8_bf16 against float64 on the dequantised pool and against the 16-bit entry."""
import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import mla_lib as ml
from tests.decode_lib import forced_split
from tests.test_mla_gpu import CASES, ELS, LSE_CANARY, O_CANARY, check, cu_of, i32
from tests.test_mla_gpu import run as run16

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
SCALE = 0.0123                            # not a power of two: randn / SCALE stays inside +-448


# uint8 codes e4m3fn(clamp(x / scale, +-448)), the division in float32; their float64 values under the scale as the kernel holds it (float32)
quantise = lambda ckv, scale: (ckv.float() / np.float32(scale)).clamp(-448.0, 448.0).to(F8).view(torch.uint8)   # noqa: E731
dequant64 = lambda codes, scale: codes.view(F8).float().double() * float(np.float32(scale))                      # noqa: E731
scale_of = lambda s: None if s is None else torch.tensor([s], dtype=torch.float32, device="cuda")   # noqa: E731


def run(q_c, q_pe, codes, kpe, table, cu, lens, max_nq, causal, split, scale):
    o, lse = torch.full(q_c.shape, O_CANARY, dtype=q_c.dtype, device="cuda"), torch.full(q_c.shape[:2], LSE_CANARY, device="cuda")
    forced_split(split, lambda: capi.attn_mla_paged_kv8(q_c.cuda(), q_pe.cuda(), codes.cuda(), kpe.cuda(), o, i32(cu), table.cuda(), i32(lens), max_nq,
                                                        ml.SM_SCALE, ckv_scale=scale_of(scale), lse=lse, causal=causal))
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def inputs(case, el, scale):
    H, nqs, lens, page = case[:4]
    cu, T = cu_of(nqs), sum(nqs) + 4                      # four canary rows behind cu_q[B]
    g = torch.Generator().manual_seed(7 * H + sum(lens))
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
    ckv, kpe, table = ml.paged(lens, page, seed=H + page, el=el)
    return q_c, q_pe, quantise(ckv, scale), kpe, table, cu


@ELS
@pytest.mark.parametrize("case,scale", [(c, SCALE) for c in CASES] + [(CASES[1], None)],
                         ids=lambda x: f"H{x[0]}-L{'_'.join(map(str, x[2]))}-p{x[3]}-S{x[5]}" if isinstance(x, tuple) else f"scale{x}")
def test_random_inputs_match_the_float64_reference_on_the_dequantised_pool(case, scale, el):
    H, nqs, lens, page, causal, split = case
    q_c, q_pe, codes, kpe, table, cu = inputs(case, el, 1.0 if scale is None else scale)
    want = ml.ref64(q_c, q_pe, dequant64(codes, 1.0 if scale is None else scale), kpe, cu, table, lens, max(nqs), ml.SM_SCALE, causal)
    o, lse = run(q_c, q_pe, codes, kpe, table, cu, lens, max(nqs), causal, split, scale)
    check(o, lse, want, el == torch.bfloat16, cu[-1], max(lens), f"kv8 {case} scale {scale} {el}")
    assert max(lens) > 0 or ((o[:cu[-1]] == 0).all() and (lse[:cu[-1]] == -np.inf).all())


@ELS
@pytest.mark.parametrize("split", (1, 2))
@pytest.mark.parametrize("case", (CASES[2], CASES[0]), ids=("R80", "four-pages"))
def test_a_power_of_two_scale_gives_the_16_bit_entrys_bits(case, split, el):
    """scale 2^-5: code x scale is exact and normal in fp16 and bf16, and the scale passes the fp32 score chain and the epilogue without a rounding"""
    H, nqs, lens, page, causal, _ = case
    q_c, q_pe, codes, kpe, table, cu = inputs(case, el, 2.0 ** -5)
    ckv16 = (codes.view(F8).float() * 2.0 ** -5).to(el)
    o, lse = run(q_c, q_pe, codes, kpe, table, cu, lens, max(nqs), causal, split, 2.0 ** -5)
    o16, lse16 = run16(q_c, q_pe, ckv16, kpe, table, cu, lens, max(nqs), causal, split)
    assert torch.equal(o.view(torch.int16), o16.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse16.view(torch.int32))


@ELS
@pytest.mark.parametrize("split", (1, 2))
def test_one_visible_key_is_every_finite_code_times_the_scale_bit_for_bit(split, el):
    """kv_len = 1 for three sequences; the key's 512 bytes run through the 254 finite codes.  P = 1 and l = 1 exactly, so O is
    fl_el(fl32(code x scale)); the accumulator starts at +0, so the code 0x80 gives +0: `row + 0.0`"""
    H, T, lens = 16, 3, (1, 1, 1)
    finite = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=torch.uint8)
    g = torch.Generator().manual_seed(11)
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el), torch.randn(T, H, ml.DR, generator=g).to(el)
    ckv, kpe, table = ml.paged(lens, 16, seed=3, el=el)
    codes = quantise(ckv, SCALE)
    for b in range(T):
        codes[table[b, 0].long(), 0] = finite.roll(37 * b).repeat(3)[:ml.DC]
    o, _ = run(q_c, q_pe, codes, kpe, table, cu_of(lens), lens, 1, False, split, SCALE)
    for b in range(T):
        row = (codes[table[b, 0].long(), 0].view(F8).float() * torch.tensor(SCALE, dtype=torch.float32)).to(el) + 0.0
        assert torch.equal(o[b].view(torch.int16), row.expand(H, ml.DC).contiguous().view(torch.int16)), b


@ELS
def test_a_captured_split_step_is_replayed_on_new_lengths_and_a_new_scale(el):
    """captured with a caller workspace under S = 2; cu_q, kv_len, block_table and the scale change on the device before the one replay"""
    H, T, max_nq, page = 16, 7, 2, 16
    old, new = ((1, 1), (60, 30)), ((2, 1), (70, 31))
    g = torch.Generator().manual_seed(5)
    q_c, q_pe = torch.randn(T, H, ml.DC, generator=g).to(el).cuda(), torch.randn(T, H, ml.DR, generator=g).to(el).cuda()
    ckv, kpe, table_new = ml.paged(new[1], page, seed=9, el=el)
    codes = quantise(ckv, SCALE)
    table_old = table_new.clone()
    table_old[:, :2] = table_new[:, :2].flip(1)             # the same pages in another order: valid for the old lengths too
    cu_d, len_d, tab_d, scale_d, codes_d, kpe_d = i32(cu_of(old[0])), i32(old[1]), table_old.cuda(), scale_of(0.5), codes.cuda(), kpe.cuda()
    o, lse = torch.full(q_c.shape, O_CANARY, dtype=el, device="cuda"), torch.full((T, H), LSE_CANARY, device="cuda")
    capi.tune("attn_decode_split", 2)
    try:
        ws = torch.empty(capi.attn_mla_paged_workspace_bytes(2, H, T, max_nq, page, table_new.shape[1]), dtype=torch.uint8, device="cuda")
        def step(o_, lse_):
            capi.attn_mla_paged_kv8(q_c, q_pe, codes_d, kpe_d, o_, cu_d, tab_d, len_d, max_nq, ml.SM_SCALE, ckv_scale=scale_d, lse=lse_, causal=True,
                                    workspace=ws)
        st, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            step(torch.empty_like(o), torch.empty_like(lse))     # warm-up on buffers of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=st):
                step(o, lse)
        torch.cuda.synchronize()
        assert (o == O_CANARY).all()                             # captured, not run
        for dst, src in ((cu_d, i32(cu_of(new[0]))), (len_d, i32(new[1])), (tab_d, table_new.cuda()), (scale_d, scale_of(SCALE))):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
    finally:
        capi.tune("attn_decode_split", 0)
    want = ml.ref64(q_c.cpu(), q_pe.cpu(), dequant64(codes, SCALE), kpe, cu_of(new[0]), table_new, new[1], max_nq, ml.SM_SCALE, True)
    check(o.cpu(), lse.cpu(), want, el == torch.bfloat16, 3, max(new[1]), f"kv8 replay {el}")
