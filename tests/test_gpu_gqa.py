"""GPU tests of grouped-query attention (lc_attn_fwd_f16_gqa): Q, O [B,H,N,D] on K / V [B,Hkv,N,D]; query head h reads K / V head
h // (H // Hkv).  The truth is the EXISTING oracle on K / V expanded on the CPU (repeat_interleave along the head axis) under the bounds
of tests/tol.py (causal row i: the bound of i + 1 keys, as tests/test_gpu_causal.py); the stronger yardstick is bit-equality with the
MHA kernels on expanded K / V on every path the planner can pick — only an address differs.  tests/test_abi_cpu_gqa.py shows that a
wrong head map on these inputs misses the oracle bound by >= 20 x on every head it touches."""

import numpy as np
import pytest
import torch

from tests import tol
from tests.test_abi_cpu_gqa import expand_kv, gqa_inputs
from tests.test_gpu_causal import _check_dense, _check_rows, _rows

pytestmark = pytest.mark.gpu


def _capi():
    from leetcuda_amd import capi
    capi.load()
    return capi


def _inputs(B, H, Hkv, N, D, seed):
    return [x.cuda() for x in gqa_inputs(B, H, Hkv, N, D, seed)]


def _vin(v, vt):
    return v.transpose(-2, -1).contiguous() if vt else v


def _gqa(capi, q, k, v, vt=False, causal=False):
    """O of the GQA entry (NaN-prefilled); k, v are [B,Hkv,N,D] — v handed over as [B,Hkv,D,N] when vt"""
    o = torch.full_like(q, float("nan"))
    capi.attn_fwd_gqa(q, k, _vin(v, vt), o, v_transposed=vt, causal=causal)
    torch.cuda.synchronize()
    return o


def _mha(capi, q, k, v, vt=False, causal=False):
    """O of the EXISTING entries (lc_attn_fwd_f16 / _ex) on K / V expanded to H heads: the kernels of the parent commit"""
    G = q.shape[1] // k.shape[1]
    ke, ve = expand_kv(k, G).contiguous(), expand_kv(v, G).contiguous()
    o = torch.full_like(q, float("nan"))
    capi.attn_fwd(q, ke, _vin(ve, vt), o, v_transposed=vt, causal=causal)
    torch.cuda.synchronize()
    return o


def _names(capi, q, k, vt, causal):
    """(GQA kernel, MHA kernel) of a launch of this shape under the current knobs; the first is the second's `_gqa` twin"""
    B, H, N, D = q.shape
    mha = capi.attn_kernel_name(N, D, v_transposed=vt, bh=B * H, causal=causal)
    gqa = capi.attn_kernel_name(N, D, v_transposed=vt, bh=B * H, causal=causal, group=H // k.shape[1])
    assert mha.count("_kernel<") == 1 and gqa == mha.replace("_kernel<", "_gqa_kernel<"), (gqa, mha)
    return gqa, mha


def _want(N, D, vt, causal):
    """kernel family a (2 x {4, 6} heads, N, D) launch reaches on a device of >= 64 CUs"""
    if causal:
        return "attn_fwd_w4u_causal_gqa_kernel<" if D in (64, 128) and N % 256 == 0 else "attn_fwd_causal_gqa_kernel<"
    if D in (64, 128):      # small grids: split-KV, the 128-row lock-step kernel or the merged-phase kernel (tu_plan.hip choose_attn_nw)
        return ("attn_fwd_w4u_gqa_kernel<", "attn_fwd_gqa_kernel<") if N % 256 == 0 or N >= 1152 else ("attn_fwd_gqa_kernel<",)
    return "attn_fwd_w4i_gqa_kernel<" if not vt and N % 256 == 0 else "attn_fwd_gqa_kernel<"


def _check_dense_full(oracle, q, ke, ve, o):
    B, H, N, D = q.shape
    truth = oracle.attn(q, ke, ve, B, H, N, D, mode="f32")
    out = o.float().cpu().numpy()
    assert np.isfinite(out).all()
    ok, err, excess = tol.attn_close(out, truth, N)
    assert ok, (err, excess)


def _check_rows_full(oracle, q, ke, ve, o, rows):
    B, H, N, D = q.shape
    BH = B * H
    qc, kc, vc = (x.reshape(BH, N, D).cpu() for x in (q, ke, ve))
    out = o.reshape(BH, N, D).float().cpu().numpy()
    assert np.isfinite(out).all()
    truth = oracle.attn_rows(qc[:, rows].contiguous(), kc, vc, BH, len(rows), N, D)
    ok, err, excess = tol.attn_close(out[:, rows], truth, N)
    assert ok, (err, excess)


@pytest.mark.parametrize("heads", [(2, 6, 2), (2, 4, 1)], ids=["gqa_2x6on2", "mqa_2x4on1"])
@pytest.mark.parametrize("N", [64, 192, 256, 320, 1024, 1152, 4096])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_gqa_vs_oracle(oracle, D, vt, causal, N, heads):
    capi = _capi()
    B, H, Hkv = heads
    q, k, v = _inputs(B, H, Hkv, N, D, seed=D * 7919 + N * 4 + 2 * vt + causal + Hkv)
    gqa, _ = _names(capi, q, k, vt, causal)
    assert gqa.startswith(_want(N, D, vt, causal)), gqa
    o = _gqa(capi, q, k, v, vt, causal)
    ke, ve = expand_kv(k, H // Hkv).contiguous(), expand_kv(v, H // Hkv).contiguous()
    if N <= 1152:            # every row of every head
        if causal:
            _check_dense(oracle, q, ke, ve, o, gqa)
        else:
            _check_dense_full(oracle, q, ke, ve, o)
    elif causal:
        _check_rows(oracle, q, ke, ve, o, _rows(N))
    else:
        _check_rows_full(oracle, q, ke, ve, o, _rows(N))


class _knobs:
    def __init__(self, capi, **kv):
        self.capi, self.kv = capi, kv

    def __enter__(self):
        self.old = {k: self.capi.tune_get(k)[0] for k in self.kv}
        for k, val in self.kv.items():
            self.capi.tune(k, val)

    def __exit__(self, *a):
        for k, val in self.old.items():
            self.capi.tune(k, val)


def _bit_equal(capi, shape, vt, causal, want, seed=0, **knobs):
    """GQA == MHA on expanded K / V, bit for bit, under `knobs`; `want`: what the MHA kernel's name must start / end with"""
    B, H, Hkv, N, D = shape
    q, k, v = _inputs(B, H, Hkv, N, D, seed=seed + sum(shape) + 2 * vt + causal)
    with _knobs(capi, **knobs):
        gqa, mha = _names(capi, q, k, vt, causal)
        assert mha.startswith(want[0]) and mha.endswith(want[1]), (mha, want)
        a = _gqa(capi, q, k, v, vt, causal)
        b = _mha(capi, q, k, v, vt, causal)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), (gqa, float((a.float() - b.float()).abs().max()))
    return a


@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("nw,walk", [(513, 0), (515, 1), (517, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_bits_of_the_merged_phase_walks(D, nw, walk, vt):
    """(2, 12, 4, 4096): 384 query blocks, more than the CUs of the device — the persistent walks really walk, and the heads of a
    group (G = 3, not a power of two) and of two groups meet inside one workgroup's walk"""
    capi = _capi()
    assert 2 * 12 * (4096 // 256) > torch.cuda.get_device_properties(0).multi_processor_count
    _bit_equal(capi, (2, 12, 4, 4096, D), vt, False, (f"attn_fwd_w4u_kernel<{D},", f",{walk}>"), attn_nw=nw)


@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("split", [2, 4, 0])
@pytest.mark.parametrize("D", [64, 128])
def test_bits_of_split_kv(D, split, vt):
    capi = _capi()
    # (auto: the rule reasons as on a 256-CU device with the built-in constants, as tests/test_gpu_attn.py SPLIT_SHAPES)
    _bit_equal(capi, (1, 8, 2, 2048, D), vt, False, (f"attn_fwd_w4u_kernel<{D},", ",3>"), attn_split=split, rule_cus=256, attn_calib=1)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("nw", [8, 4, 2])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_bits_of_the_lockstep_kernels(D, nw, vt, causal):
    capi = _capi()
    v = "true" if vt else "false"
    want = (f"attn_fwd_causal_kernel<{D},{nw},{v}>", "") if causal else (f"attn_fwd_kernel<{D},{nw},{v},0>", "")
    _bit_equal(capi, (2, 6, 2, 1024, D), vt, causal, want, attn_nw=nw)


@pytest.mark.parametrize("D,nw", [(32, 0), (96, 0), (64, 514), (128, 514)])
@pytest.mark.parametrize("sched", [0, 1])
def test_bits_of_the_generated_kernel(D, nw, sched):
    capi = _capi()
    _bit_equal(capi, (2, 6, 2, 1024, D), False, False, (f"attn_fwd_w4i_kernel<{D},{sched}>", ""), attn_nw=nw, attn_w4i_sched=sched)
    _bit_equal(capi, (2, 9, 3, 2048, D), False, False, (f"attn_fwd_w4i_kernel<{D},{sched}>", ""), seed=3, attn_nw=nw, attn_w4i_sched=sched)


@pytest.mark.parametrize("order", [1, 2], ids=["longest_first", "head_major"])
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_bits_of_the_causal_kernels_under_both_grid_orders(D, vt, order):
    capi = _capi()
    v = "true" if vt else "false"
    want = f"attn_fwd_w4u_causal_kernel<{D},{v}>" if D in (64, 128) else f"attn_fwd_causal_kernel<{D},8,{v}>"
    a = _bit_equal(capi, (2, 12, 4, 2048, D), vt, True, (want, ""), attn_causal_order=order)
    b = _bit_equal(capi, (2, 12, 4, 2048, D), vt, True, (want, ""))       # auto
    assert torch.equal(a, b)


def _in_front_of_nan(x, factor):
    """x at the front of an allocation `factor` times its size whose remainder is NaN (what a kernel that indexed K / V by the query head
    would read)"""
    buf = torch.full((x.numel() * factor,), float("nan"), dtype=x.dtype, device=x.device)
    buf[:x.numel()] = x.reshape(-1)
    return buf[:x.numel()].view(x.shape), buf


GUARDED = [  # (shape, vt, causal, knobs)
    ((2, 12, 4, 4096, 128), False, False, dict(attn_nw=515)),      # static persistent walk, 384 blocks: the last block of every workgroup has no next block
    ((2, 12, 4, 4096, 64), True, False, dict(attn_nw=517)),        # dynamic queue
    ((2, 12, 4, 4096, 128), True, False, dict(attn_nw=513)),
    ((1, 8, 2, 2048, 128), False, False, dict(attn_split=4)),
    ((2, 12, 4, 2048, 64), False, True, dict(attn_causal_order=1)),
    ((2, 12, 4, 2048, 128), True, True, dict(attn_causal_order=2)),
    ((2, 6, 2, 1024, 96), False, False, dict()),                   # the generated kernel
    ((2, 6, 2, 320, 32), True, False, dict()),                     # lock-step
    ((2, 4, 1, 1152, 96), True, True, dict()),                     # lock-step causal, multi-query
]


@pytest.mark.parametrize("case", GUARDED, ids=[f"{'x'.join(map(str, c[0]))}-{'dn' if c[1] else 'nd'}-{'causal' if c[2] else 'full'}" for c in GUARDED])
def test_no_read_outside_the_kv_tensors(case):
    """K and V (the last K / V head of the last batch included) end where an allocation G times as large goes on with NaN: a read behind
    [B,Hkv,N,D] — the base of a query-head index, a next-block prefetch past the last head — would reach O.  O stays finite and is the
    bits of the MHA kernel on expanded K / V."""
    capi = _capi()
    shape, vt, causal, knobs = case
    B, H, Hkv, N, D = shape
    q, k, v = _inputs(B, H, Hkv, N, D, seed=17 + sum(shape))
    with _knobs(capi, **knobs):
        ref = _mha(capi, q, k, v, vt, causal)
        kg, kbuf = _in_front_of_nan(k, H // Hkv)
        vg, vbuf = _in_front_of_nan(_vin(v, vt), H // Hkv)
        assert torch.isnan(kbuf[k.numel():]).all() and torch.isnan(vbuf[v.numel():]).all()
        o = torch.full_like(q, float("nan"))
        capi.attn_fwd_gqa(q, kg, vg, o, v_transposed=vt, causal=causal)
        torch.cuda.synchronize()
    assert torch.isfinite(o).all()
    assert torch.equal(o, ref)


@pytest.mark.parametrize("D,N,causal", [(128, 1024, False), (96, 512, True), (256, 512, False)])
def test_equal_head_counts_are_the_ex_entry(D, N, causal):
    capi = _capi()
    B, H = 2, 3
    q, k, v = _inputs(B, H, H, N, D, seed=D + N)
    assert capi.attn_kernel_name(N, D, bh=B * H, causal=causal, group=1) == capi.attn_kernel_name(N, D, bh=B * H, causal=causal)
    a = _gqa(capi, q, k, v, False, causal)
    b = torch.full_like(q, float("nan"))
    rc = capi.load().lc_attn_fwd_f16_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), b.data_ptr(), B, H, N, D,
                                        capi.ATTN_CAUSAL if causal else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == capi.LC_OK
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_graph_capture_replays_the_eager_bits(oracle):
    capi = _capi()
    # causal: one kernel, no workspace — the replay is the eager launch
    for D, N in ((128, 1024), (96, 512)):
        q, k, v = _inputs(2, 6, 2, N, D, seed=77 + D)
        eager = _gqa(capi, q, k, v, causal=True)
        assert torch.equal(eager, _mha(capi, q, k, v, causal=True))
        o = torch.full_like(q, float("nan"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            capi.attn_fwd_gqa(q, k, v, o, causal=True)
        o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager), D
    # non-causal on a split-KV shape: the captured launch falls back to the one-block walk (ONE kernel node, no workspace), as the MHA call
    B, H, Hkv, N, D = 1, 4, 2, 1024, 128
    q, k, v = _inputs(B, H, Hkv, N, D, seed=78)
    with _knobs(capi, rule_cus=256, attn_calib=1):
        assert capi.attn_kernel_name(N, D, bh=B * H, group=2) == "attn_fwd_w4u_gqa_kernel<128,false,3>"
        split = _gqa(capi, q, k, v)
        with _knobs(capi, attn_split=1):          # what the capture falls back to (also warms that kernel up outside the capture)
            unsplit = _gqa(capi, q, k, v)
            assert torch.equal(unsplit, _mha(capi, q, k, v))
        o = torch.full_like(q, float("nan"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            capi.attn_fwd_gqa(q, k, v, o)
        o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(o, unsplit)
    assert float((o.float() - split.float()).abs().max()) <= 2.0 ** -9 * float(v.float().abs().max())
    _check_dense_full(oracle, q, expand_kv(k, 2).contiguous(), expand_kv(v, 2).contiguous(), o)


def test_non_default_stream():
    capi = _capi()
    for causal in (False, True):
        q, k, v = _inputs(2, 6, 3, 2048, 128, seed=99 + causal)
        ref = _gqa(capi, q, k, v, causal=causal)
        s = torch.cuda.Stream()
        o = torch.full_like(q, float("nan"))
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            capi.attn_fwd_gqa(q, k, v, o, causal=causal)
        s.synchronize()
        assert torch.equal(o, ref)


@pytest.mark.parametrize("shape,causal", [((2, 32, 8, 4096, 128), True), ((1, 64, 8, 8192, 128), False), ((1, 16, 1, 4096, 64), False),
                                          ((1, 16, 1, 4096, 64), True)],
                         ids=["llama_2x32on8_causal", "llama_1x64on8_8k", "mqa_1x16on1", "mqa_1x16on1_causal"])
def test_model_sized(oracle, shape, causal):
    capi = _capi()
    B, H, Hkv, N, D = shape
    G = H // Hkv
    q, k, v = _inputs(B, H, Hkv, N, D, seed=sum(shape))
    gqa, _ = _names(capi, q, k, False, causal)
    assert gqa.startswith("attn_fwd_w4u_causal_gqa_kernel<" if causal else "attn_fwd_w4u_gqa_kernel<"), gqa
    o = _gqa(capi, q, k, v, causal=causal)
    heads = sorted(h for h in {0, G - 1, G, H - G - 1, H - 1, B * H - 1, B * H - G, (B - 1) * H} if 0 <= h < B * H)   # group seams, the last group, the last batch
    qs = q.reshape(1, B * H, N, D)[:, heads].contiguous()
    ks, vs = (expand_kv(x, G).reshape(1, B * H, N, D)[:, heads].contiguous() for x in (k, v))
    os_ = o.reshape(1, B * H, N, D)[:, heads].contiguous()
    if causal:
        _check_rows(oracle, qs, ks, vs, os_, _rows(N) + [N // 2 - 1, N // 2])
    else:
        _check_rows_full(oracle, qs, ks, vs, os_, _rows(N) + [N // 2 - 1, N // 2])
    # V = const per K / V head  =>  O = that constant on every row of the heads of its group (softmax weights sum to one)
    c = ((torch.arange(B * Hkv, device="cuda") % 7 - 3).float() / 4).half().view(B, Hkv, 1, 1)      # -0.75 .. 0.75, neighbours differ
    oc = _gqa(capi, q, k, c.expand(B, Hkv, N, D).contiguous(), causal=causal)
    assert (oc.float() - expand_kv(c, G).float()).abs().max().item() < 1e-3


@pytest.mark.parametrize("D,causal", [(128, True), (64, True), (128, False), (64, False), (96, False)])
def test_slow_path_counters_of_the_gqa_units_are_summed_and_reset(D, causal):
    """lc_attn_slowpath_stats covers the grouped-query units: on the inputs of tests/test_gpu_causal.py
    test_overflow_slow_path_under_the_mask (scores that grow along the key index) the `_gqa` twin counts what the MHA kernel counts on
    expanded K / V — the same body on the same values —, and a read with reset leaves nothing behind.  D = 64 / 128: the merged-phase
    units (tu_attn_w4u_gqa_*.hip); D = 96: the generated kernel's (tu_attn_w4i_gqa.hip)."""
    capi = _capi()
    B, H, Hkv, N = 1, 4, 2, 1024
    torch.manual_seed(1234 + D)
    q = torch.full((B, H, N, D), 4.0 / D ** 0.5, dtype=torch.half, device="cuda")
    ramp = (4.0 * torch.arange(N, device="cuda", dtype=torch.float32) / N).half()
    k = ramp.view(1, 1, N, 1).expand(B, Hkv, N, D).contiguous()
    v = torch.randn(B, Hkv, N, D, dtype=torch.half, device="cuda")
    with _knobs(capi, rule_cus=256, attn_calib=1):      # (the split rule as on a 256-CU device with the built-in constants: no lock-step kernel here)
        gqa, _ = _names(capi, q, k, False, causal)
        assert "_gqa_kernel<" in gqa and gqa.startswith("attn_fwd_w4i_gqa" if D == 96 else "attn_fwd_w4u_"), gqa
        capi.attn_slowpath_stats(reset=True)
        _mha(capi, q, k, v, causal=causal)
        m = capi.attn_slowpath_stats(reset=True)
        _gqa(capi, q, k, v, causal=causal)
        g = capi.attn_slowpath_stats(reset=True)
        z = capi.attn_slowpath_stats(reset=False)
    assert g[:3] == m[:3], (g, m)
    if causal:
        assert g[0] > 0, g
    assert z[:3] == [0, 0, 0], z
