"""CPU tests of grouped-query attention's boundary (lc_attn_fwd_f16_gqa, lc_attn_kernel_name_gqa; neither name call launches): the plan of
a GQA call is the plan of the MHA call on the same query shape under every knob, the error codes and their order, the audit report of the
`_gqa` kernels — and a test of the GPU test's inputs: a wrong head map leaves the bound by a wide margin on every head it touches."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import tol

# (B, H, Hkv, N, D) of the wrong-map check; B >= 2 and Hkv >= 2 both occur (with B = 1 the "batch 0" slip is invisible, with Hkv = 1 the
# `h % Hkv` slip is).  tests/test_gpu_gqa.py runs its oracle parity on the (B, H, Hkv) of the first two.
GQA_SHAPES = [(2, 6, 2, 1024, 64), (2, 4, 1, 1024, 128), (2, 8, 2, 256, 32), (1, 6, 3, 320, 96)]


def gqa_inputs(B, H, Hkv, N, D, seed):
    """fp16 randn q [B,H,N,D], k, v [B,Hkv,N,D] on the CPU (the GPU tests move them over: both files test the same inputs)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, N, D, generator=g).half(), torch.randn(B, Hkv, N, D, generator=g).half(),
            torch.randn(B, Hkv, N, D, generator=g).half())


def expand_kv(x, G):
    """[B,Hkv,...] -> [B,Hkv G,...]: query head h reads K / V head h // G (torch SDPA enable_gqa, flash-attn)"""
    return x.repeat_interleave(G, dim=1)


def _name_gqa(bh, g, n, d, flags):
    buf = C.create_string_buffer(128)
    rc = capi.load().lc_attn_kernel_name_gqa(bh, g, n, d, flags, buf, 128)
    return rc, buf.value.decode()


def _name_ex(bh, n, d, flags):
    buf = C.create_string_buffer(128)
    rc = capi.load().lc_attn_kernel_name_ex(bh, n, d, flags, buf, 128)
    return rc, buf.value.decode()


FLAGS = (0, capi.ATTN_V_TRANSPOSED, capi.ATTN_CAUSAL, capi.ATTN_CAUSAL | capi.ATTN_V_TRANSPOSED)
BHS = (-1, 1, 2, 8, 24, 64, 256, 4096)
NS = (64, 128, 192, 256, 384, 1024, 1152, 2048, 4096, 4224, 8192, 16384)


def _plan_parity():
    """every (G, BH, N, D <= 128, flags): the GQA name is the MHA name with `_kernel<` -> `_gqa_kernel<`; returns the kernels seen"""
    seen = set()
    for bh in BHS:
        for g in sorted({2, 3, 4, 8, bh} - {-1, 1}):
            if bh > 0 and bh % g != 0:
                continue
            for n in NS:
                for d in (32, 64, 96, 128):
                    for flags in FLAGS:
                        rc, mha = _name_ex(bh, n, d, flags)
                        assert rc == capi.LC_OK and mha.count("_kernel<") == 1, (bh, n, d, flags, rc, mha)
                        assert _name_gqa(bh, g, n, d, flags) == (capi.LC_OK, mha.replace("_kernel<", "_gqa_kernel<")), (bh, g, n, d, flags)
                        seen.add(mha.split("<")[0])
    return seen


def test_gqa_plan_is_the_mha_plan_of_the_same_query_shape(built):
    seen = _plan_parity()
    assert seen == {"attn_fwd_w4u_kernel", "attn_fwd_w4i_kernel", "attn_fwd_kernel", "attn_fwd_w4u_causal_kernel", "attn_fwd_causal_kernel"}
    assert capi.attn_kernel_name(4096, 128, bh=128, group=4) == "attn_fwd_w4u_gqa_kernel<128,false,1>"
    assert capi.attn_kernel_name(4096, 64, v_transposed=True, bh=32, causal=True, group=8) == "attn_fwd_w4u_causal_gqa_kernel<64,true>"
    assert capi.attn_kernel_name(1024, 96, bh=64, group=2) == "attn_fwd_w4i_gqa_kernel<96,1>"
    assert capi.attn_kernel_name(192, 32, bh=4, causal=True, group=4) == "attn_fwd_causal_gqa_kernel<32,2,false>"
    assert capi.attn_kernel_name(4096, 128, bh=128, group=1) == capi.attn_kernel_name(4096, 128, bh=128)


@pytest.mark.parametrize("knob,values", [("attn_nw", (8, 4, 2, 513, 514, 515, 517)), ("attn_split", (1, 2, 4)), ("attn_causal_order", (1, 2))])
def test_gqa_plan_parity_under_every_selection_knob(built, knob, values):
    old = capi.tune_get(knob)[0]
    for val in values:
        capi.tune(knob, val)
        try:
            _plan_parity()
        finally:
            capi.tune(knob, old)


def test_group_of_one_is_the_ex_name_call_for_every_head_dim(built):
    for bh in BHS:
        for n in NS + (96, 100):
            for d in (32, 64, 96, 128, 256, 512, 1024, 48, 0):
                for flags in FLAGS + (4, -1):
                    assert _name_gqa(bh, 1, n, d, flags) == _name_ex(bh, n, d, flags), (bh, n, d, flags)


def test_gqa_errors(built):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    c, vt = capi.ATTN_CAUSAL, capi.ATTN_V_TRANSPOSED
    # ---- the name call
    for flags in FLAGS:
        for d in (256, 512, 1024, 16, 48, 0):
            assert _name_gqa(8, 2, 1024, d, flags)[0] == capi.LC_ERR_HEADDIM, (d, flags)
        for g in (0, -1, -8):
            assert _name_gqa(8, g, 1024, 128, flags)[0] == capi.LC_ERR_SHAPE, g
        for bh, g in ((8, 3), (6, 4), (1, 2), (4, 8)):
            assert _name_gqa(bh, g, 1024, 128, flags)[0] == capi.LC_ERR_SHAPE, (bh, g)
        for n in (96, 100, 1000, 4100, 0, -64):
            assert _name_gqa(8, 2, n, 128, flags)[0] == capi.LC_ERR_SHAPE, n
        assert _name_gqa(8, 3, 1024, 256, flags)[0] == capi.LC_ERR_SHAPE      # shape before head dim
    for bad in (4, 8, 1 << 30, -1, c | 4):
        assert _name_gqa(8, 2, 1024, 128, bad)[0] == capi.LC_ERR_ARG, bad
        assert _name_gqa(8, 0, 1024, 256, bad)[0] == capi.LC_ERR_ARG, bad     # flags before shape and head dim
    assert lib.lc_attn_kernel_name_gqa(8, 2, 1024, 128, 0, None, 128) == capi.LC_ERR_ARG
    assert lib.lc_attn_kernel_name_gqa(8, 2, 1024, 128, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
    # ---- the launch entry: argument checks before any device work (these pointers are never dereferenced, no GPU is touched)
    p = C.c_void_p(16)
    f = lib.lc_attn_fwd_f16_gqa
    for flags in FLAGS:
        assert f(None, p, p, p, 1, 8, 2, 1024, 128, flags, None) == capi.LC_ERR_ARG
        assert f(p, None, p, p, 1, 8, 2, 1024, 128, flags, None) == capi.LC_ERR_ARG
        assert f(p, p, None, p, 1, 8, 2, 1024, 128, flags, None) == capi.LC_ERR_ARG
        assert f(p, p, p, None, 1, 8, 2, 1024, 128, flags, None) == capi.LC_ERR_ARG
        assert f(None, p, p, p, 1, 8, 3, 1000, 256, flags, None) == capi.LC_ERR_ARG          # null pointer first
        for hkv in (0, -1, 3, 5, 9, 16):
            assert f(p, p, p, p, 1, 8, hkv, 1024, 128, flags, None) == capi.LC_ERR_SHAPE, hkv
        assert f(p, p, p, p, 1, 8, 3, 1024, 256, flags, None) == capi.LC_ERR_SHAPE           # shape before head dim
        assert f(p, p, p, p, 1, 8, 2, 1000, 128, flags, None) == capi.LC_ERR_SHAPE           # N % 64 != 0
        assert f(p, p, p, p, 1, 8, 2, 100, 256, flags, None) == capi.LC_ERR_SHAPE
        assert f(p, p, p, p, 0, 8, 2, 1024, 128, flags, None) == capi.LC_ERR_SHAPE
        assert f(p, p, p, p, 1, 0, 0, 1024, 128, flags, None) == capi.LC_ERR_SHAPE
        assert f(C.c_void_p(8), p, p, p, 1, 8, 2, 1024, 128, flags, None) == capi.LC_ERR_SHAPE   # alignment, as lc_attn_fwd_f16
        for d in (256, 512, 1024, 16, 48):
            assert f(p, p, p, p, 1, 8, 2, 1024, d, flags, None) == capi.LC_ERR_HEADDIM, d
    for bad in (4, -1, c | vt | 4):
        assert f(p, p, p, p, 1, 8, 2, 1024, 128, bad, None) == capi.LC_ERR_ARG
        assert f(p, p, p, p, 1, 8, 8, 1024, 128, bad, None) == capi.LC_ERR_ARG
        assert f(p, p, p, p, 1, 8, 3, 1024, 256, bad, None) == capi.LC_ERR_ARG               # flags before everything
    # Hkv == H: lc_attn_fwd_f16_ex's own codes
    assert f(None, p, p, p, 1, 8, 8, 1024, 128, c, None) == capi.LC_ERR_ARG
    assert f(p, p, p, p, 1, 8, 8, 1000, 128, 0, None) == capi.LC_ERR_SHAPE
    assert f(p, p, p, p, 1, 8, 8, 1000, 128, c, None) == capi.LC_ERR_SHAPE


def test_capi_wrapper_checks_shapes_without_a_gpu(built):
    """capi.attn_fwd keeps refusing a K of another shape; capi.attn_fwd_gqa refuses CPU tensors (there is no CPU path) and, through
    _attn_dims_gqa, head counts that do not divide"""
    q, k, v = gqa_inputs(1, 6, 2, 64, 32, seed=1)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims(q, k, v, torch.empty_like(q))
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_fwd_gqa(q, k, v, torch.empty_like(q))
    assert capi._attn_dims_gqa(q, k, v, torch.empty_like(q)) == (1, 6, 2, 64, 32)
    assert capi._attn_dims_gqa(q, k, v.transpose(-2, -1).contiguous(), torch.empty_like(q), v_transposed=True) == (1, 6, 2, 64, 32)
    for bad_k in (torch.empty(1, 4, 64, 32), torch.empty(1, 12, 64, 32), torch.empty(2, 2, 64, 32), torch.empty(1, 2, 128, 32)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._attn_dims_gqa(q, bad_k.half(), bad_k.half(), torch.empty_like(q))
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi._attn_dims_gqa(q, k, v, torch.empty_like(q), v_transposed=True)


def test_audit_report_lists_the_gqa_kernels_under_their_twins_rules(built):
    from leetcuda_amd import isa_audit
    rep = json.loads((built["abi"].parent / "obj" / "isa_audit.json").read_text())
    by_name = {r["kernel"]: r for r in rep}
    gqa = [r for r in rep if "_gqa_kernel" in r["kernel"]]
    names = " ".join(r["kernel"] for r in gqa)
    for d in (64, 128):
        for vt in (0, 1):
            for walk in (0, 1, 2, 3):
                assert f"attn_fwd_w4u_gqa_kernelILi{d}ELb{vt}ELi{walk}E" in names, (d, vt, walk)
            assert f"attn_fwd_w4u_causal_gqa_kernelILi{d}ELb{vt}E" in names, (d, vt)
    for d, lb in ((32, 104), (64, 88), (96, 72), (128, 64)):
        for sched in (0, 1):
            k = [r["kernel"] for r in gqa if f"attn_fwd_w4i_gqa_kernelILi{d}ELi{sched}E" in r["kernel"]]
            assert len(k) == 1, (d, sched, k)
            assert [rng for rx, rng in isa_audit.OWNED_VGPRS if rx.search(k[0])] == [(lb, 255)]      # the reserved literal VGPRs of its twin
    assert len([r for r in gqa if "attn_fwd_w4u_gqa_kernel" in r["kernel"]]) == 16
    assert len([r for r in gqa if "attn_fwd_w4u_causal_gqa_kernel" in r["kernel"]]) == 4
    assert len([r for r in gqa if "attn_fwd_w4i_gqa_kernel" in r["kernel"]]) == 8
    for r in gqa:
        assert r["scratch"] == 0 and not r["violations"] and r["compiler_accvgpr"] == 0, r
        key = r["kernel"][r["kernel"].index("attn_fwd"):r["kernel"].index("EEv") + 2]      # e.g. attn_fwd_w4u_gqa_kernelILi128ELb0ELi0EE
        twins = [n for n in by_name if key.replace("_gqa_kernel", "_kernel") + "v" in n]
        assert len(twins) == 1 and r["agpr"] == by_name[twins[0]]["agpr"], (r["kernel"], twins)
        if "w4u" in r["kernel"] or "w4i" in r["kernel"]:
            assert isa_audit._owned(r["kernel"]) == set(range(256)), r["kernel"]


def _attn64(q, k, v, causal):
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(q.shape[-1])
    if causal:
        N = q.shape[2]
        s = np.where(np.tril(np.ones((N, N), bool)), s, -np.inf)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    return (p / p.sum(-1, keepdims=True)) @ v


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("shape", GQA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_wrong_head_map_leaves_the_bound_on_every_head_it_touches(shape, causal):
    """A test of the GPU test's inputs: under `h % Hkv` (tile instead of repeat_interleave), "every batch reads batch 0" and the flat
    `bh % (B Hkv)`, the fp64 result misses the bound of tests/tol.py (causal row i: that of i + 1 keys) by >= 20 x on EVERY head whose
    K / V head the wrong map changes — so none of these slips can pass the oracle parity of tests/test_gpu_gqa.py."""
    B, H, Hkv, N, D = shape
    G = H // Hkv
    q, k, v = (x.double().numpy() for x in gqa_inputs(B, H, Hkv, N, D, seed=B * 1000 + H * 100 + Hkv * 10 + D))
    kk, vv = k.reshape(B * Hkv, N, D), v.reshape(B * Hkv, N, D)
    bh = np.arange(B * H)
    b, h = bh // H, bh % H
    right = b * Hkv + h // G
    assert (right == bh // G).all()                    # the flat form the kernels use
    wrong = {"h % Hkv": b * Hkv + h % Hkv, "batch 0": h // G, "bh % (B Hkv)": bh % (B * Hkv)}
    truth = _attn64(q, kk[right].reshape(B, H, N, D), vv[right].reshape(B, H, N, D), causal)
    if causal:
        atol = np.array([tol.attn_max_abs(i + 1) for i in range(N)]).reshape(1, 1, N, 1)
    else:
        atol = tol.attn_max_abs(N)
    bound = atol + tol.ATTN_RTOL_F16 * np.abs(truth)
    touched_any = 0
    for name, idx in wrong.items():
        touched = np.flatnonzero(idx != right)
        touched_any += touched.size
        if touched.size == 0:
            continue
        out = _attn64(q, kk[idx].reshape(B, H, N, D), vv[idx].reshape(B, H, N, D), causal)
        ratio = (np.abs(out - truth) / bound).reshape(B * H, -1).max(axis=1)
        assert ratio[touched].min() >= 20.0, (name, shape, causal, float(ratio[touched].min()))
        assert ratio[np.setdiff1d(bh, touched)].max(initial=0.0) == 0.0
    assert touched_any > 0
    if B >= 2 and Hkv >= 2:                            # the shapes that see all three slips
        assert all((idx != right).any() for idx in wrong.values())
