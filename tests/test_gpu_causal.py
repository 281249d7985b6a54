"""GPU tests of causal attention (lc_attn_fwd_f16_ex with LC_ATTN_CAUSAL): parity with the dense C oracle on EVERY row (causal row i is
the oracle's row over keys 0 .. i, held to the bound of a sequence of i + 1 keys), masking that no value behind the diagonal can reach, the two kernels against each other, batch and
grid-order invariance, the overflow slow path under the mask and the launch conditions (graph capture, another stream)."""

import numpy as np
import pytest
import torch

from tests import tol

pytestmark = pytest.mark.gpu


def _capi():
    from leetcuda_amd import capi
    capi.load()
    return capi


def _name(capi, N, D, vt, bh):
    return capi.attn_kernel_name(N, D, v_transposed=vt, bh=bh, causal=True)


def _want(N, D, vt):
    v = "true" if vt else "false"
    if D in (64, 128) and N % 256 == 0:
        return f"attn_fwd_w4u_causal_kernel<{D},{v}>"
    nw = 8 if N % 256 == 0 else 4 if N % 128 == 0 else 2
    return f"attn_fwd_causal_kernel<{D},{nw},{v}>"


def _inputs(B, H, N, D, seed):
    torch.manual_seed(seed)
    return [torch.randn(B, H, N, D, dtype=torch.half, device="cuda") for _ in range(3)]


def _run(capi, q, k, v, vt=False):
    """causal O (NaN-prefilled); v is [B,H,N,D] — handed over as [B,H,D,N] when vt"""
    o = torch.full_like(q, float("nan"))
    capi.attn_fwd(q, k, v.transpose(-2, -1).contiguous() if vt else v, o, v_transposed=vt, causal=True)
    torch.cuda.synchronize()
    return o


def _rows(N):
    """rows 0, 1, 63, 64, 255, 256, N - 1 and the first / last row of every 32-row wave slice of the first and the last 256-row
    block (the merged-phase kernel's waves own 64 rows, the lock-step kernel's 32)"""
    rs = {0, 1, 63, 64, 255, 256, N - 1}
    for base in (0, max(0, N - 256)):
        for w in range(0, 256, 32):
            rs |= {base + w, base + w + 31}
    return sorted(r for r in rs if 0 <= r < N)


def report_worst_row(excess, kernel, err=None):
    """Where a dense check failed: excess (and err) are [BH, N, D]; names the worst row, its 256-row block, its wave there (64 rows in
    the merged-phase kernel, 32 in the lock-step one) and row % 16, the row's place in an MFMA operand."""
    h, i, d = (int(x) for x in np.unravel_index(np.argmax(excess), excess.shape))
    per = 64 if "w4u" in kernel else 32
    bad = np.flatnonzero((excess > 0).any(axis=(0, 2)))
    return (f"{kernel}: worst at head {h} row {i} (block {i // 256}, wave {i % 256 // per} of {per} rows, row % 16 = {i % 16}) col {d}: "
            f"excess {excess[h, i, d]:.3e}" + ("" if err is None else f", |err| {err[h, i, d]:.3e}")
            + f"; {bad.size} rows over the bound, first {bad[:8].tolist()}")


def _check_dense(oracle, q, k, v, o, kernel):
    """EVERY row of every head against the dense causal oracle; row i under the bound of a sequence of i + 1 keys (tol.attn_close(N = i + 1),
    what _check_rows applies to the rows it samples)"""
    B, H, N, D = q.shape
    truth = oracle.attn_causal(q, k, v, B, H, N, D).reshape(B * H, N, D).astype(np.float64)
    out = o.reshape(B * H, N, D).float().cpu().numpy()
    assert np.isfinite(out).all(), report_worst_row(np.where(np.isfinite(out), 0.0, 1.0), kernel)
    err = np.abs(out.astype(np.float64) - truth)
    atol = np.array([tol.attn_max_abs(i + 1) for i in range(N)]).reshape(1, N, 1)
    excess = err - (atol + tol.ATTN_RTOL_F16 * np.abs(truth))
    assert (excess <= 0).all(), report_worst_row(excess, kernel, err)
    return float(err.max())


def _check_rows(oracle, q, k, v, o, rows, atol=None):
    B, H, N, D = q.shape
    BH = B * H
    qc, kc, vc = (x.reshape(BH, N, D).cpu() for x in (q, k, v))
    out = o.reshape(BH, N, D).float().cpu().numpy()
    assert np.isfinite(out).all()
    for i in rows:
        truth = oracle.attn_rows(qc[:, i:i + 1].contiguous(), kc[:, :i + 1].contiguous(), vc[:, :i + 1].contiguous(), BH, 1, i + 1, D)
        if atol is None:
            ok, err, excess = tol.attn_close(out[:, i:i + 1], truth, i + 1)
        else:   # (scores of many units: Q is rounded to fp16 after the scale, tests/tol.py ATTN_RTOL_SPIKE)
            d = np.abs(out[:, i:i + 1].astype(np.float64) - truth)
            excess = d - (atol + tol.ATTN_RTOL_SPIKE * np.abs(truth))
            ok, err, excess = bool((excess <= 0).all()), float(d.max()), float(excess.max())
        assert ok, (i, err, excess)


@pytest.mark.parametrize("N", [64, 128, 192, 256, 320, 1024, 1152, 4096])
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_causal_vs_oracle(oracle, D, vt, N):
    capi = _capi()
    B, H = 1, 3      # (three heads: a slip in the head index of a block cannot cancel between two)
    assert _name(capi, N, D, vt, B * H) == _want(N, D, vt)
    q, k, v = _inputs(B, H, N, D, seed=D * 7919 + N + vt)
    o = _run(capi, q, k, v, vt)
    _check_dense(oracle, q, k, v, o, _want(N, D, vt))
    # row 0 sees key 0 only: O[0] = V[0] within one fp16 ulp
    o0, v0 = o[:, :, 0].float(), v[:, :, 0].float()
    assert ((o0 - v0).abs() <= v0.abs() * 2.0 ** -10 + 2.0 ** -24).all()
    # the last row sees every key: the non-causal result's last row
    full = torch.full_like(q, float("nan"))
    capi.attn_fwd(q, k, v, full)
    torch.cuda.synchronize()
    d = (o[:, :, N - 1].float() - full[:, :, N - 1].float()).abs()
    assert d.max().item() <= 2 * tol.attn_max_abs(N) + 2.0 ** -9 * full[:, :, N - 1].float().abs().max().item()


# (j, kernel): j at a tile boundary, inside a diagonal tile, at a wave boundary of either kernel
@pytest.mark.parametrize("j", [63, 255, 300, 319, 700])
@pytest.mark.parametrize("D", [128, 64, 96])
def test_keys_behind_the_diagonal_change_nothing(D, j):
    capi = _capi()
    B, H, N = 1, 3, 1024
    q, k, v = _inputs(B, H, N, D, seed=31 + D + j)
    assert _name(capi, N, D, False, B * H) == _want(N, D, False)
    ref = _run(capi, q, k, v)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, j + 1:] = 0.5 * torch.randn_like(k2[:, :, j + 1:])
    v2[:, :, j + 1:] = torch.randn_like(v2[:, :, j + 1:])
    o = _run(capi, q, k2, v2)
    assert torch.equal(o[:, :, :j + 1], ref[:, :, :j + 1])
    assert not torch.equal(o[:, :, j + 1:], ref[:, :, j + 1:])


# Non-finite keys: j at wave boundaries of both kernels (64-row waves contain 32-row waves).  Row j + 1 of a wave that also holds
# rows <= j would see a non-finite score of its own; the wave-wide overflow guard / deferred rescale then takes its slow path for the
# whole wave, which rounds the other rows differently (still correct, not bit-identical).
@pytest.mark.parametrize("j", [63, 255, 319, 511])
@pytest.mark.parametrize("D", [128, 64, 32])
def test_non_finite_keys_behind_the_diagonal_stay_invisible(D, j):
    capi = _capi()
    B, H, N = 1, 2, 1024
    q, k, v = _inputs(B, H, N, D, seed=97 + D + j)
    ref = _run(capi, q, k, v)
    k2 = k.clone()
    k2[:, :, j + 1::3] = float("nan")
    k2[:, :, j + 2::3] = float("inf")
    k2[:, :, j + 3::3] = float("-inf")
    o = _run(capi, q, k2, v)
    assert torch.isfinite(o[:, :, :j + 1]).all()
    assert torch.equal(o[:, :, :j + 1], ref[:, :, :j + 1])


@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("D", [64, 128])
def test_merged_phase_agrees_with_the_lockstep_cross_check(oracle, D, vt):
    capi = _capi()
    B, H, N = 2, 2, 2048
    q, k, v = _inputs(B, H, N, D, seed=4242 + D)
    merged = _run(capi, q, k, v, vt)
    outs = {}
    for nw in (8, 4, 2):
        capi.tune("attn_nw", nw)
        try:
            assert _name(capi, N, D, vt, B * H) == f"attn_fwd_causal_kernel<{D},{nw},{'true' if vt else 'false'}>"
            outs[nw] = _run(capi, q, k, v, vt)
        finally:
            capi.tune("attn_nw", 0)
    for nw, o in outs.items():
        ok, err, excess = tol.attn_close(o.float().cpu().numpy(), merged.float().cpu().numpy(), 256, rtol=2.0 ** -9)
        assert ok, (nw, err, excess)
    _check_dense(oracle, q, k, v, outs[2], f"attn_fwd_causal_kernel<{D},2,{'true' if vt else 'false'}>")


@pytest.mark.parametrize("D,N", [(128, 1024), (64, 2048), (96, 512), (128, 320)])
def test_a_head_alone_matches_the_same_head_in_a_large_batch(D, N):
    capi = _capi()
    B, H = 4, 16
    q, k, v = _inputs(B, H, N, D, seed=5 + D + N)
    assert _name(capi, N, D, False, 1) == _name(capi, N, D, False, B * H) == _want(N, D, False)
    big = _run(capi, q, k, v)
    for b, h in ((0, 0), (2, 9), (3, 15)):
        one = _run(capi, *(x[b:b + 1, h:h + 1].contiguous() for x in (q, k, v)))
        assert torch.equal(one[0, 0], big[b, h]), (b, h)


@pytest.mark.parametrize("D", [64, 128])
def test_both_grid_orders_give_the_same_bits(D):
    capi = _capi()
    B, H, N = 3, 5, 2048
    q, k, v = _inputs(B, H, N, D, seed=808 + D)
    assert capi.tune_get("attn_causal_order") == (0, 0)
    a = _run(capi, q, k, v)
    outs = {}
    for order in (1, 2):      # longest block first, head-major
        capi.tune("attn_causal_order", order)
        try:
            outs[order] = (_run(capi, q, k, v, False), _run(capi, q, k, v, True))
        finally:
            capi.tune("attn_causal_order", 0)
    assert torch.equal(outs[1][0], a) and torch.equal(outs[2][0], a)
    assert torch.equal(outs[1][1], outs[2][1])
    assert (a.float() - outs[1][1].float()).abs().max().item() < 1e-3


@pytest.mark.parametrize("D", [64, 128])
def test_the_auto_rule_reaches_head_major_order_with_the_same_bits(oracle, D):
    """66 heads x 8 blocks = 528 blocks: more than 8 rounds of a 64-CU device ("rule_cus" = 64), so the auto rule launches head-major —
    the branch the forced knob value 2 reaches otherwise —, and fewer than 8 rounds of the 256-CU device itself, so auto is longest-first
    there.  Both, and both forced orders, give one set of bits; a head of the large launch is the same head launched alone; one head is
    compared densely with the oracle."""
    capi = _capi()
    B, H, N = 2, 33, 2048
    assert B * H * (N // 256) > 8 * 64
    q, k, v = _inputs(B, H, N, D, seed=606 + D)
    assert capi.tune_get("attn_causal_order") == (0, 0) and capi.tune_get("rule_cus") == (0, 0)
    assert _name(capi, N, D, False, B * H) == _want(N, D, False)
    own = _run(capi, q, k, v)
    capi.tune("rule_cus", 64)
    try:
        assert _name(capi, N, D, False, B * H) == _want(N, D, False)
        auto64 = _run(capi, q, k, v)
    finally:
        capi.tune("rule_cus", 0)
    forced = {}
    for order in (1, 2):
        capi.tune("attn_causal_order", order)
        try:
            forced[order] = _run(capi, q, k, v)
        finally:
            capi.tune("attn_causal_order", 0)
    assert torch.equal(auto64, own) and torch.equal(forced[1], own) and torch.equal(forced[2], own)
    for b, h in ((0, 0), (1, 16), (1, 32)):
        one = _run(capi, *(x[b:b + 1, h:h + 1].contiguous() for x in (q, k, v)))
        assert torch.equal(one[0, 0], auto64[b, h]), (b, h)
    _check_dense(oracle, *(x[1:2, 32:33].contiguous() for x in (q, k, v, auto64)), _want(N, D, False))


@pytest.mark.parametrize("D,N", [(128, 1024), (64, 4096), (96, 768), (32, 320)])
def test_ex_entry_without_the_mask_is_lc_attn_fwd_f16(D, N):
    capi = _capi()
    lib = capi.load()
    B, H = 2, 3
    q, k, v = _inputs(B, H, N, D, seed=11 + D)
    for vt in (0, 1):
        vv = v.transpose(-2, -1).contiguous() if vt else v
        a, b = torch.full_like(q, float("nan")), torch.full_like(q, float("nan"))
        capi.attn_fwd(q, k, vv, a, v_transposed=bool(vt))
        rc = lib.lc_attn_fwd_f16_ex(q.data_ptr(), k.data_ptr(), vv.data_ptr(), b.data_ptr(), B, H, N, D,
                                    capi.ATTN_V_TRANSPOSED if vt else 0, torch.cuda.current_stream().cuda_stream)
        assert rc == capi.LC_OK
        torch.cuda.synchronize()
        assert torch.equal(a, b), vt


@pytest.mark.parametrize("D", [128, 64, 96])
def test_overflow_slow_path_under_the_mask(oracle, D):
    """Scores grow along the key index (s_ij = 16 j / N in natural units for every row): inside a diagonal tile the masked keys are the
    largest of their tile, so a mask applied after the overflow guard's row max — or after the exponentiation — would show."""
    capi = _capi()
    B, H, N = 1, 2, 1024
    torch.manual_seed(1234 + D)
    a = 4.0 / D ** 0.5
    q = torch.full((B, H, N, D), a, dtype=torch.half, device="cuda")
    ramp = (4.0 * torch.arange(N, device="cuda", dtype=torch.float32) / N).half()
    k = ramp.view(1, 1, N, 1).expand(B, H, N, D).contiguous()
    v = torch.randn(B, H, N, D, dtype=torch.half, device="cuda")
    assert _name(capi, N, D, False, B * H) == _want(N, D, False)
    capi.attn_slowpath_stats(reset=True)
    o = _run(capi, q, k, v)
    st = capi.attn_slowpath_stats(reset=True)
    if D in (64, 128):
        assert st[0] > 0 and st[2] == 0, st
    _check_rows(oracle, q, k, v, o, _rows(N) + [400, 500, 777], atol=8e-3)


def test_graph_capture_replays_the_eager_bits():
    capi = _capi()
    for D, N in ((128, 1024), (96, 512)):
        q, k, v = _inputs(2, 4, N, D, seed=77 + D)
        eager = _run(capi, q, k, v)
        o = torch.full_like(q, float("nan"))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # (warm the launcher outside the capture)
            capi.attn_fwd(q, k, v, o, causal=True)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            capi.attn_fwd(q, k, v, o, causal=True)
        o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager), D


def test_non_default_stream():
    capi = _capi()
    q, k, v = _inputs(2, 3, 2048, 128, seed=99)
    ref = _run(capi, q, k, v)
    s = torch.cuda.Stream()
    o = torch.full_like(q, float("nan"))
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        capi.attn_fwd(q, k, v, o, causal=True)
    s.synchronize()
    assert torch.equal(o, ref)
