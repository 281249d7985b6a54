"""Numerics at the edges of the value range, against the fp64 oracle or against the kernel itself: power-of-two scaling that must commute
bit for bit, overflow to +-inf, fp16 subnormal outputs, Inf / NaN operands on every path a special value can take (clamped sources,
zero-padded copies, split-K partials and their reduce, the forked border launch, the vector-ALU ladder), workspace that holds poison from
an earlier call, fp8 / MX scaling and NaN codes, and attention on scaled V.  Every case first asserts the kernel it covers."""
import contextlib
import math

import numpy as np
import pytest
import torch

from leetcuda_amd import host
from tests import tol

pytestmark = pytest.mark.gpu


def _capi():
    from leetcuda_amd import capi
    capi.load()
    return capi


@contextlib.contextmanager
def _knobs(capi, knobs):
    for k, v in knobs.items():
        capi.tune(k, v)
    try:
        yield
    finally:
        for k in knobs:
            capi.tune(k, capi.tune_get(k)[1])


def _bits(t):
    return t.view(torch.int16)


def _same_bits(x, y):
    return torch.equal(_bits(x), _bits(y))


def _cls(x):
    """numpy array -> per element 0 finite, 1 NaN, 2 +inf, 3 -inf."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 1, np.where(x == np.inf, 2, np.where(x == -np.inf, 3, 0)))


# ---- HGEMM families ---------------------------------------------------------------------------------------------------------------------
# (id, layout, shape, variant, knobs, name check).  The name check is (kind, text): "eq" / "start" / "start+end" (text = (start, end)).
# ks: the split factor of the case (first k of the second K range gets a planted value), or 1.
V_MFMA256, V_P2, V_W4B, V_W4C, V_W4X, V_W4Y, V_GENERIC = 1, 4, 9, 10, 12, 13, 3


def _nnn(lay):
    return "true" if lay == "nn" else "false"


def _families():
    out = []
    for lay in ("nn", "tn"):
        n = _nnn(lay)
        for vid, v, pre in (("mfma256", V_MFMA256, "hgemm_mfma256_kernel<"), ("pingpong2", V_P2, "hgemm_pingpong2_kernel<"), ("w4b", V_W4B, "hgemm_w4"),
                            ("w4c", V_W4C, "hgemm_w4"), ("w4x", V_W4X, "hgemm_w4"), ("w4y", V_W4Y, "hgemm_w4y_kernel<")):
            out.append((f"{vid}-{lay}", lay, (512, 256, 448), v, {}, ("start", pre), 1))
        out.append((f"w4y_border_splitk3-{lay}", lay, (384, 384, 4192), V_W4Y, {"hgemm_splitk": 3}, ("start", "hgemm_w4y_kernel<"), 3))
        out.append((f"mfma128-{lay}", lay, (384, 128, 160), "MFMA128", {}, ("start", f"hgemm_mfma128_kernel<{n},"), 1))
        out.append((f"mid22-{lay}", lay, (256, 256, 1056), "MID", {"hgemm_mid": 22, "hgemm_mid_ns": 3}, ("eq", f"hgemm_mid_kernel<{n},2,2,3>"), 1))
        out.append((f"mid_splitk3-{lay}", lay, (512, 512, 8224), "MID", {"hgemm_mid": 22, "hgemm_mid_splitk": 3},
                    ("start+end", ("hgemm_mid_sk_kernel<", "> x3")), 3))
        for fork in (0, 2):
            out.append((f"ragged_w4y_fork{fork}-{lay}", lay, (4100, 4104, 320), "RAGGED", {"hgemm_ragged_fork": fork},
                        ("start+end", (f"hgemm_w4y_kernel<{n},", f" + hgemm_mid_edge_kernel<{n},2,2,3>")), 1))
        out.append((f"ragged_mid_edge-{lay}", lay, (1000, 3000, 512), "RAGGED", {}, ("start", f"hgemm_mid_edge_kernel<{n},"), 1))
        out.append((f"ragged_splitk2-{lay}", lay, (100, 1032, 4096), "AUTO", {"hgemm_mid_splitk": 2},
                    ("start+end", (f"hgemm_mid_edge_sk_kernel<{n},", "> x2")), 2))
        for shp in ((1000, 3000, 520), (512, 1024, 4104)):
            out.append((f"kpad{shp[2]}-{lay}", lay, shp, "KPAD", {}, ("start", "hgemm_pad_copy_kernel + "), 1))
        out.append((f"edge-{lay}", lay, (257, 136, 72), "EDGE", {}, ("eq", f"hgemm_edge_kernel<{n}>"), 1))
        out.append((f"generic-{lay}", lay, (257, 129, 65), V_GENERIC, {}, ("eq", f"hgemm_generic_kernel<{n}>"), 1))
    out.append(("edge_n130-tn", "tn", (130, 130, 64), "EDGE", {}, ("eq", "hgemm_edge_kernel<false>"), 1))
    for rung in range(20, 31):
        out.append((f"valu{rung}-nn", "nn", (512, 384, 320), rung, {}, ("start", "hgemm_valu_"), 1))
    return out


FAMILIES = _families()
FAM_IDS = [f[0] for f in FAMILIES]


class _Case:
    def __init__(self, capi, fam):
        self.id, lay, (self.M, self.N, self.K), v, self.knobs, self.want, self.ks = fam
        self.capi = capi
        self.lay = capi.LAYOUT_NN if lay == "nn" else capi.LAYOUT_TN
        self.variant = v if isinstance(v, int) else getattr(capi, "HGEMM_" + v)
        self.auto_named = isinstance(v, str) and v in ("AUTO", "RAGGED", "KPAD", "MID")

    def assert_kernel(self):
        """The kernel this case covers (auto / ragged / padded routes as a 256-CU device decides them)."""
        capi = self.capi
        if self.auto_named and capi.device_check() != 256:
            return
        with _knobs(capi, self.knobs):
            name = capi.hgemm_kernel_name(self.M, self.N, self.K, self.lay, self.variant)
        kind, txt = self.want
        ok = name == txt if kind == "eq" else name.startswith(txt) if kind == "start" else (name.startswith(txt[0]) and name.endswith(txt[1]))
        assert ok, (self.id, name)

    def run(self, a, b, stream=None):
        """a [M,K], b [K,N] fp16 (logical NN operands) -> C, with NaN canaries on both sides of C checked."""
        M, N = self.M, self.N
        bb = host.as_col_major(b) if self.lay == self.capi.LAYOUT_TN else b
        pad = 2048
        buf = torch.full((M * N + 2 * pad,), float("nan"), dtype=torch.half, device="cuda")
        c = buf[pad:pad + M * N].view(M, N)
        torch.cuda.synchronize()
        with _knobs(self.capi, self.knobs), torch.cuda.stream(stream or torch.cuda.current_stream()):
            self.capi.hgemm(a, bb, c, layout=self.lay, variant=self.variant, swizzle_stride=256)
        torch.cuda.synchronize()
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + M * N:]).all(), (self.id, "wrote outside C")
        return c

    def rows(self, extra=()):
        M = self.M
        base = {0, 1, 63, 64, 127, 128, 255, 256, M // 2 + 3, M - 129, M - 65, M - 2, M - 1} if M > 512 else set(range(M))
        return sorted(r for r in base | set(extra) if 0 <= r < M)


def _base_operands(M, N, K, seed):
    """randn with every magnitude clamped to [2^-6, 8]: scaling by 2^e for |e| <= 7 stays exact and normal in fp16."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def one(r, c):
        x = torch.randn(r, c, device="cuda", generator=g)
        return (torch.sign(x) + (x == 0)) * x.abs().clamp(2.0 ** -6, 8.0)
    return one(M, K).half(), one(K, N).half()


def _normal16(x):
    """torch fp16 -> bool: finite and fp16-normal (or exactly zero)."""
    f = x.float().abs()
    return torch.isfinite(f) & ((f >= 2.0 ** -14) | (f == 0))


# ---- H1: power-of-two scaling commutes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_hgemm_power_of_two_scaling_commutes(fam):
    """out(2^ea A, 2^eb B) == 2^(ea+eb) out(A, B) bit for bit wherever both are fp16-normal: fp32 accumulation scales exactly, so a difference
    is a magnitude-dependent defect (a saturating or flushing conversion, an fp16 intermediate)."""
    capi = _capi()
    case = _Case(capi, fam)
    case.assert_kernel()
    a, b = _base_operands(case.M, case.N, case.K, case.M + case.N + case.K)
    c0 = case.run(a, b)
    assert torch.isfinite(c0).all()
    for ea, eb in ((5, 2), (-4, -3), (0, 7)):
        c = case.run(a * 2.0 ** ea, b * 2.0 ** eb)
        want = (c0.float() * 2.0 ** (ea + eb))
        m = _normal16(c) & _normal16(c0) & (want.abs() <= 65504) & ((want.abs() >= 2.0 ** -14) | (want == 0))
        assert m.float().mean().item() > 0.5, (case.id, ea, eb, "too few comparable outputs")
        bad = (c.float() != want) & m
        assert not bad.any(), (case.id, ea, eb, int(bad.sum()), c.float()[bad][:4].tolist(), want[bad][:4].tolist())


# ---- H2: overflow -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_hgemm_overflow_matches_round_to_nearest_even(oracle, fam):
    """Inputs scaled so that about half of the outputs exceed 65520: the correctly rounded fp16 result is +-inf there.  Outside a band of
    2^-20 sum|a b| around +-65520 the output's class (finite / +inf / -inf) equals the oracle's; inside it 65504 or inf of the right sign; never
    NaN; the finite outputs within the usual bound."""
    capi = _capi()
    case = _Case(capi, fam)
    case.assert_kernel()
    M, N, K = case.M, case.N, case.K
    e = round((17 - 0.5 * math.log2(K)) / 2)
    g = torch.Generator(device="cuda").manual_seed(K + 17)
    a = (torch.randn(M, K, device="cuda", generator=g) * 2.0 ** e).half()
    b = (torch.randn(K, N, device="cuda", generator=g) * 2.0 ** e).half()
    c = case.run(a, b)
    assert not torch.isnan(c).any(), case.id
    rows = case.rows()
    ar = a[rows].contiguous()
    exact = oracle.hgemm(ar, b.contiguous(), len(rows), N, K, 0, "exact").astype(np.float64)
    truth = oracle.hgemm(ar, b.contiguous(), len(rows), N, K, 0, "f32").astype(np.float64)
    absum = oracle.hgemm(ar.abs(), b.abs().contiguous(), len(rows), N, K, 0, "f32").astype(np.float64)
    out = c[rows].float().cpu().numpy().astype(np.float64)
    band = np.abs(np.abs(truth) - 65520.0) <= 2.0 ** -20 * absum
    frac = np.isinf(exact).mean()
    assert 0.25 < frac < 0.85, (case.id, frac)
    diff = (_cls(out) != _cls(exact)) & ~band
    assert not diff.any(), (case.id, int(diff.sum()), out[diff][:4], truth[diff][:4])
    inb = out[band]
    assert ((np.abs(inb) == 65504) | np.isinf(inb)).all() and (np.sign(inb) == np.sign(truth[band])).all(), case.id
    fin = np.isfinite(exact) & ~band
    err = np.abs(out[fin] - truth[fin])
    bound = tol.HGEMM_RTOL * np.abs(truth[fin]) + tol.hgemm_atol(K, 2.0 ** e)
    assert (err <= bound).all(), (case.id, float(err.max()))


# ---- H3: subnormal outputs ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_hgemm_subnormal_inputs_and_outputs(oracle, fam):
    """A = randn 2^-16 (mostly fp16 subnormals), B = randn 2^-6: outputs in the fp16 subnormal range.  |out - truth| <= 2^-24 (one subnormal
    step) everywhere and as many nonzero outputs as the correctly rounded result: catches flushed inputs as well as flushed outputs."""
    capi = _capi()
    case = _Case(capi, fam)
    case.assert_kernel()
    M, N, K = case.M, case.N, case.K
    g = torch.Generator(device="cuda").manual_seed(K + 3)
    a = (torch.randn(M, K, device="cuda", generator=g) * 2.0 ** -16).half()
    b = (torch.randn(K, N, device="cuda", generator=g) * 2.0 ** -6).half()
    assert (a.float().abs() < 2.0 ** -14).float().mean().item() > 0.99
    c = case.run(a, b)
    rows = case.rows()
    truth = oracle.hgemm(a[rows].contiguous(), b.contiguous(), len(rows), N, K, 0, "f32").astype(np.float64)
    exact = oracle.hgemm(a[rows].contiguous(), b.contiguous(), len(rows), N, K, 0, "exact")
    out = c[rows].float().cpu().numpy().astype(np.float64)
    assert (np.abs(truth) < 2.0 ** -14).mean() > 0.5, case.id
    err = np.abs(out - truth)
    assert np.isfinite(out).all() and (err <= 2.0 ** -24).all(), (case.id, float(np.nanmax(err)) * 2 ** 24, "subnormal steps")
    assert np.count_nonzero(out) == np.count_nonzero(exact.astype(np.float64)), (case.id, np.count_nonzero(out), np.count_nonzero(exact))


# ---- H4: non-finite operands --------------------------------------------------------------------------------------------------------

def _plant(case, a, b):
    """Inf / NaN at the places a kernel treats specially; returns (a, b, special rows of A, special columns of B).  Every other entry is
    finite and nonzero except a few exact zeros of B, which are planted in the unplanted run as well."""
    M, N, K = case.M, case.N, case.K
    a, b = a.clone(), b.clone()
    inf, nan = float("inf"), float("nan")
    r = [min(x, M - 1) for x in (3, 17, 40, 66, 91, 130)]
    ca = [min(x, N - 1) for x in (5, 29, 70, 101)]
    a[r[0], 0] = inf                                   # first K tile
    a[r[1], K - 1] = -inf                              # last K tile
    a[r[2], K // 2] = nan
    a[r[3], 3] = inf                                   # +inf and -inf in one row: NaN where the two products have the same sign
    a[r[3], K - 5] = -inf
    a[r[4], 7] = inf                                   # inf against exact zeros of B: NaN there
    b[7, ca[3]:ca[3] + 3] = 0.0
    a[M - 1, K // 3] = -inf                            # last row / column: clamped-source rows of ragged shapes
    b[K // 3 + 1, N - 1] = nan
    b[K - 1, ca[0]] = inf                              # last k (a chunk past K clamps to it)
    b[0, ca[1]] = nan
    b[K // 2 + 1, ca[2]] = -inf
    rows = {r[0], r[1], r[2], r[3], r[4], M - 1}
    cols = {ca[0], ca[1], ca[2], N - 1}
    if case.ks > 1:                                    # the first k of the second K range (both roundings of an uneven split)
        kt = -(-K // 64)
        for i, kk in enumerate(sorted({64 * (kt // case.ks), 64 * -(-kt // case.ks)})):
            if kk < K:
                a[r[5] - i, kk] = nan if i == 0 else inf
                rows.add(r[5] - i)
                b[kk, min(130 + i, N - 1)] = -inf
                cols.add(min(130 + i, N - 1))
    clean_a, clean_b = a.clone(), b.clone()
    clean_a[~torch.isfinite(clean_a)] = 1.0
    clean_b[~torch.isfinite(clean_b)] = 1.0
    return a, b, clean_a, clean_b, sorted(rows), sorted(cols)


@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_hgemm_non_finite_operands_reach_exactly_their_outputs(oracle, fam):
    """+inf / -inf / NaN in A and B (first and last K tile, the second K range of split-K, the last row and column, +inf and -inf in one row,
    inf against exact zeros): the NaN / +inf / -inf pattern equals the fp64 oracle's on sampled rows that include every planted row, and every
    output whose row and column carry no special value is bit-equal to the same kernel's result on the unplanted operands."""
    capi = _capi()
    case = _Case(capi, fam)
    case.assert_kernel()
    M, N, K = case.M, case.N, case.K
    a0, b0 = _base_operands(M, N, K, M * 3 + N + K)
    a, b, ca, cb, srows, scols = _plant(case, a0, b0)
    c = case.run(a, b)
    cref = case.run(ca, cb)
    rows = case.rows(srows)
    exact = oracle.hgemm(a[rows].contiguous(), b.contiguous(), len(rows), N, K, 0, "exact")
    out = c[rows].float().cpu().numpy()
    want = _cls(exact.astype(np.float64))
    got = _cls(out)
    assert (want[[rows.index(r) for r in srows]] != 0).any(axis=1).all(), case.id      # every planted row reaches some output
    bad = got != want
    assert not bad.any(), (case.id, int(bad.sum()), [(rows[i], j, int(got[i, j]), int(want[i, j])) for i, j in zip(*np.nonzero(bad))][:6])
    clean = torch.ones(M, N, dtype=torch.bool, device="cuda")
    clean[srows] = False
    clean[:, scols] = False
    assert torch.equal(_bits(c)[clean], _bits(cref)[clean]), (case.id, int((_bits(c) != _bits(cref))[clean].sum()))
    fin = (want == 0)
    ok, mx, _ = tol.hgemm_close(out[fin], oracle.hgemm(a[rows].contiguous(), b.contiguous(), len(rows), N, K, 0, "f32")[fin], K)
    assert ok, (case.id, mx)


# ---- W: reused workspace ------------------------------------------------------------------------------------------------------------
# (id, layout, shape, variant, knobs of the checked call, name check, poison knob sets, poison K)

def _ws_users():
    out = []
    for lay in ("nn", "tn"):
        n = _nnn(lay)
        out.append((f"w4y_border_splitk-{lay}", lay, (384, 384, 4192), V_W4Y, {"hgemm_splitk": 2}, ("start", "hgemm_w4y_kernel<"), 1, 4192,
                    [{"hgemm_splitk": 8}, {"hgemm_splitk": 2}]))
        out.append((f"mid_splitk-{lay}", lay, (512, 512, 8224), "MID", {"hgemm_mid": 22, "hgemm_mid_splitk": 3},
                    ("start+end", ("hgemm_mid_sk_kernel<", "> x3")), 3, 8224,
                    [{"hgemm_mid": 22, "hgemm_mid_splitk": 8}, {"hgemm_mid": 22, "hgemm_mid_splitk": 3}]))
        out.append((f"ragged_splitk-{lay}", lay, (100, 1032, 4096), "AUTO", {"hgemm_mid_splitk": 2},
                    ("start+end", (f"hgemm_mid_edge_sk_kernel<{n},", "> x2")), 2, 4096,
                    [{"hgemm_mid_splitk": 8}, {"hgemm_mid_splitk": 2}]))
        for (M, N, K) in ((1000, 3000, 520), (512, 1024, 4104)):
            out.append((f"kpad{K}-{lay}", lay, (M, N, K), "KPAD", {}, ("start", "hgemm_pad_copy_kernel + "), 1, K + 8, [{}]))
            out.append((f"kpad{K}_same-{lay}", lay, (M, N, K), "KPAD", {}, ("start", "hgemm_pad_copy_kernel + "), 1, K, [{}]))
    return out


WS_USERS = _ws_users()


@pytest.mark.parametrize("user", WS_USERS, ids=[u[0] for u in WS_USERS])
@pytest.mark.parametrize("poison_stream", ["same", "other"])
def test_hgemm_workspace_poison_does_not_leak(user, poison_stream):
    """Split-K partials and K-padded operand copies live in a cached buffer per (device, stream).  A call on NaN operands that leases at least
    as much of it (a larger split factor first; K + 8 before K, which pads to the same width, so the poison sits where the checked call needs
    zeros) goes first; the checked call must be bit-equal to the reference computed on a freshly allocated workspace.  The poison on another
    stream must not matter either."""
    capi = _capi()
    uid, lay, (M, N, K), v, knobs, want, ks, Kpoison, poisons = user
    case = _Case(capi, (uid, lay, (M, N, K), v, knobs, want, ks))
    case.assert_kernel()
    a, b = _base_operands(M, N, K, M + N + K + 1)
    capi.workspace_release()
    s = torch.cuda.Stream()
    ref = case.run(a, b, stream=s)
    assert torch.isfinite(ref).all()
    pa = torch.full((M, Kpoison), float("nan"), dtype=torch.half, device="cuda")
    pb = torch.full((Kpoison, N), float("nan"), dtype=torch.half, device="cuda")
    ps = s if poison_stream == "same" else torch.cuda.Stream()
    for pk in poisons:
        pcase = _Case(capi, (uid, lay, (M, N, Kpoison), v, pk, want, ks))
        pcase.run(pa, pb, stream=ps)
        c = case.run(a, b, stream=s)
        assert _same_bits(c, ref), (uid, pk, int((_bits(c) != _bits(ref)).sum()), int(torch.isnan(c).sum()))


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("poison_stream", ["same", "other"])
def test_attention_split_kv_workspace_poison_does_not_leak(D, poison_stream):
    """Split-KV partials (normalised O + log-sum-exp per row) in the stream's workspace: NaN V at factor 8 first, then factors 2 and 8 on clean
    inputs must reproduce the reference computed on a freshly allocated workspace bit for bit."""
    capi = _capi()
    B, H, N = 1, 6, 2048
    torch.manual_seed(D + 11)
    q = torch.randn(B, H, N, D, dtype=torch.half, device="cuda")
    k = torch.randn(B, H, N, D, dtype=torch.half, device="cuda")
    v = torch.randn(B, H, N, D, dtype=torch.half, device="cuda")
    vnan = torch.full_like(v, float("nan"))
    s = torch.cuda.Stream()
    ps = s if poison_stream == "same" else torch.cuda.Stream()

    def run(vv, S, st):
        o = torch.full_like(q, float("nan"))
        with _knobs(capi, {"attn_split": S}):
            assert capi.attn_kernel_name(N, D, bh=B * H) == f"attn_fwd_w4u_kernel<{D},false,3>"
            with torch.cuda.stream(st):
                capi.attn_fwd(q, k, vv, o)
        torch.cuda.synchronize()
        return o
    for S in (2, 8):
        capi.workspace_release()
        ref = run(v, S, s)
        assert torch.isfinite(ref).all()
        assert torch.isnan(run(vnan, 8, ps)).all()
        assert _same_bits(run(v, S, s), ref), S


# ---- F: fp8 and MX ------------------------------------------------------------------------------------------------------------------

FP8_FORMS = [3, 1, 2, 0]
FP8_IDS = ["mx_k128_generated", "mx_k64_4wave", "mx_k64_8wave", "plain_k16"]


def _fp8_run(capi, form, a, b, alpha, sa=None, sb=None):
    M, N = a.shape[0], b.shape[0]
    c = torch.full((M, N), float("nan"), dtype=torch.half, device="cuda")
    if form == "mxfp8":
        capi.gemm_mxfp8(a, capi.mxfp8_pack_scales(sa), b, capi.mxfp8_pack_scales(sb), c, alpha=alpha, swizzle_stride=512)
    else:
        with _knobs(capi, {"fp8_mx": form}):
            capi.gemm_fp8(a, b, c, alpha=alpha, swizzle_stride=512)
    torch.cuda.synchronize()
    return c


def _fp8_inputs(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g).to(torch.float8_e4m3fn)
    b = torch.randn(N, K, device="cuda", generator=g).to(torch.float8_e4m3fn)
    return a, b


@pytest.mark.parametrize("form", FP8_FORMS + ["mxfp8"], ids=FP8_IDS + ["mxfp8"])
def test_fp8_alpha_power_of_two_commutes_and_overflows_to_inf(oracle, form):
    """gemm(alpha 2^e) == 2^e gemm(alpha) bit for bit wherever both stay fp16-normal (alpha = 0.7, e = -5, +3); an alpha that overflows half of
    the outputs gives the oracle's +-inf pattern outside the 2^-20 sum|a b| band around +-65520, never NaN."""
    capi = _capi()
    M, N, K = 512, 256, 1024
    a, b = _fp8_inputs(M, N, K, 41)
    sa = torch.full((M, K // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
    c0 = _fp8_run(capi, form, a, b, 0.7, sa, sb)
    for e in (-5, 3):
        c = _fp8_run(capi, form, a, b, 0.7 * 2.0 ** e, sa, sb)
        want = c0.float() * 2.0 ** e
        m = _normal16(c) & _normal16(c0) & (want.abs() <= 65504) & ((want.abs() >= 2.0 ** -14) | (want == 0))
        assert m.float().mean().item() > 0.5
        assert not ((c.float() != want) & m).any(), (form, e)
    alpha = 2.0 ** 17 / 32.0        # |C| ~ 2^17: sum of K = 1024 randn products ~ 32
    c = _fp8_run(capi, form, a, b, alpha, sa, sb)
    assert not torch.isnan(c).any()
    rows = list(range(0, M, 16)) + [M - 1]
    truth = oracle.gemm_fp8(a[rows].contiguous(), b, len(rows), N, K, alpha).astype(np.float64)
    absum = oracle.gemm_fp8(a[rows].float().abs().to(torch.float8_e4m3fn).contiguous(), b.float().abs().to(torch.float8_e4m3fn), len(rows), N, K,
                            alpha).astype(np.float64)
    exact = truth.astype(np.float16).astype(np.float64)
    out = c[rows].float().cpu().numpy().astype(np.float64)
    band = np.abs(np.abs(truth) - 65520.0) <= 2.0 ** -20 * absum + 2.0 ** -11 * 65520 * (form != 0)   # (MX forms: block alignment, see _mx_bound)
    assert 0.25 < np.isinf(exact).mean() < 0.85
    diff = (_cls(out) != _cls(exact)) & ~band
    assert not diff.any(), (form, int(diff.sum()))


def _plant_e4m3_nan(a, b):
    a8, b8 = a.view(torch.uint8).clone(), b.view(torch.uint8).clone()
    a8[5, 0] = 0x7F
    a8[200, -1] = 0xFF
    b8[17, 64] = 0xFF
    b8[255, 127] = 0x7F
    return a8.view(torch.float8_e4m3fn), b8.view(torch.float8_e4m3fn), [5, 200], [17, 255]


@pytest.mark.parametrize("form", FP8_FORMS + ["mxfp8"], ids=FP8_IDS + ["mxfp8"])
def test_fp8_e4m3_nan_codes(oracle, form):
    """0x7F / 0xFF (the e4m3fn NaN codes) in rows of A and B: NaN exactly where the oracle has it, every other output bit-equal to the run
    without them."""
    capi = _capi()
    M, N, K = 256, 512, 384
    a, b = _fp8_inputs(M, N, K, 43)
    sa = torch.randint(124, 131, (M, K // 32), dtype=torch.uint8, device="cuda")
    sb = torch.randint(124, 131, (N, K // 32), dtype=torch.uint8, device="cuda")
    pa, pb, rs, cs = _plant_e4m3_nan(a, b)
    c0 = _fp8_run(capi, form, a, b, 1 / 3, sa, sb)
    c = _fp8_run(capi, form, pa, pb, 1 / 3, sa, sb)
    if form == "mxfp8":
        truth = oracle.gemm_mxfp8(pa, sa, pb, sb, M, N, K, 1 / 3)
    else:
        truth = oracle.gemm_fp8(pa, pb, M, N, K, 1 / 3)
    nan_want = np.isnan(truth)
    assert nan_want[rs].all() and nan_want[:, cs].all()
    assert np.array_equal(torch.isnan(c).cpu().numpy(), nan_want), (form, int((torch.isnan(c).cpu().numpy() != nan_want).sum()))
    clean = torch.ones(M, N, dtype=torch.bool, device="cuda")
    clean[rs] = False
    clean[:, cs] = False
    assert torch.equal(_bits(c)[clean], _bits(c0)[clean])


def _mx_run(capi, a, sa, b, sb, alpha):
    return _fp8_run(capi, "mxfp8", a, b, alpha, sa, sb)


def test_mxfp8_scale_offsets_and_extremes(oracle):
    """Adding d = +-20 to every scale of SA equals alpha 2^d bit for bit; SA = 254 against SB = 0 on the same blocks (and the reverse) matches the
    oracle (the two exponents are combined before they are applied: 2^127 2^-127 = 1, not an overflow)."""
    capi = _capi()
    M, N, K = 256, 256, 512
    a, b = _fp8_inputs(M, N, K, 47)
    g = torch.Generator(device="cuda").manual_seed(47)
    sa = torch.randint(124, 131, (M, K // 32), device="cuda", generator=g, dtype=torch.uint8)
    sb = torch.randint(124, 131, (N, K // 32), device="cuda", generator=g, dtype=torch.uint8)
    alpha = 1 / 3
    for d in (-20, 20):
        c1 = _mx_run(capi, a, (sa.int() + d).to(torch.uint8), b, sb, alpha)
        c2 = _mx_run(capi, a, sa, b, sb, alpha * 2.0 ** d)
        assert _same_bits(c1, c2), d
    # extremes: rows 0..63 of A at 254 where columns 0..63 of B are at 0, rows 64..127 of A at 0 where columns 64..127 of B are at 254
    # (the other outputs of those rows / columns overflow or underflow: not checked); rows and columns 128.. keep their scales
    sa2, sb2 = sa.clone(), sb.clone()
    sa2[:64] = 254
    sb2[:64] = 0
    sa2[64:128] = 0
    sb2[64:128] = 254
    c0 = _mx_run(capi, a, sa, b, sb, alpha)
    c = _mx_run(capi, a, sa2, b, sb2, alpha)
    truth = oracle.gemm_mxfp8(a, sa2, b, sb2, M, N, K, alpha).astype(np.float64)
    absum = oracle.gemm_mxfp8(a.float().abs().to(torch.float8_e4m3fn), sa2, b.float().abs().to(torch.float8_e4m3fn), sb2, M, N, K,
                              alpha).astype(np.float64)
    out = c.float().cpu().numpy().astype(np.float64)
    for q in (slice(0, 64), slice(64, 128)):
        t, o, s_ = truth[q, q], out[q, q], absum[q, q]
        assert np.isfinite(t).all() and np.isfinite(o).all(), (q, int((~np.isfinite(o)).sum()))
        err = np.abs(o - t)
        assert (err <= 2.0 ** -11 * np.abs(t) + 2.0 ** -12 * s_ + 1e-7).all(), (q, float(err.max()))
    assert _same_bits(c[128:, 128:], c0[128:, 128:])


@pytest.mark.parametrize("side", ["a", "b"])
def test_mxfp8_scale_255_is_nan(oracle, side):
    """E8M0 255 is NaN (OCP MX): SA = 255 on (row r, block kb) makes row r of C NaN and leaves everything else bit-equal to the run with 127
    there; the same for SB and its column."""
    capi = _capi()
    M, N, K = 256, 256, 512
    a, b = _fp8_inputs(M, N, K, 53)
    sa = torch.full((M, K // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
    c0 = _mx_run(capi, a, sa, b, sb, 1 / 3)
    where = [(0, 0), (37, 5), (255, 15)]
    s2 = (sa if side == "a" else sb).clone()
    for r, kb in where:
        s2[r, kb] = 255
    c = _mx_run(capi, a, s2 if side == "a" else sa, b, sb if side == "a" else s2, 1 / 3)
    truth = oracle.gemm_mxfp8(a, s2 if side == "a" else sa, b, sb if side == "a" else s2, M, N, K, 1 / 3)
    lines = [r for r, _ in where]
    nan = torch.isnan(c).cpu().numpy()
    assert np.array_equal(nan, np.isnan(truth)), (side, int(nan.sum()), int(np.isnan(truth).sum()))
    clean = torch.ones(M, N, dtype=torch.bool, device="cuda")
    if side == "a":
        clean[lines] = False
    else:
        clean[:, lines] = False
    assert torch.equal(_bits(c)[clean], _bits(c0)[clean])


# ---- A: attention on scaled V -------------------------------------------------------------------------------------------------------

def _attn_families():
    out = []
    for D in (64, 128):
        for vt in (False, True):
            out.append((f"w4u-d{D}-{'vt' if vt else 'v'}", D, vt, 1, 2, 1024, {"attn_nw": 513, "attn_split": 1},
                        ("eq", f"attn_fwd_w4u_kernel<{D},{str(vt).lower()},0>")))
    for D in (32, 96):
        out.append((f"w4i-d{D}", D, False, 1, 2, 1024, {"attn_nw": 514}, ("start", f"attn_fwd_w4i_kernel<{D},")))
    for D in (32, 64, 96, 128):
        for vt in (False, True):
            out.append((f"lockstep-d{D}-{'vt' if vt else 'v'}", D, vt, 1, 2, 512, {"attn_nw": 4}, ("eq", f"attn_fwd_kernel<{D},4,{str(vt).lower()},0>")))
    for D in (64, 128):
        for S in (2, 8):
            out.append((f"split{S}-d{D}", D, False, 1, 6, 2048, {"attn_split": S}, ("eq", f"attn_fwd_w4u_kernel<{D},false,3>")))
    for D in (256, 512, 1024):
        out.append((f"bigd-d{D}", D, False, 1, 2, 256, {}, ("start", "attn_fwd_bigd")))
    for D in (256, 512):
        out.append((f"bf16-d{D}", D, False, 1, 2, 256, {}, ("start", "attn_fwd_bigd")))
    # causal (lc_attn_fwd_f16_ex): the merged-phase kernel, and the lock-step kernel with 8, 4 and 2 waves
    for D in (64, 128):
        for vt in (False, True):
            out.append((f"causal-w4u-d{D}-{'vt' if vt else 'v'}", D, vt, 1, 2, 1024, {}, ("eq", f"attn_fwd_w4u_causal_kernel<{D},{str(vt).lower()}>")))
    for D in (32, 64, 96, 128):
        for nw, N, knobs in ((8, 512, {"attn_nw": 8}), (4, 384, {}), (2, 320, {})):
            for vt in (False, True):
                out.append((f"causal-lockstep{nw}-d{D}-{'vt' if vt else 'v'}", D, vt, 1, 2, N, knobs,
                            ("eq", f"attn_fwd_causal_kernel<{D},{nw},{str(vt).lower()}>")))
    return out


ATTN_FAMILIES = _attn_families()


def _attn_run(capi, fam, q, k, v):
    fid, D, vt, B, H, N, knobs, want = fam
    o = torch.full_like(q, float("nan"))
    causal = fid.startswith("causal")
    with _knobs(capi, knobs):
        name = capi.attn_kernel_name(N, D, vt, bf16=fid.startswith("bf16"), bh=B * H, causal=causal)
        kind, txt = want
        assert (name == txt) if kind == "eq" else name.startswith(txt), (fid, name)
        if fid.startswith("bf16"):
            capi.attn_fwd_bf16(q, k, v, o)
        elif fid.startswith("bigd"):
            capi.attn_call("flash_attn_mma_stages_split_q_tiling_qkv", q, k, v, o, 2)
        else:
            capi.attn_fwd(q, k, v.transpose(-2, -1).contiguous() if vt else v, o, v_transposed=vt, causal=causal)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("fam", ATTN_FAMILIES, ids=[f[0] for f in ATTN_FAMILIES])
def test_attention_v_scaling_commutes(fam):
    """V with magnitudes in [2^-6, 8] and one sign per column d: every partial and final O is a convex combination bounded away from 0, so
    O(Q, K, 2^e V) == 2^e O(Q, K, V) bit for bit for e = -8, +6, +12 (|V| up to 32768: an unnormalised fp16 intermediate of O would overflow).
    The causal families keep the premise: a masked row is a convex combination of fewer same-signed values (row 0: of one)."""
    capi = _capi()
    fid, D, vt, B, H, N, knobs, want = fam
    dt = torch.bfloat16 if fid.startswith("bf16") else torch.half
    g = torch.Generator(device="cuda").manual_seed(D + N)
    q = torch.randn(B, H, N, D, device="cuda", generator=g).to(dt)
    k = torch.randn(B, H, N, D, device="cuda", generator=g).to(dt)
    mag = torch.rand(B, H, N, D, device="cuda", generator=g) * 9.0 - 6.0
    sign = torch.where(torch.rand(D, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    v = (sign * torch.pow(2.0, mag).clamp(2.0 ** -6, 8.0)).to(dt)
    o0 = _attn_run(capi, fam, q, k, v)
    assert torch.isfinite(o0.float()).all()
    for e in (-8, 6, 12):
        o = _attn_run(capi, fam, q, k, (v.float() * 2.0 ** e).to(dt))
        assert torch.equal(o.float(), o0.float() * 2.0 ** e), (fid, e, float((o.float() - o0.float() * 2.0 ** e).abs().max()))


@pytest.mark.parametrize("fam", [f for f in ATTN_FAMILIES if not f[0].startswith("bf16")], ids=[f[0] for f in ATTN_FAMILIES if not f[0].startswith("bf16")])
def test_attention_subnormal_output(oracle, fam):
    """V = randn 2^-20: O lies in the fp16 subnormal range; |out - truth| <= 2^-24 + ATTN_RTOL_F16 |truth| (one subnormal step)."""
    capi = _capi()
    fid, D, vt, B, H, N, knobs, want = fam
    g = torch.Generator(device="cuda").manual_seed(D * 7 + N)
    q = torch.randn(B, H, N, D, device="cuda", generator=g).half()
    k = torch.randn(B, H, N, D, device="cuda", generator=g).half()
    v = (torch.randn(B, H, N, D, device="cuda", generator=g) * 2.0 ** -20).half()
    o = _attn_run(capi, fam, q, k, v)
    if fid.startswith("causal"):
        truth = oracle.attn_causal(q, k, v, B, H, N, D).astype(np.float64)
    else:
        truth = oracle.attn(q, k, v, B, H, N, D, mode="f32").astype(np.float64)
    out = o.float().cpu().numpy().astype(np.float64)
    assert (np.abs(truth) < 2.0 ** -14).all()
    err = np.abs(out - truth)
    assert np.isfinite(out).all() and (err <= 2.0 ** -24 + tol.ATTN_RTOL_F16 * np.abs(truth)).all(), (fid, float(err.max()) * 2 ** 24)
    assert (out != 0).mean() > 0.25, fid
