"""The walks of the fp8 / MX GEMM kernels, checked on EVERY element with inputs whose result is exact in any summation order.

gemm_fp8_w4k_kernel<MX> (lc_gemm_fp8_e4m3 with "fp8_mx" = 3, lc_gemm_mxfp8) is hgemm_w4y_kernel outside its K loop: the K-loop stagger
(start tile ((idx & mask) * step) % KT, wrapping), one persistent workgroup per CU that prefetches the next C tile's first two K tiles
under the epilogue, the block -> tile rasters; the MX form adds a scale prefetch one K tile ahead into one of two register sets chosen
by the tile's parity.  gemm_fp8_w4_kernel ("fp8_mx" = 1) has the stagger too.  A skipped, doubled or mis-paired K tile, a scale set of the
wrong parity behind the seam or a C tile the walk never writes would pass a randn comparison under fp8_atol / _mx_bound on sampled
rows; here it cannot:

  e4m3 values from {0.5, 1, 1.5, -1, 2, -0.5, 0.75, -2}, E8M0 scales from {126, 127, 128} per (row, 32 k) on both operands: every product
  is a multiple of 2^-6 with |product| <= 16, so while sum |terms| < 2^12 every partial sum, in any order, is an integer below 2^18 in
  units of 2^-6 and fits fp32's 24 bits; with alpha a power of two the fp16 output is the exact sum rounded once.

The truth is alpha * (da.double() @ db.double().t()) with torch on the dequantised operands (checker math on the GPU in fp64, not ours),
anchored to the project's oracle on a handful of rows.  C is NaN-prefilled before every launch; the assertion is
torch.isfinite(c).all() and torch.equal(c, truth_half).  What arithmetic cannot settle is the matrix core's in-instruction block sum, so
every test first asserts its BASELINE launch (stagger off, "hgemm_persist" 0, "hgemm_raster" 1) against the truth."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_gqa import _knobs

pytestmark = pytest.mark.gpu

STAGGER_OFF = 1 << 27            # lc_tune_set "hgemm_stagger": exactly this value = the plain walk from tile 0; 0 = auto (by XCD)
VALUES = (0.5, 1.0, 1.5, -1.0, 2.0, -0.5, 0.75, -2.0)
ALPHAS = (1.0, 1.0 / 16)
FORMS = (3, 1, 2, 0, "mx")       # lc_gemm_fp8_e4m3 under "fp8_mx" = 3 / 1 / 2 / 0, lc_gemm_mxfp8
BASELINE = dict(hgemm_stagger=STAGGER_OFF, hgemm_persist=0, hgemm_raster=1)


def _capi():
    from leetcuda_amd import capi
    capi.load()
    return capi


def _exact_inputs(oracle, M, N, K, seed):
    """One input set: a [M,K], b [N,K] e4m3, sa / sb E8M0 with their packed forms pa / pb, and truth[kind, alpha]: the fp16 truth with
    unit scales (kind "unit": lc_gemm_fp8_e4m3) and with the block scales (kind "mx": lc_gemm_mxfp8)."""
    capi = _capi()
    g = torch.Generator(device="cuda").manual_seed(seed)
    vals = torch.tensor(VALUES, device="cuda")
    x = SimpleNamespace()
    x.M, x.N, x.K = M, N, K
    x.a = vals[torch.randint(0, 8, (M, K), device="cuda", generator=g)].to(torch.float8_e4m3fn)
    x.b = vals[torch.randint(0, 8, (N, K), device="cuda", generator=g)].to(torch.float8_e4m3fn)
    x.sa = torch.randint(126, 129, (M, K // 32), device="cuda", generator=g, dtype=torch.uint8)
    x.sb = torch.randint(126, 129, (N, K // 32), device="cuda", generator=g, dtype=torch.uint8)
    x.pa, x.pb = capi.mxfp8_pack_scales(x.sa), capi.mxfp8_pack_scales(x.sb)
    rows = sorted({0, 1, 255, 256, M // 2 + 17, M - 1})
    x.truth = {}
    for kind in ("unit", "mx"):
        da, db = x.a.double(), x.b.double()
        if kind == "mx":
            da = da * torch.pow(2.0, x.sa.double() - 127).repeat_interleave(32, dim=1)
            db = db * torch.pow(2.0, x.sb.double() - 127).repeat_interleave(32, dim=1)
        t = da @ db.t()
        # the premises of "exact in any order": multiples of 2^-6, sum |terms| < 2^18 / 64, nothing near the fp16 range's end
        assert bool((t * 64 == torch.round(t * 64)).all()), (kind, M, N, K)
        span = float((da.abs() @ db.abs().t()).max())
        assert span < 2.0 ** 18 / 64, (kind, M, N, K, span)
        assert float(t.abs().max()) * max(ALPHAS) < 65504.0
        for alpha in ALPHAS:
            x.truth[kind, alpha] = (alpha * t).half()
            # the anchor: the project's oracle (fp64 accumulation of the decoded values, returned as fp32) says the same on these rows
            if kind == "mx":
                o = oracle.gemm_mxfp8(x.a[rows].contiguous(), x.sa[rows].contiguous(), x.b, x.sb, len(rows), N, K, alpha)
            else:
                o = oracle.gemm_fp8(x.a[rows].contiguous(), x.b, len(rows), N, K, alpha)
            assert np.array_equal(o.astype(np.float64), (alpha * t[rows]).cpu().numpy()), (kind, M, N, K, alpha)
        del t, da, db
    return x


def _launch(capi, x, form, alpha, stride=1, **knobs):
    """C (NaN-prefilled) of one launch of `form` under `knobs`; every knob is back at its previous value on return"""
    c = torch.full((x.M, x.N), float("nan"), dtype=torch.half, device="cuda")
    if form == "mx":
        with _knobs(capi, **knobs):
            capi.gemm_mxfp8(x.a, x.pa, x.b, x.pb, c, alpha=alpha, swizzle_stride=stride)
    else:
        with _knobs(capi, fp8_mx=form, **knobs):
            capi.gemm_fp8(x.a, x.b, c, alpha=alpha, swizzle_stride=stride)
    torch.cuda.synchronize()
    return c


def _want(x, form, alpha):
    return x.truth["mx" if form == "mx" else "unit", alpha]


def report_first_bad(c, want, what):
    """Where a launch differs from the truth: the first wrong element's C tile and its place inside it, the share of wrong elements
    and the wrong tiles (a NaN is an element no workgroup wrote)."""
    bad = (c != want) | ~torch.isfinite(c)
    idx = torch.nonzero(bad)
    r, col = (int(v) for v in idx[0])
    tiles = sorted({(int(i) // 256, int(j) // 256) for i, j in idx[:: max(1, len(idx) // 4096)].tolist()})
    return (f"{what}: first wrong element in C tile (row {r // 256}, col {col // 256}) at row % 256 = {r % 256}, col % 256 = {col % 256}: "
            f"got {float(c[r, col])}, want {float(want[r, col])}; {len(idx) / bad.numel():.4%} of the elements wrong, "
            f"{int((~torch.isfinite(c)).sum())} not finite; wrong tiles (sampled) {tiles[:12]}")


def _assert_exact(c, want, what):
    assert bool(torch.isfinite(c).all()) and torch.equal(c, want), report_first_bad(c, want, what)


def _assert_baseline(capi, x, form):
    """stagger off, one tile per workgroup, the block-swizzle raster: must be exact before any walk variant is judged against the truth"""
    for alpha in ALPHAS:
        c = _launch(capi, x, form, alpha, **BASELINE)
        _assert_exact(c, _want(x, form, alpha), f"BASELINE launch of form {form} at {(x.M, x.N, x.K)} alpha {alpha}")


STAGGER_KNOBS = (STAGGER_OFF, 0, 1 | 16 << 12 | 7 << 20, 1 << 4 | 2 << 12 | 31 << 20, 1 << 8 | 2 << 12 | 31 << 20,
                 1 << 4 | 3 << 8 | 3 << 12 | 31 << 20, 15 | 15 << 4 | 15 << 8 | 255 << 12 | 127 << 20)


@pytest.mark.parametrize("K", [128, 256, 384, 640, 1024, 1152])
@pytest.mark.parametrize("shape", [(512, 1024), (768, 768)], ids=["8_tiles", "9_tiles"])
def test_stagger_walks_every_k_tile_once(oracle, shape, K):
    """lc_tune_set "hgemm_stagger" on the fp8 kernels that take it ("fp8_mx" = 3, 1 and lc_gemm_mxfp8): off, auto, XCD / tile row / tile
    column / mixed indices and start tiles beyond KT, on KT = 1, 2, 3 (the clamped prefetch of the last iterations wraps too), 5, 9 (odd,
    no multiple of the auto step) and 8.  2 x 4 tiles: all eight values of v & 7 with tm in {0, 1}, tn in {0..3}; 3 x 3: id 8 wraps onto XCD
    0.  Every launch equals the truth bit for bit — a skipped, doubled or mis-paired K tile changes > 99 % of the outputs.  The two
    kernels without a stagger ("fp8_mx" = 2, 0) run once, so that the cross-check kernels stand on the same exact footing."""
    capi = _capi()
    M, N = shape
    x = _exact_inputs(oracle, M, N, K, seed=M + N + K)
    for form in (3, 1, "mx"):
        _assert_baseline(capi, x, form)
        for knob in STAGGER_KNOBS:
            for alpha in ALPHAS:
                c = _launch(capi, x, form, alpha, stride=512, hgemm_stagger=knob)
                _assert_exact(c, _want(x, form, alpha), f"form {form} {(M, N, K)} hgemm_stagger {knob:#x} alpha {alpha}")
    for form in (2, 0):
        for alpha in ALPHAS:
            c = _launch(capi, x, form, alpha, stride=512)
            _assert_exact(c, _want(x, form, alpha), f"form {form} {(M, N, K)} alpha {alpha}")


@pytest.mark.parametrize("K", [128, 256, 384, 640])
@pytest.mark.parametrize("r", [2, 3], ids=["two_tiles_per_cu", "three_tiles_per_cu"])
def test_persistent_walk_crosses_the_seam_with_the_same_bits(oracle, r, K):
    """One persistent workgroup per CU walking r C tiles ("hgemm_persist" = 1, taken when the tile count is a larger multiple of the CU
    count) against one workgroup per tile, "fp8_mx" = 3 and lc_gemm_mxfp8: KT = 1 (the prefetch under the epilogue is the whole K loop's
    supply), 2, 3 and 5 (odd: the ring slot and the scale registers' parity at the seam differ from the tile's start); r = 3 crosses the seam
    twice, and the last tile of every workgroup has no successor.  With both rasters and the stagger off / auto the two launches
    agree bit for bit, and both equal the truth on every element."""
    capi = _capi()
    ncu = capi.device_check()
    assert ncu % 8 == 0, ncu
    tiles_m, tiles_n = ncu // 8, 8 * r
    nblk = tiles_m * tiles_n
    assert nblk > ncu and nblk % ncu == 0      # the launcher's own condition (tu_fp8k.hip launch_w4k)
    M, N = 256 * tiles_m, 256 * tiles_n
    x = _exact_inputs(oracle, M, N, K, seed=M + N + K)
    for form in (3, "mx"):
        _assert_baseline(capi, x, form)
        for raster in (1, 2):
            for stagger in (STAGGER_OFF, 0):
                for alpha in ALPHAS:
                    what = f"form {form} {(M, N, K)} hgemm_raster {raster} hgemm_stagger {stagger:#x} alpha {alpha}"
                    one = _launch(capi, x, form, alpha, stride=2048, hgemm_persist=0, hgemm_raster=raster, hgemm_stagger=stagger)
                    walk = _launch(capi, x, form, alpha, stride=2048, hgemm_persist=1, hgemm_raster=raster, hgemm_stagger=stagger)
                    _assert_exact(walk, one, what + ": persistent walk against one workgroup per tile")
                    _assert_exact(one, _want(x, form, alpha), what + " hgemm_persist 0")
                    _assert_exact(walk, _want(x, form, alpha), what + " hgemm_persist 1")


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("shape", [(256 * 17, 256 * 9), (256 * 33, 256 * 18), (1024, 1280)], ids=["17x9_tiles", "33x18_tiles", "4x5_tiles"])
def test_rasters_and_panel_widths_reach_every_tile(oracle, shape, K):
    """Both block -> tile maps on ragged tile grids (rows / columns of tiles no multiple of 16; fewer than 256 trailing blocks; a grid
    below one block per CU) with every form: under the block swizzle one-tile panels (swizzle_stride 256), a width that does not divide
    N (768 on 5 tile columns, 1280 on 9 and 18), the plain N-major raster (1) and a width beyond N (65536); under the XCD super-block
    raster one stride (the kernel ignores it).  The NaN prefill catches a tile no workgroup visits, exactness a tile computed with
    another tile's operand or scale base."""
    capi = _capi()
    M, N = shape
    x = _exact_inputs(oracle, M, N, K, seed=M + N + K)
    for form in FORMS:
        _assert_baseline(capi, x, form)
        for raster, stride in [(1, s) for s in (1, 256, 768, 1280, 65536)] + [(2, 1024)]:
            for alpha in ALPHAS:
                c = _launch(capi, x, form, alpha, stride=stride, hgemm_raster=raster)
                _assert_exact(c, _want(x, form, alpha), f"form {form} {(M, N, K)} hgemm_raster {raster} swizzle_stride {stride} alpha {alpha}")
