"""hgemm_w4y_kernel<false, 2>: the K loop that issues both k-steps of an accumulator block back to back (tools/gen_hgemm_w4y.py,
the pair loop) against schedule 1 (k-step outer) and the compiler-scheduled hgemm_w4x_kernel.  Same products, same order per
accumulator (k-step 0, then k-step 1, tile after tile): the results must be the same BITS.  Shapes: every exit of the body that is
unrolled over two K tiles, a full cycle of the 2-slot A / 3-slot B ring, the half-step tail behind an odd tile, and two C tiles per
persistent workgroup (the B register bank parity restarts at the seam)."""
import pytest
import torch

from leetcuda_amd import host
from tests import tol

pytestmark = pytest.mark.gpu

W4X, W4Y = 12, 13   # lc_hgemm_variant (lc_abi.h)
PLAIN = 1 << 27     # hgemm_stagger: every workgroup walks K from tile 0


def _capi():
    from leetcuda_amd import capi
    capi.load()
    return capi


def _tn(capi, a, bb, variant, sched=2, stagger=PLAIN):
    M, N = a.shape[0], bb.shape[1]   # host.as_col_major: shape [K, N], storage [N, K]
    c = torch.full((M, N), float("nan"), dtype=torch.half, device="cuda")
    capi.tune("hgemm_stagger", stagger)
    capi.tune("w4y_sched", sched)
    try:
        capi.hgemm(a, bb, c, layout=capi.LAYOUT_TN, variant=variant, swizzle_stride=2048)
        torch.cuda.synchronize()
    finally:
        capi.tune("w4y_sched", 2)
        capi.tune("hgemm_stagger", 0)
    return c


def _inputs(M, N, K):
    """Column k of A scaled by a ramp over K: a skipped, doubled or misplaced K tile shows in every element."""
    torch.manual_seed(M + 3 * N + 7 * K)
    ramp = 1.0 + torch.arange(K, device="cuda").float() / K
    a = (torch.randn(M, K, device="cuda") * ramp[None, :]).half()
    b = torch.randn(K, N, dtype=torch.half, device="cuda")
    return a, b, host.as_col_major(b)


def _same_bits(capi, M, N, K, stagger=PLAIN):
    a, b, bb = _inputs(M, N, K)
    assert capi.hgemm_kernel_name(M, N, K, capi.LAYOUT_TN, W4Y).startswith("hgemm_w4y_kernel<false,2>")
    got = _tn(capi, a, bb, W4Y, 2, stagger)
    assert torch.isfinite(got).all()
    assert torch.equal(got, _tn(capi, a, bb, W4Y, 1, stagger)), (M, N, K, "schedule 1")
    if K % 64 == 0 and stagger == PLAIN:
        assert torch.equal(got, _tn(capi, a, bb, W4X)), (M, N, K, "w4x")
    return a, b, got


@pytest.mark.parametrize("K", [64, 128, 192, 256, 448, 512])
def test_one_tile_every_exit_of_the_unrolled_body(K):
    """K = 64: the loop runs once and leaves after its first half; odd / even tile counts leave after the first / second half; 7 tiles
    (K = 448) walk one full cycle of the A ring (2 slots) against the B ring (3 slots)."""
    _same_bits(_capi(), 256, 256, K)


def test_half_step_tail_behind_an_odd_tile(oracle):
    capi = _capi()
    M, N, K = 256, 256, 480
    a, b, got = _same_bits(capi, M, N, K)
    rows = [0, 15, 16, 127, 128, 255]
    truth = oracle.hgemm(a[rows].contiguous(), b, len(rows), N, K, 0, "f32")
    ok, mx, _ = tol.hgemm_close(got[rows].float().cpu().numpy(), truth, K, 2.0)   # the ramp doubles the operand amplitude at most
    assert ok, mx


def test_two_tiles_one_launch():
    _same_bits(_capi(), 512, 256, 320)


@pytest.mark.parametrize("K", [192, 256])
def test_two_c_tiles_per_persistent_workgroup(K):
    """Tile count = 2 x the CU count: every workgroup computes two C tiles; the second starts again on B register bank 0, behind an
    odd (K = 192) and an even (K = 256) number of K tiles of the first."""
    capi = _capi()
    cus = capi.device_check()
    assert cus > 0
    _same_bits(capi, 512, 256 * cus, K)


def test_default_stagger_matches_schedule_1_under_the_same_stagger():
    _same_bits(_capi(), 1024, 1024, 448, stagger=0)
