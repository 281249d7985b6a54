"""Causal attention on inputs that pin the mask and the tile walk: every row carries ONE key that outweighs all others, so a single
wrong key — masked one too tight or too loose on any lane, a tile skipped, walked twice or taken from another head — moves that row by
far more than the bound, whichever row, lane or block it is in.  On randn inputs row i spreads its weight over i + 1 keys and a one-key
error sinks below the bound after a few dozen rows (tests/test_gpu_causal.py covers those inputs, every row).

Construction (build_inputs): K has random +-1 entries, Q_i = (SCORE / sqrt(D)) K[pi(i)], V is randn.  Key pi(i) scores SCORE = 12
natural units for row i, every other key about N(0, 144 / D); everything is exact in fp16 up to the one rounding of Q.  The maps pi:

  diag           i                       mask one too tight (j < i) on any lane: the row loses most of its weight.  Every row's running
                                         max rises in its diagonal tile, so the rescale runs inside the masked phase (in the merged-phase
                                         kernel's wave 0 three fully masked tiles follow it).
  next           min(i + 1, N - 1)       mask one too loose, or applied after the row max / exponential / overflow guard: the strongest
                                         key of every row is its first MASKED key.
  past           uniform in [0, i]       a plain tile skipped, walked twice or taken from another head, in any block (seeded per head)
  seam           64 (i // 64) - 1        the last key of the tile before the row's own (clipped to key 0)
  seam256_plain  256 (i // 256) - 1      the last plain key of the merged-phase kernel's block (clipped to key 0)
  seam256_diag   256 (i // 256)          its first diagonal key

Every row of every head is compared with the dense fp64 oracle (Oracle.attn_causal) under the project's bound for scores of many
units, |out - truth| <= 8e-3 + tol.ATTN_RTOL_SPIKE |truth| (test_overflow_slow_path_under_the_mask uses it with scores up to 16).

The CPU tests below (no gpu mark) prove on the same inputs, at the shapes the GPU tests run, that the inputs have teeth: an
off-by-one mask (the oracle's diag_offset = -1 / +1) moves EVERY row 1 .. N - 2 of `diag` / `next` by at least 20 x the bound, and
dropping the 64-key tile that holds pi(i) moves every row >= 1 of `past`, `seam` and `seam256_*` by at least 20 x the bound.

Measured worst |out - truth| per (kernel, D, map) over all N, both V layouts and all heads (MI355X; bound >= 8e-3):
  kernel        D             diag           next           past           seam  seam256_plain   seam256_diag
  merged-phase  64        3.01e-03       1.18e-03       3.18e-03       3.28e-03       1.98e-03       1.98e-03
  merged-phase  128       2.04e-03       1.36e-03       3.05e-03       2.08e-03       1.82e-03       1.89e-03
  lock-step     32        1.59e-03       1.11e-03       1.92e-03       1.72e-03       9.93e-04       1.94e-03
  lock-step     64        1.92e-03       1.18e-03       1.94e-03       1.91e-03       9.78e-04       9.78e-04
  lock-step     96        1.94e-03       9.77e-04       1.94e-03       9.78e-04       9.78e-04       9.79e-04
  lock-step     128       1.95e-03       1.02e-03       1.92e-03       1.94e-03       9.78e-04       1.89e-03
The largest |err| / bound over all cases is 0.14.  The floor of 9.8e-4 is the output's own rounding (half an fp16 ulp at 2 <= |O| < 4);
the 2e-3 to 3.3e-3 figures are the fp16 rounding of Q * scale * log2e at a score of 12 (tests/tol.py, ATTN_RTOL_SPIKE), larger in the
merged-phase kernel.  `lock-step` covers 2, 4 and 8 waves, D = 64 / 128 there being the forced cross-check ("attn_nw" = 8, 4, 2).
"""

import functools

import numpy as np
import pytest
import torch

from tests import tol
from tests.test_gpu_causal import _capi, _name, _want, report_worst_row

SCORE = 12.0      # natural units; the bound's atol was set for scores up to 16
ATOL = 8e-3
TEETH = 20.0      # an injected one-key / one-tile error must exceed the bound by this factor
BH = 3            # B x H: a head-index slip cannot cancel between two heads
MAPS = ("diag", "next", "past", "seam", "seam256_plain", "seam256_diag")
DS = (32, 64, 96, 128)
NS = (320, 384, 1024, 4096)


def target_map(name, N, seed):
    """pi: row -> the key that scores SCORE for it (int64 [N])"""
    i = torch.arange(N)
    if name == "diag":
        return i
    if name == "next":
        return (i + 1).clamp(max=N - 1)
    if name == "past":
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(N, generator=g, dtype=torch.float64) * (i + 1)).long().clamp(max=N - 1).minimum(i)
    if name == "seam":
        return (64 * (i // 64) - 1).clamp(min=0)
    if name == "seam256_plain":
        return (256 * (i // 256) - 1).clamp(min=0)
    if name == "seam256_diag":
        return 256 * (i // 256)
    raise KeyError(name)


@functools.lru_cache(maxsize=4)
def build_inputs(D, N, name):
    """(q, k, v, pi): fp16 CPU tensors [1, BH, N, D] and the maps [BH, N]; a different seed per head"""
    qs, ks, vs, pis = [], [], [], []
    for h in range(BH):
        seed = 1000003 * D + 101 * N + 7 * MAPS.index(name) + h
        g = torch.Generator().manual_seed(seed)
        k = (torch.randint(0, 2, (N, D), generator=g) * 2 - 1).to(torch.float32)
        v = torch.randn(N, D, generator=g)
        pi = target_map(name, N, seed + 1)
        qs.append((SCORE / D ** 0.5) * k[pi])
        ks.append(k)
        vs.append(v)
        pis.append(pi)
    q, k, v = (torch.stack(x).unsqueeze(0).half() for x in (qs, ks, vs))
    return q, k, v, torch.stack(pis)


@functools.lru_cache(maxsize=4)
def _truth(D, N, name):
    from tests import oracle_lib
    q, k, v, _ = build_inputs(D, N, name)
    return oracle_lib.load().attn_causal(q, k, v, 1, BH, N, D)


def _bound(truth):
    return ATOL + tol.ATTN_RTOL_SPIKE * np.abs(truth.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------------------
# teeth (CPU)

def _every_row_moves(truth, wrong, rows):
    """smallest over `rows` of the largest |wrong - truth| / bound over the row's columns, and the row it belongs to"""
    ratio = (np.abs(wrong.astype(np.float64) - truth) / _bound(truth)).max(axis=-1)[..., rows]     # [.., rows]
    flat = int(ratio.argmin())
    return float(ratio.min()), (flat // len(rows), rows[flat % len(rows)])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name,off", [("diag", -1), ("next", +1)])
def test_an_off_by_one_mask_moves_every_row(oracle, name, off, D, N):
    q, k, v, _ = build_inputs(D, N, name)
    truth = oracle.attn_causal(q, k, v, 1, BH, N, D)[0]
    wrong = oracle.attn_causal(q, k, v, 1, BH, N, D, diag_offset=off)[0]
    worst, where = _every_row_moves(truth, wrong, list(range(1, N - 1)))
    assert worst >= TEETH, (worst, where)


def _without_target_tile(q, k, v, pi):
    """(truth, wrong) in fp64, one head: causal attention, and the same with the weights of the 64-key tile that holds pi(i) zeroed
    before the row is normalised (what skipping that tile does); a row left with no key is zeros"""
    N, D = q.shape
    q, k, v = q.double(), k.double(), v.double()
    truth, wrong = torch.empty(N, D, dtype=torch.float64), torch.empty(N, D, dtype=torch.float64)
    j = torch.arange(N).view(1, N)
    for r0 in range(0, N, 512):
        i = torch.arange(r0, min(N, r0 + 512)).view(-1, 1)
        s = (q[r0:r0 + 512] @ k.T / D ** 0.5).masked_fill(j > i, -float("inf"))
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        truth[r0:r0 + 512] = (p / p.sum(-1, keepdim=True)) @ v
        p = p.masked_fill(j // 64 == (pi[r0:r0 + 512] // 64).view(-1, 1), 0.0)
        l = p.sum(-1, keepdim=True)
        wrong[r0:r0 + 512] = torch.where(l > 0, p / l.clamp(min=1e-300), torch.zeros_like(p)) @ v
    return truth.numpy(), wrong.numpy()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", ["past", "seam", "seam256_plain", "seam256_diag"])
def test_dropping_the_target_tile_moves_every_row(oracle, name, D, N):
    q, k, v, pi = build_inputs(D, N, name)
    dense = oracle.attn_causal(q, k, v, 1, BH, N, D)[0]
    for h in range(BH):
        truth, wrong = _without_target_tile(q[0, h], k[0, h], v[0, h], pi[h])
        assert np.abs(truth - dense[h]).max() <= 1e-6      # (the fp64 torch restatement is the oracle's definition)
        worst, where = _every_row_moves(truth, wrong, list(range(1, N)))
        assert worst >= TEETH, (h, worst, where)


def test_the_inputs_are_what_the_docstring_says():
    for name in MAPS:
        q, k, v, pi = build_inputs(64, 1024, name)
        assert (pi <= torch.arange(1024)).all() or name == "next"
        assert (k.abs() == 1).all() and torch.isfinite(v).all()
        s = (q[0].double() @ k[0].double().transpose(-2, -1)) / 8.0
        hit = s.gather(-1, pi.unsqueeze(-1)).squeeze(-1)
        assert (hit - SCORE).abs().max().item() <= SCORE * 2.0 ** -11      # the one rounding of Q
        assert s.max().item() <= 16.0
        assert not torch.equal(k[0, 0], k[0, 1]) and not torch.equal(v[0, 1], v[0, 2])      # a seed per head
    i = torch.arange(4096)
    assert torch.equal(target_map("seam", 4096, 0)[[0, 63, 64, 127, 4095]], torch.tensor([0, 0, 63, 63, 4031]))
    assert torch.equal(target_map("seam256_plain", 4096, 0)[[0, 255, 256, 4095]], torch.tensor([0, 0, 255, 3839]))
    assert torch.equal(target_map("seam256_diag", 4096, 0)[[0, 255, 256, 4095]], torch.tensor([0, 0, 256, 3840]))
    past = target_map("past", 4096, 5)
    assert (past <= i).all() and (past >= 0).all() and past[0] == 0 and (past[2048:] < 1024).any() and (past[2048:] >= 2048).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernels (GPU)

def _run_case(capi, D, N, vt, name, want):
    assert _name(capi, N, D, vt, BH) == want
    q, k, v, _ = build_inputs(D, N, name)
    truth = _truth(D, N, name)
    qg, kg, vg = (x.cuda() for x in (q, k, v))
    o = torch.full_like(qg, float("nan"))
    capi.attn_fwd(qg, kg, vg.transpose(-2, -1).contiguous() if vt else vg, o, v_transposed=vt, causal=True)
    torch.cuda.synchronize()
    out = o.float().cpu().numpy()
    err = np.abs(out.astype(np.float64) - truth)
    print(f"[causal_mask] {want} N={N} {name}: worst err {np.nanmax(err):.3e}, worst err / bound {np.nanmax(err / _bound(truth)):.3f}")
    assert np.isfinite(out).all(), report_worst_row(np.where(np.isfinite(out), 0.0, 1.0)[0], want)
    excess = err - _bound(truth)
    assert (excess <= 0).all(), report_worst_row(excess[0], want, err[0])


@pytest.mark.gpu
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", DS)
def test_every_row_with_one_dominant_key(D, N, name, vt):
    _run_case(_capi(), D, N, vt, name, _want(N, D, vt))


@pytest.mark.gpu
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("nw", [8, 4, 2])
@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("N", [1024, 4096])
@pytest.mark.parametrize("D", [64, 128])
def test_every_row_with_one_dominant_key_on_the_cross_check_kernel(D, N, name, nw, vt):
    capi = _capi()
    capi.tune("attn_nw", nw)
    try:
        _run_case(capi, D, N, vt, name, f"attn_fwd_causal_kernel<{D},{nw},{'true' if vt else 'false'}>")
    finally:
        capi.tune("attn_nw", 0)
