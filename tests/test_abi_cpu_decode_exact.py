"""The teeth tests of the inputs of tests/test_gpu_decode_exact.py; the inputs, truths, bounds and the fault locator themselves, which this
docstring describes, are in tests/decode_lib.py (there pinned_inputs, PIN_LENS and PLACES carry the prefix exact_ / EXACT_).  Decode attention (attn_decode_kernel<D,RT>,
attn_decode_combine_kernel<D> and attn_decode_paged_kernel<D,RT>) on inputs whose answer is exact, pinned to one key or moved by a score
step.  No call here reaches a device.  Ncap = 1024, D in {64, 128}; one launch carries one batch entry per length; every (batch entry, K / V
head) pair has its own seed, so a head or batch slip cannot cancel.  Row r = g Nq + i of a K / V head is query head kvh G + g, token i.

Truths are fp64 torch straight from the definition (bottom-right aligned mask: token i of entry b sees keys 0 .. L_b - Nq + i; head map
h // G; zeros for a row without a visible key), anchored to the project's oracle (decode_lib.decode_truth) on a handful of rows per
class to 1e-6.  Three input classes, each blind where another sees:

  uniform   even K / V heads: Q = 0, K random +-1; odd K / V heads: Q random +-1, K = 0.  Every score is exactly 0, every visible key has
            weight exactly 1 and row (b, h, i) is the mean E of V[0 : nk].  V is drawn from test_gpu_attn_exact.V16 (the eight values of V8,
            weighted to mean 0) at EVERY position below Ncap, so the first invisible key carries a set value too.  Every partial sum is a
            multiple of 1/4 below 2^13: exact in fp32 in any order, so l = nk and the O accumulators are exact in every wave, range and order.
            Bounds, ulp16(x) the fp16 spacing at |x| (2^-24 below 2^-14):
              S = 1   |out - E| < ulp16(E); for nk a power of two out is BIT-EQUAL to E rounded once (the reciprocal is exact too)
              S > 1   |out - E| <= ulp16(max(|E|, 2^-6)).  The partial means are fp32 and the weights pass through the device's log2f and
                      exp2 in fp32.  ASSUMPTION (never measured in this project): both are within 8 fp32 ulps; then a weight is off by at
                      most ~2^-18 relative (lse <= 10, 8 ulps of it are 2^-19 absolute, as much again for exp2) and the combine's error is
                      below 2^-18 max|v| = 2^-17; the floor of ulp16(2^-6) = 2^-16 covers it beside the output's rounding.
            A key counted 0 or 2 times moves a column by |v - E| / (nk -+ 1).  Cannot see: which key carries which weight, a wrong rescale.
  pinned    decode_lib.pinned_inputs' construction for any (H, Hkv, Nq) and any lengths: K random +-1, Q_row = (12 / sqrt(D)) K[target],
            V randn; key `target` scores 12 for its row and every other key at most 12 |cos| <= 12.  Places (pin_target, unchanged): last,
            first_invisible (its target t carries the V row 8 K[t]: +-8 with the key's own signs — with one fixed +-8 pattern, as in
            decode_lib.pinned_inputs, token i + 1 sees the target of token i under the causal mask, at Nq = 64 nearly every visible V row is
            that pattern and the row sits on it before the mask is wrong), key0, tile_seam, range_seam — and step_seam: key 64 t + 31 for even r, 64 t + 32
            for odd r, t the last tile that holds both below the row's limit: the seam between the two 32-key pipeline steps of
            attn_decode_kernel<128,4>, the only instantiation with STEP = 32.  Rows without a target keep randn.  Bound: check_decode.
            Cannot see: a block walked twice, a skipped block that is not the target's, a wrong rescale (the dominant key renormalises).
  step      per (b, K / V head) a tile t* drawn from [ceil(T_b / 4), floor((L_b - Nq + 1) / 64)), T_b = ceil(L_b / 64) (L = 130: t* = 0 unless
            Nq = 1); K[j] = u (random +-1) for the 40
            keys [64 t* + 24, 64 t* + 64) and 0 elsewhere, Q_r = (c_r / sqrt(D)) u with c_r = (2, 3, 4)[r % 3]; V from V8, the 40 step keys
            sharing one V row w (test_gpu_attn_exact.py says why).  The wave that owns t* raises its max in mid-walk (alpha != 1 behind the
            ballot), the other waves rescale in the merge, and under S > 1 the range that holds t* outweighs the others in the combine.
            The draw stops below the smallest causal limit of the entry and not at T_b: the ragged last tile of L = 1000 holds 16 of its
            40 step keys, that of L = 577 and L = 130 none, and under the causal mask the first tokens of Nq = 64 would see a few step
            keys or none — a row without a step key has no rescale anywhere and one with a few is moved by less than 20 bounds when the
            combine's weights are wrong (measured: 6 ... 14).  So every row of every launch, causal or not, sees all 40.
            Bound: tol.attn_close(N = nk, rtol = tol.ATTN_RTOL_SPIKE).  Cannot see: a dropped or doubled plain block.

Teeth (factor TEETH = 20 over the row's bound, in at least one column of EVERY row a fault touches; fp64, at exactly the GPU tests' shapes):
  uniform   limit +- 1 at every nk; token offset +- 1 under causal; a dropped and a doubled 16-, 32- and 64-key block at every block index
            for the lengths 1024, 1000, 577, 130 — each against the S = 1 and the S > 1 bound.  The fp64 mean rounded once to fp16 stays
            strictly inside ulp16(E): the reference alone never fails.
  pinned    zeroing the weights of the 16-key block that holds the target, every place, every row shape.  For first_invisible the target
            has weight 0 in the truth and zeroing its block cannot touch it: there the fault is the block becoming visible up to the target.
  step      an fp64 emulation of the kernel's structure (ranges [s T / S, (s + 1) T / S), tile t of a range on wave (t - t0) mod 4, steps of
            STEP keys, the merge through (m, l) and `mine`, the combine) with alpha left out of l, alpha left out of O, `mine` left out for
            one wave and all combine weights equal.  A fault APPLIES to a row when the factor it drops differs from 1 there and scales
            something: alpha faults need an earlier tile of the owning wave in the same range (t* - t0 >= 4: S = 1 at L >= 577, S = 2 at
            L >= 1000); `mine` of a wave is judged on the rows that see the wave's first tile of the range whole (a causal row may see one
            plain key of a tile behind t*, too little to move it); the combine fault needs a visible step key, two ranges with a visible key, one of
            them with a true share of the weight at least 1/16 away from 1 / ranges (equal weights are nearly RIGHT for a causal row of
            L = 1000, Nq = 64, S = 2 that sees 17 of the 40 step keys: the ranges weigh 512 : 533).  Each fault moves
            every row it applies to, and the test asserts that each applies somewhere at every row shape and head dim.
The fault locator names kernel, batch entry, K / V head, group member g, token i, nk and the share of wrong elements, and for `uniform` the
closest one-fault hypothesis (the mean recomputed under: limit one key short / long, the limit of token i +- 1, a key block of 16 / 32 / 64
dropped / doubled, a wave's tiles dropped, a range dropped / doubled, K / V head h % Hkv, batch 0); a CPU test feeds it each injected fault.
"""
import math

import numpy as np
import pytest
import torch

from tests.decode_lib import EXACT_PIN_LENS as PIN_LENS
from tests.decode_lib import EXACT_PLACES as PLACES
from tests.decode_lib import NCAP_POW2 as NCAP
from tests.decode_lib import (BLOCK_LENS, DS, FLOOR, GRID, LENS, PAGE_SIZES, PINNED_SPLITS, ROW_SHAPES, SCORE, STEP_FAULTS, STEP_LENS, STEP_SPLITS, TEETH,
                              UNIFORM_SPLITS, attend64, decode_bound, decode_truth, emulate_kernel, gather, judge, locate_uniform, paginate,
                              pinned_split_key, pinned_truth, prefix_sums, rt_of, step_bound, step_inputs, step_of, step_truth, target_of, truth64,
                              ulp16, uniform_bound, uniform_hint, uniform_hypotheses, uniform_inputs, uniform_means, uniform_truth, visible, weights64)
from tests.decode_lib import exact_pinned_inputs as pinned_inputs
from tests.test_gpu_attn_exact import STEP_C, V8, V16, round_once

# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs are what the docstring says

def test_the_value_set_sums_exactly_in_any_order():
    assert set(V16) == set(V8) and sum(V16) == 0 and len(V16) == 16
    for x in V8:
        assert 4 * x == round(4 * x) and abs(x) <= 2 and float(torch.tensor(x).half()) == x      # multiples of 1/4, exact in fp16
    assert 4 * 2 * NCAP <= 2 ** 13 < 2 ** 24              # |any partial sum| <= 2 Ncap = 2^11 < 2^13, in quarters an integer below 2^24: exact in fp32
    assert ulp16(1.0) == 2.0 ** -10 and ulp16(2.0 ** -15) == 2.0 ** -24 and ulp16(0.0) == 2.0 ** -24 and ulp16(FLOOR) == 2.0 ** -16


@pytest.mark.parametrize("H,Hkv,Nq", GRID)
@pytest.mark.parametrize("D", DS)
def test_uniform_inputs_are_what_the_docstring_says(D, H, Hkv, Nq):
    q, k, v = uniform_inputs(D, H, Hkv, Nq)
    G = H // Hkv
    s = q.double() @ k.double()[:, torch.arange(H) // G].transpose(-2, -1)
    assert (s == 0).all()
    for kvh in range(Hkv):
        qs = q[:, kvh * G:(kvh + 1) * G]
        assert ((qs == 0).all() and (k[:, kvh].abs() == 1).all()) if kvh % 2 == 0 else ((qs.abs() == 1).all() and (k[:, kvh] == 0).all())
    assert set(v.double().unique().tolist()) <= set(V8)                       # at EVERY position below Ncap
    flat = v.reshape(-1, NCAP, D)
    assert all(not torch.equal(flat[0], flat[j]) for j in range(1, flat.shape[0]))      # a seed per (b, K / V head)
    for causal in (False, True):
        E, nks, P = uniform_truth(D, H, Hkv, Nq, causal)
        assert (np.abs(round_once(E, False) - E) < ulp16(E)).all()            # the reference alone stays inside the bound
        assert nks.min() == 0 and nks.max() == NCAP
        if causal and Nq > 1:
            assert (nks[LENS.index(1)] == [0] * (Nq - 1) + [1]).all()
    assert (P * 4 == np.round(P * 4)).all() and np.abs(P).max() < 2 ** 13


@pytest.mark.parametrize("H,Hkv,Nq", ROW_SHAPES)
@pytest.mark.parametrize("D", DS)
def test_pinned_inputs_are_what_the_docstring_says(D, H, Hkv, Nq):
    G = H // Hkv
    for causal in (False, True):
        for place in PLACES:
            q, k, v, targets = pinned_inputs(D, place, causal, H, Hkv, Nq)
            assert (k.abs() == 1).all() and torch.isfinite(v).all()
            s = q.double() @ k.double()[:, torch.arange(H) // G].transpose(-2, -1) / D ** 0.5
            hits = 0
            for b, L in enumerate(PIN_LENS):
                for h in range(H):
                    for i in range(Nq):
                        t = targets[b][h][i]
                        if t is None:
                            continue
                        hits += 1
                        row = s[b, h, i].clone()
                        assert abs(row[t].item() - SCORE) <= 2.0 ** -11 * SCORE
                        row[t] = -1e9
                        assert row.max().item() <= 16.0 and row.max().item() < SCORE - 1
                        lim = visible(L, Nq, NCAP, causal, i)
                        assert (t == lim) if place == "first_invisible" else (0 <= t < lim)
                        if place == "first_invisible":
                            assert v[b, h // G, t].abs().min().item() == 8.0
                        if place == "step_seam":
                            assert t % 64 == (31 if ((h % G) * Nq + i) % 2 == 0 else 32) and (t // 64) * 64 + 32 < lim <= (t // 64) * 64 + 96
            assert hits > 0, place
            if place in ("last", "key0") and not causal:
                assert hits == len(PIN_LENS) * H * Nq
    sides = {target_of("step_seam", 577, Nq, False, r, 3) % 64 for r in range(G * Nq)}
    assert sides == ({31, 32} if G * Nq > 1 else {31})


@pytest.mark.parametrize("H,Hkv,Nq", ROW_SHAPES)
@pytest.mark.parametrize("D", DS)
def test_step_inputs_are_what_the_docstring_says(D, H, Hkv, Nq):
    q, k, v, tiles = step_inputs(D, H, Hkv, Nq)
    G = H // Hkv
    s = q.double() @ k.double()[:, torch.arange(H) // G].transpose(-2, -1) / D ** 0.5
    assert set(v.double().unique().tolist()) <= set(V8)
    for b, L in enumerate(STEP_LENS):
        T = -(-L // 64)
        for kvh in range(Hkv):
            t = tiles[b][kvh]
            lo, hi = 64 * t + 24, 64 * t + 64
            assert (T / 4 <= t or (L == 130 and t == 0)) and hi <= L - Nq + 1 and hi - lo == 40      # below every row's limit, causal or not
            assert (v[b, kvh, lo:hi] == v[b, kvh, lo]).all()
            for g in range(G):
                for i in range(Nq):
                    c = STEP_C[(g * Nq + i) % 3]
                    row = s[b, kvh * G + g, i]
                    assert ((row[lo:hi] - c).abs() <= c * 2.0 ** -11).all() and (row[:lo] == 0).all() and (row[hi:] == 0).all()
    every = [t for row in tiles for t in row]
    assert len(every) == 1 or len(set(every)) > 1


def test_the_fp64_torch_truths_are_the_oracles(oracle):
    """the anchor: on a handful of rows per class the project's oracle says what the fp64 torch restatement says"""
    D, (H, Hkv, Nq) = 64, (6, 2, 5)
    G = H // Hkv
    rows = ((0, 0, 0), (1, 5, 4), (3, 2, 1), (4, 3, 0), (10, 4, 4), (11, 1, 2))           # (b, h, i) over LENS; the last two: one key / none
    for causal in (False, True):
        cases = [("uniform", uniform_inputs(D, H, Hkv, Nq), LENS, uniform_truth(D, H, Hkv, Nq, causal)[0]),
                 ("pinned", pinned_inputs(D, "step_seam", causal, H, Hkv, Nq)[:3], PIN_LENS, pinned_truth(D, "step_seam", causal, H, Hkv, Nq)[0]),
                 ("step", step_inputs(D, H, Hkv, Nq)[:3], STEP_LENS, step_truth(D, H, Hkv, Nq, causal)[0])]
        for cls, (q, k, v), lens, mine in cases:
            for b, h, i in rows:
                b = b % len(lens)
                one = (q[b:b + 1, h:h + 1], k[b:b + 1, h // G:h // G + 1], v[b:b + 1, h // G:h // G + 1])
                want, nks = decode_truth(oracle, *one, [lens[b]], causal)
                assert int(nks[0, i]) == visible(lens[b], Nq, NCAP, causal, i)
                assert np.abs(want[0, 0, i] - mine[b, h, i]).max() <= 1e-6, (cls, causal, b, h, i)
            if cls == "uniform":                       # the direct softmax agrees with the prefix-sum mean everywhere
                assert np.abs(truth64(q, k, v, lens, causal)[0] - mine).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------------
# teeth

def _both_bounds(E):
    return (("S = 1", uniform_bound(E, 1)), ("S > 1", uniform_bound(E, 2)))


def _assert_moved(what, wrong, E, touched):
    """every touched row [B,H,Nq] moves by >= TEETH x its bound in at least one column, under both of `uniform`'s bounds"""
    assert touched.any(), what
    for which, bound in _both_bounds(E):
        ratio = (np.abs(wrong - E) / bound).max(axis=-1)
        assert ratio[touched].min() >= TEETH, (what, which, float(ratio[touched].min()), np.argwhere(touched & (ratio < TEETH))[:4].tolist())


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("H,Hkv,Nq", GRID)
@pytest.mark.parametrize("D", DS)
def test_uniform_one_key_or_one_token_off_moves_every_row(D, H, Hkv, Nq, causal):
    E, nks, P = uniform_truth(D, H, Hkv, Nq, causal)
    B = len(LENS)
    full = np.ones((B, H, Nq), bool)
    short, long_ = np.maximum(nks - 1, 0), np.minimum(nks + 1, NCAP)
    _assert_moved("limit one key short", uniform_means(P, short, H), E, full & (short != nks)[:, None, :])
    _assert_moved("limit one key long", uniform_means(P, long_, H), E, full & (long_ != nks)[:, None, :])
    assert (short != nks).sum() == (nks > 0).sum() and (long_ != nks).sum() == (nks < NCAP).sum()       # at every nk there is
    if causal:
        for d in (-1, 1):
            off = np.array([[min(visible(L, Nq, NCAP, True, i + d), NCAP) for i in range(Nq)] for L in LENS])
            _assert_moved(f"the limit of token i {d:+d}", uniform_means(P, off, H), E, full & (off != nks)[:, None, :])


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("H,Hkv,Nq", GRID)
@pytest.mark.parametrize("D", DS)
def test_uniform_a_block_dropped_or_doubled_moves_every_row(D, H, Hkv, Nq, causal):
    E, nks, P = uniform_truth(D, H, Hkv, Nq, causal)
    G = H // Hkv
    seen = 0
    for b, L in enumerate(LENS):
        if L not in BLOCK_LENS:
            continue
        for i in range(Nq):
            nk = int(nks[b, i])
            for size in (16, 32, 64):
                edges = np.minimum(np.arange(0, nk + size, size), nk)
                edges = edges[:-(-nk // size) + 1]
                cnt = np.diff(edges)[None, :, None].astype(np.float64)                    # [1, blocks, 1]
                seg = P[b][:, edges[1:]] - P[b][:, edges[:-1]]                             # [Hkv, blocks, D]
                tot = P[b][:, nk][:, None, :]
                want = (tot / nk)
                assert (cnt > 0).all() and nk > size
                for what, wrong in (("dropped", (tot - seg) / (nk - cnt)), ("doubled", (tot + seg) / (nk + cnt))):
                    for which, bound in _both_bounds(want):
                        ratio = (np.abs(wrong - want) / bound).max(axis=-1)                # [Hkv, blocks]
                        assert ratio.min() >= TEETH, (what, which, size, b, i, nk, float(ratio.min()), np.unravel_index(ratio.argmin(), ratio.shape))
                seen += seg.shape[1]
            assert np.array_equal(P[b][np.arange(H) // G, nk] / nk, E[b, :, i])           # `want` above is the test's E
    assert seen > 0


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("H,Hkv,Nq", ROW_SHAPES)
@pytest.mark.parametrize("D", DS)
def test_pinned_losing_the_target_block_moves_every_row(D, H, Hkv, Nq, causal):
    j = torch.arange(NCAP)
    for place in PLACES:
        for split in sorted({pinned_split_key(place, s) for s in PINNED_SPLITS}):
            q, k, v, targets = pinned_inputs(D, place, causal, H, Hkv, Nq, split)
            p, nks = weights64(q, k, PIN_LENS, causal)
            truth = attend64(p, v, H)
            tgt = torch.tensor([[[-1 if t is None else t for t in row] for row in hb] for hb in targets])      # [B, H, Nq]
            has = (tgt >= 0).numpy()
            assert has.any(), place
            in_block = (j.view(1, 1, 1, -1) // 16 == (tgt // 16).unsqueeze(-1)) & (tgt >= 0).unsqueeze(-1)
            if place == "first_invisible":             # the target's block becomes visible up to the target
                s_all = q.double() @ k.double()[:, torch.arange(H) // (H // Hkv)].transpose(-2, -1) / D ** 0.5
                vis2 = (j.view(1, 1, 1, -1) < torch.from_numpy(nks).view(len(PIN_LENS), 1, Nq, 1)) | (in_block & (j.view(1, 1, 1, -1) <= tgt.unsqueeze(-1)))
                s2 = s_all.masked_fill(~vis2, -float("inf"))
                mx = s2.max(dim=-1, keepdim=True).values
                p2 = torch.exp(s2 - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
            else:
                p2 = p.masked_fill(in_block, 0.0)
            wrong = attend64(p2, v, H)
            bound = decode_bound(truth, nks)
            ratio = (np.abs(wrong - truth) / bound).max(axis=-1)
            zero = np.broadcast_to((nks == 0)[:, None, :], ratio.shape)
            ratio = np.where(zero & (np.abs(wrong).max(axis=-1) > 0), np.inf, ratio)      # a row that must be exactly 0 and is not
            assert ratio[has].min() >= TEETH, (place, split, float(ratio[has].min()), np.argwhere(has & (ratio < TEETH))[:4].tolist())
            assert ratio[~has].max(initial=0.0) == 0.0


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("H,Hkv,Nq", ROW_SHAPES)
@pytest.mark.parametrize("D", DS)
def test_step_a_rescale_left_out_moves_every_row_it_applies_to(D, H, Hkv, Nq, causal):
    q, k, v, tiles = step_inputs(D, H, Hkv, Nq)
    truth, nks = step_truth(D, H, Hkv, Nq, causal)
    bound = step_bound(truth, nks)
    G, STEP = H // Hkv, step_of(D, H, Hkv, Nq)
    applied = {f: 0 for f in STEP_FAULTS}
    for S in STEP_SPLITS:
        for b, L in enumerate(STEP_LENS):
            for kvh in range(Hkv):
                hs = slice(kvh * G, (kvh + 1) * G)
                s = (q[b, hs].double().reshape(G * Nq, D) @ k[b, kvh].double().T) / D ** 0.5
                lims = torch.from_numpy(nks[b]).repeat(G)
                t64, bd = truth[b, hs].reshape(G * Nq, D), bound[b, hs].reshape(G * Nq, D)
                vv = v[b, kvh].double()
                right, _ = emulate_kernel(s, vv, lims, L, S, STEP)
                assert np.abs(right - t64).max() <= 1e-12, (S, b, kvh)                     # the emulation without a fault is the truth
                for fault in STEP_FAULTS:
                    if fault == "combine" and S == 1:
                        continue
                    wrong, applies = emulate_kernel(s, vv, lims, L, S, STEP, fault)
                    ratio = (np.abs(wrong - t64) / bd).max(axis=-1)
                    applied[fault] += int(applies.sum())
                    if applies.any():
                        assert ratio[applies].min() >= TEETH, (fault, S, b, kvh, tiles[b][kvh], float(ratio[applies].min()), int(ratio[applies].argmin()))
                    if fault != "combine":
                        assert ratio[~applies].max(initial=0.0) <= 1e-9, (fault, S, b, kvh)
                    if fault in ("alpha_l", "alpha_o") and S == 1 and not causal:
                        assert applies.all() == (tiles[b][kvh] >= 4), (fault, b, kvh, tiles[b][kvh])
    assert applied["alpha_l"] > 0 and applied["alpha_o"] > 0 and applied["combine"] > 0
    assert sum(applied[f] for f in STEP_FAULTS if isinstance(f, tuple)) > 0, applied


# ------------------------------------------------------------------------------------------------------------------------------------
# the locator

def _mean_under(v, counts):
    """the mean of V rows under per-key counts [Ncap] (0: dropped, 2: walked twice), rounded to fp16 as a kernel's output would be"""
    return round_once((counts.double() @ v.double()).numpy() / float(counts.sum()), False)


def test_the_locator_names_each_injected_fault():
    D, (H, Hkv, Nq) = 64, (6, 2, 5)
    G = H // Hkv
    _, _, v = uniform_inputs(D, H, Hkv, Nq)
    P = prefix_sums(v)
    j = torch.arange(NCAP)
    b, h, i = LENS.index(577), 4, 2                      # K / V head 1, g 1
    kvh = h // G
    for causal in (False, True):
        nk = visible(577, Nq, NCAP, causal, i)
        base = (j < nk).long()
        T = 10

        def block(size, t):
            return ((j // size == t) & (j < nk)).long()

        wave2 = (((j // 64) % 4 == 2) & (j < nk)).long()
        rng1 = ((j // 64 >= 1 * T // 3) & (j // 64 < 2 * T // 3) & (j < nk)).long()
        faults = [(1, "limit one key short", v[b, kvh], (j < nk - 1).long()),
                  (1, "limit one key long", v[b, kvh], (j < nk + 1).long()),
                  (1, "16-key block 5 dropped", v[b, kvh], base - block(16, 5)),
                  (1, "16-key block 35 doubled", v[b, kvh], base + block(16, 35)),
                  (1, "32-key block 3 doubled", v[b, kvh], base + block(32, 3)),
                  (1, "32-key block 17 dropped", v[b, kvh], base - block(32, 17)),
                  (1, "64-key block 2 dropped", v[b, kvh], base - block(64, 2)),
                  (3, "64-key block 7 doubled", v[b, kvh], base + block(64, 7)),
                  (1, "wave 2's tiles dropped", v[b, kvh], base - wave2),
                  (3, "range 1 of 3 dropped", v[b, kvh], base - rng1),
                  (3, "range 1 of 3 doubled", v[b, kvh], base + rng1),
                  (2, "wave 0's tiles dropped in range 0 of 2", v[b, kvh], base - (((j // 64 == 0) | (j // 64 == 4)) & (j < nk)).long()),
                  (1, "K / V head h % Hkv = 0", v[b, h % Hkv], base),
                  (3, "batch entry 0's cache", v[0, kvh], base)]
        if causal:
            faults += [(1, "the limit of token 1 (wrong r % Nq)", v[b, kvh], (j < nk - 1).long()),
                       (1, "the limit of token 3 (wrong r % Nq)", v[b, kvh], (j < nk + 1).long())]
        for S, name, vsrc, counts in faults:
            row = _mean_under(vsrc, counts)
            got, res = locate_uniform(row, P, LENS, H, Hkv, Nq, causal, S, b, h, i)
            hyps = dict(uniform_hypotheses(P, LENS, H, Hkv, Nq, causal, S, b, h, i))
            assert name in hyps, (name, sorted(hyps)[:5])
            assert np.abs(hyps[name] - row).max() <= ulp16(row).max(), name              # the named hypothesis restates the injected fault
            assert res <= ulp16(row).max() and np.abs(hyps[got] - hyps[name]).max() == 0.0, (causal, S, name, got, res)
            if "token" not in name and "one key" not in name:
                assert got == name, (causal, S, name, got)
        # the judge's message names where the failure is
        E, nks, _ = uniform_truth(D, H, Hkv, Nq, causal)
        out = round_once(E, False)
        assert judge("k", "uniform", out, E, uniform_bound(E, 1), nks, Hkv, strict=True) <= 0.5
        out[b, h, i] = _mean_under(v[b, kvh], base - block(32, 3))
        with pytest.raises(AssertionError) as e:
            judge("attn_decode_kernel<64,1>", "uniform", out, E, uniform_bound(E, 1), nks, Hkv, strict=True,
                  hint=uniform_hint(out, P, LENS, H, Hkv, Nq, causal, 1))
        msg = str(e.value)
        for piece in ("attn_decode_kernel<64,1>", f"batch entry {b}", "K / V head 1", "g 1", f"token {i}", f"nk {nk}", "of all elements",
                      "32-key block 3 dropped"):
            assert piece in msg, (piece, msg)
        out = round_once(E, False)
        out[LENS.index(0), 0, 0, 3] = 2.0 ** -24         # a row without a visible key must be exactly 0
        with pytest.raises(AssertionError, match="nk 0"):
            judge("k", "uniform", out, E, uniform_bound(E, 1), nks, Hkv, strict=True)
        out = round_once(E, False)
        out[0, 0, 0, 0] = float("nan")                   # never written
        with pytest.raises(AssertionError, match="batch entry 0"):
            judge("k", "uniform", out, E, uniform_bound(E, 64), nks, Hkv)


def test_paged_pools_hold_the_same_cache():
    """paginate / gather on the exact inputs: the gathered cache is the contiguous one below L_b and NaN from there on"""
    q, k, v = uniform_inputs(64, 8, 1, 1)
    for ps in PAGE_SIZES:
        kp, vp, table = paginate(k, v, LENS, ps, seed=ps)
        for pool, x in ((kp, k), (vp, v)):
            back = gather(pool, table)
            for b, L in enumerate(LENS):
                assert torch.equal(back[b, :, :L], x[b, :, :L]) and torch.isnan(back[b, :, L:]).all()


def test_every_instantiation_is_named_under_every_class(built):
    """the plan needs no GPU: the row shapes reach every (D, RT) under every class, <128,4> among step_seam's, with the x S suffix"""
    from leetcuda_amd import capi
    capi.load()
    want = {(D, rt) for D in DS for rt in (1, 2, 4)}
    try:
        for shapes, lens, splits in ((GRID, LENS, UNIFORM_SPLITS), (ROW_SHAPES, PIN_LENS, PINNED_SPLITS), (ROW_SHAPES, STEP_LENS, STEP_SPLITS)):
            seen = set()
            for D in DS:
                for H, Hkv, Nq in shapes:
                    for S in splits:
                        capi.tune("attn_decode_split", S)
                        name = capi.attn_decode_kernel_name(len(lens), H, Hkv, Nq, NCAP, D)
                        assert name == f"attn_decode_kernel<{D},{rt_of(H, Hkv, Nq)}>" + (f" x{S}" if S > 1 else "")
                        seen.add((D, rt_of(H, Hkv, Nq)))
            assert seen == want
        assert [(G * Nq, rt_of(H, Hkv, Nq)) for H, Hkv, Nq in GRID for G in [H // Hkv]] == \
            [(1, 1), (8, 1), (15, 1), (17, 2), (32, 2), (33, 4), (36, 4), (48, 4), (63, 4), (64, 4)]
        assert math.prod(s in GRID for s in ROW_SHAPES) and step_of(128, 8, 2, 9) == 32 and step_of(64, 8, 2, 9) == 64 and step_of(128, 2, 2, 17) == 64
    finally:
        capi.tune("attn_decode_split", 0)
