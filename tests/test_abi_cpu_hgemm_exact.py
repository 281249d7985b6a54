"""Exact-sum inputs for the fp16 HGEMM, their reference, a fault locator — and CPU tests that the inputs have teeth.  No call here reaches a
device; tests/test_gpu_hgemm_exact.py imports the builders, the reference and the locator from this module.

Two input classes, each from a seeded generator (numpy, on the CPU: both files test the same inputs):

  signed   A and B uniform over {+-0.5, +-1, +-1.5, +-2}: no zeros, so every single k contributes to every element of C.
  biased   A and B uniform over {0.5, 1, 1.5, 2}: |C| grows like 1.56 K, so from K ~ 350 on most outputs need rounding (the fp16 spacing at
           |C| >= 512 is 0.5) and the odd multiples of 1/4 land on ties.

Every product is a multiple of 1/4, and while  max(|A| . |B|) * 4 < 2^24  every partial sum of every element, in ANY order and ANY grouping,
is an integer below 2^24 in units of 1/4: exact in fp32.  The builder asserts the condition through its upper bound 4 K max|A| max|B| (= 16 K:
K < 2^20); measured with these value sets at K = 4192: 27 289 (`signed`) and 27 418 (`biased`), 4 x the largest element of |A| . |B|.  K <= 8224 keeps |C| <= 4 K
below 65504.  So whatever the summation order, the split-K factor, the stagger or the tile shape, a correct kernel stores the exact product
rounded ONCE to fp16, to nearest even: the reference is the fp64 product of the same operands, `.astype(float16)` (numpy; on the device in
torch.float64 for large shapes — both are exact here), and it equals oracle.hgemm(..., "exact") bit for bit (checked below).

Teeth, measured on the CPU with exactly these generators at M = N = 256 (share of elements whose BITS change when the fault is applied to
the reference alone; K = 96 / 352 / 1056 / 4192):

  fault                                            signed                                  biased
  one 32-slice dropped or doubled (first, middle,  0.990 ... 0.9915 (the same share for       1.0 at every K
    last slice)                                    "dropped" and "doubled")
  one single k dropped (first, middle, last k)     1.0 at every K                          (not asserted)
  round-toward-zero conversion                     0 at every K                            0 / 0.2463 / 0.3746 / 0.4673
  first half of K held as an fp16 partial          0 at every K                            0 / 0 / 0.1246 / 0.1259

The `signed` class changes no element under the two rounding faults — its |C| ~ 1.9 sqrt(K) stays below 512, where multiples of 1/4 are
fp16 numbers — and in the `biased` class a single lost k (1/4 ... 4) is below the output spacing once K is long: that is why there are two
classes.  The assertions below sit at the issue's figures (>= 0.98, 1.0, >= 0.9999, >= 0.2, >= 0.1), all at half the measured share or above.

The locator (`locate`) runs only on failure.  For the first wrong 64 x 64 block of C it finds the 32-wide k-slice t and the multiplicity
(0 = missing, 2 = doubled) for which truth -+ A[:, t] . B[t, :], rounded to fp16, explains the most wrong elements, and also tries "round
toward zero", "the first K range of a split held as an fp16 partial" and "never written"; its message names the kernel, layout and shape, the
C tile and block, the best hypothesis with the share of the block's wrong elements it explains, and the share of wrong elements overall."""
import functools
from typing import NamedTuple

import numpy as np
import pytest

CLASSES = ("signed", "biased")
VALUES = {"signed": (-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0), "biased": (0.5, 1.0, 1.5, 2.0)}
K_MAX = 8224
TEETH_K = (96, 352, 1056, 4192)


@functools.lru_cache(maxsize=8)
def exact_inputs(cls, M, N, K, seed=0):
    """(a [M,K], b [K,N]) fp16 numpy, read-only (shared between tests)"""
    assert 1 <= K <= K_MAX, K                                        # |C| <= 4 K < 65504
    vals = np.array(VALUES[cls], np.float16)
    rng = np.random.default_rng([seed, CLASSES.index(cls), M, N, K])
    a = vals[rng.integers(0, len(vals), (M, K))]
    b = vals[rng.integers(0, len(vals), (K, N))]
    assert 4.0 * K * float(np.abs(a).max()) * float(np.abs(b).max()) < 2.0 ** 24        # >= 4 max(|A| . |B|): every partial sum exact in fp32
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def truth64(a, b):
    return a.astype(np.float64) @ b.astype(np.float64)


def reference(a, b):
    """the exact product rounded once (to nearest even) to fp16"""
    return truth64(a, b).astype(np.float16)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16)


def rtz16(x):
    """fp64 -> fp16 with round-toward-zero (finite values inside the fp16 range)"""
    h = np.asarray(x, np.float64).astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h


# ---- the faults, applied to the reference alone --------------------------------------------------------------------------------------
def fault_slice(a, b, t, mult):
    """k-slice t (k = 32 t .. 32 t + 31) counted `mult` times instead of once"""
    s = slice(32 * t, min(32 * t + 32, a.shape[1]))
    return (truth64(a, b) + (mult - 1) * truth64(a[:, s], b[s])).astype(np.float16)


def fault_single_k(a, b, k):
    return (truth64(a, b) - np.outer(a[:, k].astype(np.float64), b[k].astype(np.float64))).astype(np.float16)


def fault_rtz(a, b):
    return rtz16(truth64(a, b))


def fault_f16_partial(a, b, k_end):
    """the sum over k < k_end stored as fp16 before the rest is added"""
    first = truth64(a[:, :k_end], b[:k_end]).astype(np.float16).astype(np.float64)
    return (first + truth64(a[:, k_end:], b[k_end:])).astype(np.float16)


# ---- the locator -----------------------------------------------------------------------------------------------------------------------
class Finding(NamedTuple):
    kind: str            # "slice", "rtz", "f16_partial", "unwritten", "none" (nothing explains half of the block), "equal"
    t: int               # slice: the 32-wide k-slice; f16_partial: the k the partial ends at; else -1
    mult: int            # slice: 0 = missing, 2 = doubled; else -1
    tile: tuple          # C tile (row, column) of the case's tile shape
    block: tuple         # the first wrong 64 x 64 block (row, column)
    share_block: float   # of the block's wrong elements, the share the hypothesis reproduces bit for bit
    share_all: float     # wrong elements / all elements of C
    message: str


def _split_ends(K):
    """where the first K range of a split-K launch may end: 1 / ks of the 64-wide K tiles, rounded either way, ks = 2 .. 8"""
    kt = -(-K // 64)
    ends = set()
    for ks in range(2, 9):
        ends |= {64 * (kt // ks), 64 * -(-kt // ks), 32 * (K // 32 // ks)}
    return sorted(e for e in ends if 0 < e < K)


def locate(got, a, b, ref=None, what="", tile=(256, 256)):
    """got: fp16 [M,N] as a kernel left it; a [M,K], b [K,N]: the operands; ref: reference(a, b) if the caller has it; what: "kernel layout
    (M,N,K)" for the message; tile: the C tile of the kernel (rows, columns).  Returns a Finding."""
    got = np.asarray(got)
    M, N = got.shape
    K = a.shape[1]
    if ref is None:
        ref = reference(a, b)
    wrong = bits(got) != bits(ref)
    share_all = float(wrong.mean())
    if not wrong.any():
        return Finding("equal", -1, -1, (), (), 0.0, 0.0, f"{what}: bit-equal to the reference")
    i0, j0 = np.argwhere(wrong)[0]
    # the first wrong block in block-row-major order (argwhere's first hit fixes the block row; take its leftmost wrong block)
    bi = int(i0) // 64
    bj = int(np.nonzero(wrong[64 * bi:64 * bi + 64].any(axis=0))[0][0]) // 64
    rs, cs = slice(64 * bi, min(64 * bi + 64, M)), slice(64 * bj, min(64 * bj + 64, N))
    ab, bb = a[rs].astype(np.float64), b[:, cs].astype(np.float64)
    g, w = bits(got[rs, cs]), wrong[rs, cs]
    nw = int(w.sum())
    T = ab @ bb
    nsl = -(-K // 32)
    pad = 32 * nsl - K
    P = np.einsum("msk,skn->smn", np.pad(ab, ((0, 0), (0, pad))).reshape(ab.shape[0], nsl, 32), np.pad(bb, ((0, pad), (0, 0))).reshape(nsl, 32, bb.shape[1]))
    hyps = []            # (explained, kind, t, mult)
    for mult in (0, 2):
        hit = ((bits((T[None] + (mult - 1) * P).astype(np.float16)) == g[None]) & w[None]).sum(axis=(1, 2))
        t = int(hit.argmax())
        hyps.append((int(hit[t]), "slice", t, mult))
    hyps.append((int(((bits(rtz16(T)) == g) & w).sum()), "rtz", -1, -1))
    for ke in _split_ends(K):
        cand = ((ab[:, :ke] @ bb[:ke]).astype(np.float16).astype(np.float64) + ab[:, ke:] @ bb[ke:]).astype(np.float16)
        hyps.append((int(((bits(cand) == g) & w).sum()), "f16_partial", ke, -1))
    hyps.append((int((np.isnan(got[rs, cs]) & w).sum()), "unwritten", -1, -1))
    hit, kind, t, mult = max(hyps, key=lambda h: h[0])          # (the first of equals: a slice before a rounding hypothesis)
    share = hit / nw
    th, tw = tile
    ct = (64 * bi // th, 64 * bj // tw)
    where = f"in C tile ({ct[0]},{ct[1]}), 64 x 64 block ({bi},{bj})"
    tail = f"explains {100 * share:.1f} % of the block; wrong: {100 * share_all:.1f} % of C"
    if share < 0.5:
        kind, t, mult = "none", -1, -1
        wr = np.nonzero(wrong)
        fg, fr = got[wr].astype(np.float64), ref[wr].astype(np.float64)
        ulp = np.maximum(np.spacing(np.abs(ref[wr])).astype(np.float64), 2.0 ** -24)
        d = np.abs(fg - fr) / ulp
        fin = np.isfinite(d)
        msg = (f"{what}: no slice, rounding mode or fp16 partial explains the first wrong block {where} (best {100 * share:.1f} %); differences of "
               f"{d[fin].min(initial=np.inf):.0f} .. {d[fin].max(initial=0):.0f} ulp at |C| {np.abs(fr).min():.6g} .. {np.abs(fr).max():.6g}, {int((~fin).sum())} non-finite; "
               f"wrong: {100 * share_all:.1f} % of C")
    elif kind == "slice":
        msg = f"{what}: k-slice {t} (k {32 * t}..{min(32 * t + 31, K - 1)}) {'missing' if mult == 0 else 'doubled'} {where}; {tail}"
    elif kind == "rtz":
        msg = f"{what}: outputs converted with round-toward-zero {where}; {tail}"
    elif kind == "f16_partial":
        msg = f"{what}: the sum over k 0..{t - 1} rounded to fp16 before the rest is added {where}; {tail}"
    else:
        msg = f"{what}: elements never written (still the NaN prefill) {where}; {tail}"
    return Finding(kind, t, mult, ct, (bi, bj), share, share_all, msg)


# ---- the builder and the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_the_inputs_are_what_the_docstring_says(cls):
    a, b = exact_inputs(cls, 256, 256, 4192)
    assert set(np.unique(a).tolist()) == set(VALUES[cls]) == set(np.unique(b).tolist())
    span = 4.0 * float((np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)).max())
    print(f"{cls}: 4 max(|A| . |B|) at K = 4192: {span:.0f}")
    assert span < 2.0 ** 24 and 20000 < span < 32000               # (measured 27 289 / 27 418)
    t = truth64(a, b)
    assert (t * 4 == np.round(t * 4)).all() and np.abs(t).max() < 65504
    # fp32 accumulation in another order and another grouping gives the same sums: slices of 32 summed backwards, K halves summed apart
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    acc = np.zeros((256, 256), np.float32)
    for s in range(4192 // 32 - 1, -1, -1):
        acc += a32[:, 32 * s:32 * s + 32] @ b32[32 * s:32 * s + 32]
    assert np.array_equal(acc.astype(np.float64), t)
    assert np.array_equal((a32[:, :2112] @ b32[:2112] + a32[:, 2112:] @ b32[2112:]).astype(np.float64), t)
    a2, _ = exact_inputs(cls, 256, 256, 4192)
    assert a2 is a and not a.flags.writeable                       # one copy, shared and left unchanged
    assert not np.array_equal(exact_inputs(cls, 256, 256, 4192, seed=1)[0], a)
    with pytest.raises(AssertionError):
        exact_inputs(cls, 8, 8, K_MAX + 32)
    if cls == "biased":                                             # what the class is for: most outputs need rounding, many sit on ties
        a, b = exact_inputs(cls, 256, 256, 352)
        t = truth64(a, b)
        assert (np.abs(t) >= 512).mean() > 0.9 and ((t * 4) % 4 == 1).mean() > 0.15 and ((t * 4) % 4 == 3).mean() > 0.15


@pytest.mark.parametrize("cls", CLASSES)
def test_the_reference_equals_the_oracle_bit_for_bit(oracle, cls):
    for (M, N, K) in ((96, 80, 352), (33, 65, 1056)):
        a, b = exact_inputs(cls, M, N, K)
        want = oracle.hgemm(a, np.ascontiguousarray(b), M, N, K, 0, "exact")
        assert np.array_equal(bits(reference(a, b)), bits(want)), (cls, M, N, K)
    assert rtz16(np.array([1.0 + 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 2049.0, 0.25])).tolist() == [1.0, -(1.0 + 2.0 ** -10), 2048.0, 0.25]


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------------
def _changed(a, b, wrong):
    return float((bits(wrong) != bits(reference(a, b))).mean())


@pytest.mark.parametrize("K", TEETH_K)
def test_a_dropped_or_doubled_slice_changes_nearly_every_element(K):
    for cls, floor in (("signed", 0.98), ("biased", 1.0)):
        a, b = exact_inputs(cls, 256, 256, K)
        for t in sorted({0, K // 64, K // 32 - 1}):
            for mult in (0, 2):
                share = _changed(a, b, fault_slice(a, b, t, mult))
                print(f"{cls} K {K} slice {t} x{mult}: {share:.4f}")
                assert share >= floor, (cls, K, t, mult, share)


@pytest.mark.parametrize("K", TEETH_K)
def test_a_single_dropped_k_changes_every_element_of_the_signed_class(K):
    a, b = exact_inputs("signed", 256, 256, K)
    for k in sorted({0, K // 2 + 1, K - 1}):
        share = _changed(a, b, fault_single_k(a, b, k))
        print(f"signed K {K} k {k}: {share:.5f}")
        assert share >= 0.9999, (K, k, share)


@pytest.mark.parametrize("K", TEETH_K)
def test_the_rounding_faults_show_in_the_biased_class_only(K):
    a, b = exact_inputs("biased", 256, 256, K)
    rtz, part = _changed(a, b, fault_rtz(a, b)), _changed(a, b, fault_f16_partial(a, b, K // 64 * 32))
    print(f"biased K {K}: round toward zero {rtz:.4f}, fp16 partial of the first half {part:.4f}")
    if K >= 352:
        assert rtz >= 0.2, (K, rtz)
    if K >= 1056:
        assert part >= 0.1, (K, part)
    a, b = exact_inputs("signed", 256, 256, K)
    rtz, part = _changed(a, b, fault_rtz(a, b)), _changed(a, b, fault_f16_partial(a, b, K // 64 * 32))
    print(f"signed K {K}: round toward zero {rtz:.5f}, fp16 partial of the first half {part:.5f}")
    assert rtz <= 1e-4 and part <= 1e-4, (K, rtz, part)            # blind: the reason for the second class


# ---- the locator names what was planted ----------------------------------------------------------------------------------------------
def _plant(ref, bad, rows, cols):
    got = ref.copy()
    got[rows, cols] = bad[rows, cols]
    return got


@pytest.mark.parametrize("cls", CLASSES)
def test_the_locator_names_the_planted_slice_and_multiplicity(cls):
    M, N, K = 384, 576, 352
    a, b = exact_inputs(cls, M, N, K)
    ref = reference(a, b)
    what = "hgemm_mid_kernel<false,2,3,2> tn (384,576,352)"
    assert locate(ref, a, b, ref, what).kind == "equal"
    for t, mult in ((5, 0), (0, 2), (10, 0), (7, 2)):
        got = _plant(ref, fault_slice(a, b, t, mult), slice(128, 256), slice(0, 192))       # C tile (1, 0) of the 128 x 192 tile
        f = locate(got, a, b, ref, what, tile=(128, 192))
        assert (f.kind, f.t, f.mult, f.tile, f.block) == ("slice", t, mult, (1, 0), (2, 0)), f.message
        assert f.share_block == 1.0 and abs(f.share_all - (bits(got) != bits(ref)).mean()) < 1e-12
        word = "missing" if mult == 0 else "doubled"
        assert f.message.startswith(f"{what}: k-slice {t} (k {32 * t}..{32 * t + 31}) {word} in C tile (1,0), 64 x 64 block (2,0); explains 100.0 % of the block; wrong: "), f.message
    # a slice lost in a later block column only: the block is the first wrong one in reading order
    got = _plant(ref, fault_slice(a, b, 3, 0), slice(0, M), slice(320, N))
    f = locate(got, a, b, None, what, tile=(128, 192))
    assert (f.kind, f.t, f.mult, f.tile, f.block) == ("slice", 3, 0, (0, 1), (0, 5)), f.message
    # a half step at the end of K (K % 64 == 32): the last slice
    f = locate(fault_slice(a, b, K // 32 - 1, 0), a, b, ref, what)
    assert (f.kind, f.t, f.mult, f.tile) == ("slice", 10, 0, (0, 0)) and "(k 320..351)" in f.message, f.message


def test_the_locator_names_the_rounding_faults_and_unwritten_elements():
    M, N, K = 256, 320, 1056
    a, b = exact_inputs("biased", M, N, K)
    ref = reference(a, b)
    what = "hgemm_mid_sk_kernel<true,1,3> x2 nn (256,320,1056)"
    f = locate(fault_rtz(a, b), a, b, ref, what)
    assert f.kind == "rtz" and f.share_block == 1.0 and "round-toward-zero" in f.message, f.message
    for ke in (512, 576, 384):                                       # KT = 17: 1 / 2 of the K tiles rounded down, up; 1 / 3 rounded up
        f = locate(fault_f16_partial(a, b, ke), a, b, ref, what)
        assert (f.kind, f.t) == ("f16_partial", ke) and f.share_block == 1.0 and f"k 0..{ke - 1} rounded to fp16" in f.message, f.message
    got = ref.copy()
    got[64:128, 128:] = np.float16("nan")
    f = locate(got, a, b, ref, what, tile=(64, 128))
    assert (f.kind, f.tile, f.block, f.share_block) == ("unwritten", (1, 1), (1, 2), 1.0) and abs(f.share_all - 64 * 192 / (M * N)) < 1e-12, f.message
    # one output ulp off at the largest |C| only: no hypothesis, and the message says where and by how much
    got = ref.copy()
    big = np.abs(ref) >= np.sort(np.abs(ref).ravel())[-200]
    got[big] = np.nextafter(ref[big], np.float16(np.inf))
    f = locate(got, a, b, ref, what)
    assert f.kind == "none" and "differences of 1 .. 1 ulp at |C| " in f.message and f.share_block < 0.5, f.message
