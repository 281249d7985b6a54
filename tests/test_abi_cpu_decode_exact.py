"""Inputs, truths, bounds, fault locator and teeth tests of tests/test_gpu_decode_exact.py: decode attention (attn_decode_kernel<D,RT>,
attn_decode_combine_kernel<D> and attn_decode_paged_kernel<D,RT>) on inputs whose answer is exact, pinned to one key or moved by a score
step.  No call here reaches a device.  Ncap = 1024, D in {64, 128}; one launch carries one batch entry per length; every (batch entry, K / V
head) pair has its own seed, so a head or batch slip cannot cancel.  Row r = g Nq + i of a K / V head is query head kvh G + g, token i.

Truths are fp64 torch straight from the definition (bottom-right aligned mask: token i of entry b sees keys 0 .. L_b - Nq + i; head map
h // G; zeros for a row without a visible key), anchored to the project's oracle (test_abi_cpu_decode.decode_truth) on a handful of rows per
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
  pinned    test_abi_cpu_decode.pinned_inputs' construction for any (H, Hkv, Nq) and any lengths: K random +-1, Q_row = (12 / sqrt(D)) K[target],
            V randn; key `target` scores 12 for its row and every other key at most 12 |cos| <= 12.  Places (pin_target, unchanged): last,
            first_invisible (its target t carries the V row 8 K[t]: +-8 with the key's own signs — with one fixed +-8 pattern, as in
            test_abi_cpu_decode.py, token i + 1 sees the target of token i under the causal mask, at Nq = 64 nearly every visible V row is
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
import functools
import math

import numpy as np
import pytest
import torch

from tests import tol
from tests.test_abi_cpu_decode import SCORE, TEETH, decode_truth, pin_target, rt_of, visible
from tests.test_abi_cpu_decode_paged import gather, paginate
from tests.test_gpu_attn_exact import STEP_C, V8, V16, _draw, _pm1, round_once, ulp

NCAP = 1024
DS = (64, 128)
LENS = (1024, 1000, 577, 130, 65, 64, 33, 32, 31, 16, 1, 0)
GRID = ((2, 2, 1), (8, 1, 1), (6, 2, 5), (2, 2, 17), (8, 2, 8), (6, 2, 11), (8, 2, 9), (6, 1, 8), (7, 1, 9), (2, 2, 64))      # (H, Hkv, Nq)
ROW_SHAPES = ((8, 1, 1), (2, 2, 17), (8, 2, 9), (7, 1, 9), (2, 2, 64))                # R, RT = (8, 1), (17, 2), (36, 4), (63, 4), (64, 4)
PIN_LENS = (1000, 577, 130, 65, 33)
STEP_LENS = (1024, 1000, 577, 130)
PLACES = ("last", "first_invisible", "key0", "tile_seam", "step_seam", "range_seam")
UNIFORM_SPLITS = (1, 2, 3, 8, 16, 64)
PINNED_SPLITS = (1, 3, 8)
STEP_SPLITS = (1, 2, 4, 8)
BLOCK_LENS = (1024, 1000, 577, 130)
PAGED_SHAPES = ((8, 1, 1), (8, 2, 9))                                                 # RT = 1 and RT = 4
PAGE_SIZES = (16, 64)
FLOOR = 2.0 ** -6


def ulp16(x):
    return ulp(x, False)


def step_of(D, H, Hkv, Nq):
    """keys per pipeline step of attn_decode_kernel<D, RT>"""
    return 32 if (D == 128 and rt_of(H, Hkv, Nq) == 4) else 64


def nk_table(lens, Nq, causal):
    """int64 [B, Nq]: visible keys of token i of batch entry b"""
    return np.array([[visible(L, Nq, NCAP, causal, i) for i in range(Nq)] for L in lens], np.int64)


def _seed(cls, D, H, Hkv, Nq, b, kvh, extra=0):
    return ((((("uniform", "pinned", "step").index(cls) * 7 + D // 64) * 131 + H) * 17 + Hkv) * 67 + Nq) * 4099 + 61 * b + kvh + 1000003 * extra


# ------------------------------------------------------------------------------------------------------------------------------------
# the truth of any input: fp64 torch from the definition

def weights64(q, k, lens, causal):
    """(p [B,H,Nq,Ncap] fp64: exp(score - row max) on the visible keys, 0 elsewhere; nks [B,Nq])"""
    B, H, Nq, D = q.shape
    G = H // k.shape[1]
    nks = nk_table(lens, Nq, causal)
    heads = torch.arange(H) // G
    s = q.double() @ k.double()[:, heads].transpose(-2, -1) / D ** 0.5                       # [B, H, Nq, Ncap]
    vis = torch.arange(NCAP).view(1, 1, 1, NCAP) < torch.from_numpy(nks).view(B, 1, Nq, 1)
    s = s.masked_fill(~vis, -float("inf"))
    mx = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
    return p, nks


def attend64(p, v, H):
    """[B,H,Nq,D] fp64 numpy: rows of p normalised against V; a row whose weights are all 0 is zeros"""
    G = H // v.shape[1]
    l = p.sum(-1, keepdim=True)
    w = torch.where(l > 0, p / l.clamp(min=1e-300), torch.zeros_like(p))
    return (w @ v.double()[:, torch.arange(H) // G]).numpy()


def truth64(q, k, v, lens, causal):
    p, nks = weights64(q, k, lens, causal)
    return attend64(p, v, q.shape[1]), nks


# ------------------------------------------------------------------------------------------------------------------------------------
# uniform

@functools.lru_cache(maxsize=4)
def uniform_inputs(D, H, Hkv, Nq):
    """(q [B,H,Nq,D], k, v [B,Hkv,Ncap,D]) fp16 on the CPU, B = len(LENS); the same tensors serve causal and non-causal launches"""
    B, G = len(LENS), H // Hkv
    q = torch.zeros(B, H, Nq, D)
    k = torch.zeros(B, Hkv, NCAP, D)
    v = torch.zeros(B, Hkv, NCAP, D)
    for b in range(B):
        for kvh in range(Hkv):
            g = torch.Generator().manual_seed(_seed("uniform", D, H, Hkv, Nq, b, kvh))
            v[b, kvh] = _draw(g, V16, (NCAP, D))
            if kvh % 2 == 0:
                k[b, kvh] = _pm1(g, (NCAP, D))
            else:
                q[b, kvh * G:(kvh + 1) * G] = _pm1(g, (G, Nq, D))
    return q.half(), k.half(), v.half()


def prefix_sums(v):
    """fp64 numpy [B,Hkv,Ncap+1,D]: P[n] = the sum of V[0 : n] (exact)"""
    c = v.double().cumsum(dim=2)
    return torch.cat([torch.zeros_like(c[:, :, :1]), c], dim=2).numpy()


def uniform_means(P, nks, H):
    """E [B,H,Nq,D]: the mean of V[0 : nk] of the row's K / V head, zeros where nk = 0"""
    B, Hkv = P.shape[:2]
    G = H // Hkv
    n = np.clip(nks, 0, NCAP)
    sums = P[np.arange(B)[:, None, None], (np.arange(H) // G)[None, :, None], n[:, None, :]]       # [B, H, Nq, D]
    return sums / np.maximum(n, 1)[:, None, :, None]


@functools.lru_cache(maxsize=4)
def uniform_truth(D, H, Hkv, Nq, causal):
    """(E [B,H,Nq,D], nks [B,Nq], prefix sums) of a launch over LENS; shared, never written to"""
    P = prefix_sums(uniform_inputs(D, H, Hkv, Nq)[2])
    nks = nk_table(LENS, Nq, causal)
    return uniform_means(P, nks, H), nks, P


def uniform_bound(E, split):
    return ulp16(E) if split == 1 else ulp16(np.maximum(np.abs(E), FLOOR))


# ------------------------------------------------------------------------------------------------------------------------------------
# pinned

def target_of(place, L, Nq, causal, r, split):
    if place != "step_seam":
        return pin_target(place, L, Nq, NCAP, causal, r, split)
    lim = visible(L, Nq, NCAP, causal, r % Nq)
    if lim < 33:
        return None                                     # no tile holds keys 31 and 32 of it below the limit
    t = (lim - 33) // 64
    return 64 * t + (31 if r % 2 == 0 else 32)


@functools.lru_cache(maxsize=4)
def pinned_inputs(D, place, causal, H, Hkv, Nq, split=3, lens=PIN_LENS):
    """(q, k, v, targets): fp16 CPU tensors and targets[b][h][i] (None: the row keeps its random query)"""
    B, G = len(lens), H // Hkv
    q = torch.empty(B, H, Nq, D)
    k = torch.empty(B, Hkv, NCAP, D)
    v = torch.empty(B, Hkv, NCAP, D)
    targets = [[[None] * Nq for _ in range(H)] for _ in range(B)]
    for b in range(B):
        for kvh in range(Hkv):
            g = torch.Generator().manual_seed(_seed("pinned", D, H, Hkv, Nq, b, kvh, 1 + 2 * PLACES.index(place) + int(causal)))
            k[b, kvh] = _pm1(g, (NCAP, D))
            v[b, kvh] = torch.randn(NCAP, D, generator=g)
            q[b, kvh * G:(kvh + 1) * G] = torch.randn(G, Nq, D, generator=g)
            for r in range(G * Nq):
                t = target_of(place, lens[b], Nq, causal, r, split)
                if t is None:
                    continue
                h, i = kvh * G + r // Nq, r % Nq
                targets[b][h][i] = t
                q[b, h, i] = (SCORE / D ** 0.5) * k[b, kvh, t]
                if place == "first_invisible":
                    v[b, kvh, t] = 8.0 * k[b, kvh, t]
    return q.half(), k.half(), v.half(), targets


def pinned_split_key(place, split):
    """the inputs depend on S only where the targets do"""
    return split if (place == "range_seam" and split > 1) else 3


@functools.lru_cache(maxsize=2)
def pinned_truth(D, place, causal, H, Hkv, Nq, split=3):
    q, k, v, _ = pinned_inputs(D, place, causal, H, Hkv, Nq, split)
    return truth64(q, k, v, PIN_LENS, causal)


def decode_bound(truth, nks):
    """check_decode's bound as an array [B,H,Nq,D]"""
    atol = np.array([[tol.attn_max_abs(int(n)) for n in row] for row in nks])[:, None, :, None]
    return atol + tol.ATTN_RTOL_F16 * np.abs(truth)


# ------------------------------------------------------------------------------------------------------------------------------------
# step

def step_tile(D, H, Hkv, Nq, b, kvh, L):
    T = -(-L // 64)
    hi = max((L - Nq + 1) // 64, 1)                    # the whole window below the smallest causal limit of the entry
    lo = min(-(-T // 4), hi - 1)
    g = torch.Generator().manual_seed(_seed("step", D, H, Hkv, Nq, b, kvh, 7))
    return lo + int(torch.randint(0, hi - lo, (1,), generator=g))


@functools.lru_cache(maxsize=4)
def step_inputs(D, H, Hkv, Nq):
    """(q, k, v, tiles [B][Hkv]) fp16 on the CPU, B = len(STEP_LENS)"""
    B, G = len(STEP_LENS), H // Hkv
    q = torch.empty(B, H, Nq, D)
    k = torch.zeros(B, Hkv, NCAP, D)
    v = torch.empty(B, Hkv, NCAP, D)
    c = torch.tensor(STEP_C)[torch.arange(G * Nq) % 3].view(G, Nq, 1)
    tiles = []
    for b, L in enumerate(STEP_LENS):
        tiles.append([])
        for kvh in range(Hkv):
            g = torch.Generator().manual_seed(_seed("step", D, H, Hkv, Nq, b, kvh))
            v[b, kvh] = _draw(g, V8, (NCAP, D))
            u, w = _pm1(g, (D,)), _draw(g, V8, (D,))
            t = step_tile(D, H, Hkv, Nq, b, kvh, L)
            tiles[-1].append(t)
            k[b, kvh, 64 * t + 24:64 * t + 64] = u
            v[b, kvh, 64 * t + 24:64 * t + 64] = w
            q[b, kvh * G:(kvh + 1) * G] = (c / D ** 0.5) * u
    return q.half(), k.half(), v.half(), tiles


@functools.lru_cache(maxsize=2)
def step_truth(D, H, Hkv, Nq, causal):
    q, k, v, _ = step_inputs(D, H, Hkv, Nq)
    return truth64(q, k, v, STEP_LENS, causal)


def step_bound(truth, nks):
    """tol.attn_close(N = nk, rtol = tol.ATTN_RTOL_SPIKE) as an array"""
    atol = np.array([[tol.attn_max_abs(int(n)) for n in row] for row in nks])[:, None, :, None]
    return atol + tol.ATTN_RTOL_SPIKE * np.abs(truth)


def emulate_kernel(s, v, lims, L, S, STEP, fault=None):
    """One (batch entry, K / V head) the way the kernel walks it, in fp64 and natural units: s [R,Ncap] scores, v [Ncap,D], lims [R].
    fault: None, "alpha_l", "alpha_o", ("mine", w), "combine".  Returns (out [R,D], applies [R]: the dropped factor differed from 1 on
    something non-zero)."""
    R, D = s.shape[0], v.shape[1]
    ninf = -float("inf")
    s = s.masked_fill(torch.arange(NCAP).view(1, -1) >= lims.view(-1, 1), ninf)
    T = -(-L // 64)
    applies = torch.zeros(R, dtype=torch.bool)
    parts, lses = [], []
    for si in range(S):
        t0, t1 = si * T // S, (si + 1) * T // S
        M = torch.full((4, R), ninf, dtype=torch.float64)
        Lw = torch.zeros(4, R, dtype=torch.float64)
        Ow = torch.zeros(4, R, D, dtype=torch.float64)
        for w in range(4):
            m, l, o = M[w].clone(), Lw[w].clone(), Ow[w].clone()
            for t in range(t0 + w, t1, 4):
                for a in range(64 * t, 64 * t + 64, STEP):
                    blk = s[:, a:a + STEP]
                    mn = torch.maximum(m, blk.max(dim=1).values)
                    mu = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
                    alpha, p = torch.exp(m - mu), torch.exp(blk - mu.view(-1, 1))
                    if fault in ("alpha_l", "alpha_o"):
                        applies |= (alpha != 1) & (l > 0)
                    l = (l if fault == "alpha_l" else l * alpha) + p.sum(dim=1)
                    o = (o if fault == "alpha_o" else o * alpha.view(-1, 1)) + p @ v[a:a + STEP]
                    m = mn
            M[w], Lw[w], Ow[w] = m, l, o
        mm = M.max(dim=0).values
        mu = torch.where(torch.isinf(mm), torch.zeros_like(mm), mm)
        f = torch.exp(M - mu)
        ls = (Lw * f).sum(dim=0)
        mine = f.clone()
        if isinstance(fault, tuple):
            w = fault[1]
            whole = torch.zeros(R, dtype=torch.bool)    # `mine` of wave w is judged on the rows that see the wave's first tile of the range whole
            if t0 + w < t1:
                whole = (s[:, 64 * (t0 + w):64 * (t0 + w) + 64] > ninf).all(dim=1)
            hit = whole & (f[w] != 1) & (Lw[w] > 0)
            mine[w] = torch.where(hit, torch.ones_like(f[w]), f[w])
            applies |= hit
        o = (Ow * mine.unsqueeze(-1)).sum(dim=0)
        inv = torch.where(ls > 0, 1 / ls.clamp(min=1e-300), torch.zeros_like(ls))
        parts.append(o * inv.view(-1, 1))
        lses.append(torch.where(ls > 0, mm + torch.log(ls.clamp(min=1e-300)), torch.full_like(ls, ninf)))
    if S == 1:
        return parts[0].numpy(), applies.numpy()
    part, lse = torch.stack(parts), torch.stack(lses)                                   # [S, R, D], [S, R]
    mx = lse.max(dim=0).values
    wgt = torch.exp(lse - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
    wgt = torch.where(torch.isinf(lse), torch.zeros_like(wgt), wgt)
    if fault == "combine":
        live = ~torch.isinf(lse)
        n = live.sum(dim=0)
        off = ((wgt / wgt.sum(dim=0).clamp(min=1e-300) - 1 / n.clamp(min=1)).abs() * live).max(dim=0).values
        applies |= (n >= 2) & (off >= COMBINE_OFF) & (s.max(dim=1).values > 0)      # (a row that sees no step key is `uniform`'s business)
        wgt = live.double()
    ws = wgt.sum(dim=0)
    out = (part * wgt.unsqueeze(-1)).sum(dim=0) * torch.where(ws > 0, 1 / ws.clamp(min=1e-300), torch.zeros_like(ws)).view(-1, 1)
    return out.numpy(), applies.numpy()


COMBINE_OFF = 1.0 / 16      # "all combine weights equal" is judged on rows where some range's true share of the weight is this far from 1 / ranges
STEP_FAULTS = ("alpha_l", "alpha_o", ("mine", 0), ("mine", 1), ("mine", 2), ("mine", 3), "combine")


# ------------------------------------------------------------------------------------------------------------------------------------
# the judge and the fault locator

def uniform_hypotheses(P, lens, H, Hkv, Nq, causal, S, b, h, i):
    """(name, the mean [D] a kernel with that ONE fault would give row (b, h, i)) for every candidate fault"""
    G = H // Hkv
    kvh, L = h // G, min(max(int(lens[b]), 0), NCAP)
    nk = visible(L, Nq, NCAP, causal, i)
    tot = P[b, kvh, nk]

    def mean(x, n):
        return x / n if n > 0 else np.zeros_like(x)

    if nk >= 1:
        yield "limit one key short", mean(P[b, kvh, nk - 1], nk - 1)
    if nk < NCAP:
        yield "limit one key long", mean(P[b, kvh, nk + 1], nk + 1)
    for d in (-1, 1):
        n2 = min(visible(L, Nq, NCAP, causal, i + d), NCAP)
        if n2 != nk:
            yield f"the limit of token {i + d} (wrong r % Nq)", mean(P[b, kvh, n2], n2)
    for size in (16, 32, 64):
        for t in range(-(-nk // size)):
            a, e = size * t, min(size * t + size, nk)
            seg = P[b, kvh, e] - P[b, kvh, a]
            yield f"{size}-key block {t} dropped", mean(tot - seg, nk - (e - a))
            yield f"{size}-key block {t} doubled", mean(tot + seg, nk + (e - a))
    T = -(-L // 64)
    for s in range(S):
        t0, t1 = s * T // S, (s + 1) * T // S
        a, e = min(64 * t0, nk), min(64 * t1, nk)
        if S > 1 and e > a:
            seg = P[b, kvh, e] - P[b, kvh, a]
            yield f"range {s} of {S} dropped", mean(tot - seg, nk - (e - a))
            yield f"range {s} of {S} doubled", mean(tot + seg, nk + (e - a))
        for w in range(4):
            seg, cnt = np.zeros_like(tot), 0
            for t in range(t0 + w, t1, 4):
                a, e = min(64 * t, nk), min(64 * t + 64, nk)
                seg, cnt = seg + P[b, kvh, e] - P[b, kvh, a], cnt + e - a
            if cnt:
                yield f"wave {w}'s tiles dropped" + (f" in range {s} of {S}" if S > 1 else ""), mean(tot - seg, nk - cnt)
    if h % Hkv != kvh:
        yield f"K / V head h % Hkv = {h % Hkv}", mean(P[b, h % Hkv, nk], nk)
    if b != 0:
        yield "batch entry 0's cache", mean(P[0, kvh, nk], nk)


def locate_uniform(row, P, lens, H, Hkv, Nq, causal, S, b, h, i):
    """(name, residual): the one-fault hypothesis closest to an output row (largest |difference| over its columns)"""
    best = ("none of the one-fault hypotheses", float("inf"))
    for name, hyp in uniform_hypotheses(P, lens, H, Hkv, Nq, causal, S, b, h, i):
        res = float(np.nan_to_num(np.abs(hyp - row), nan=np.inf).max())
        if res < best[1]:
            best = (name, res)
    return best


def judge(kernel, cls, out, truth, bound, nks, Hkv, strict=False, hint=None):
    """out, truth [B,H,Nq,D] fp64 numpy: rows without a visible key exactly 0, every other element finite and inside `bound` (strict: |err|
    < bound).  Returns the worst |err| / bound; a failure names kernel, batch entry, K / V head, g, token, nk, the share of wrong elements
    and hint(b, h, i)."""
    B, H, Nq, D = truth.shape
    G = H // Hkv
    zero = np.broadcast_to((nks == 0)[:, None, :, None], truth.shape)
    finite = np.isfinite(out)
    err = np.abs(out - truth)
    with np.errstate(invalid="ignore"):
        bad = ~finite | ((err >= bound) if strict else (err > bound))
        ratio = np.where(zero | ~finite, 0.0, err / bound)
    wrong = np.where(zero, out != 0, bad)
    if wrong.any():
        score = np.where(wrong, np.where(zero | ~finite, np.inf, err / bound), -1.0)
        b, h, i, d = (int(x) for x in np.unravel_index(np.argmax(score), score.shape))
        msg = (f"{kernel} [{cls}]: batch entry {b}, K / V head {h // G}, g {h % G} (query head {h}), token {i}, nk {int(nks[b, i])}, column {d}: "
               f"got {out[b, h, i, d]!r}, want {truth[b, h, i, d]!r} (bound {float(np.broadcast_to(bound, truth.shape)[b, h, i, d]):.3e}); wrong: "
               f"{wrong.mean():.2%} of all elements, {int(wrong.any(axis=-1).sum())} of {B * H * Nq} rows, {wrong[b, h, i].mean():.0%} of this row"
               + ("; " + hint(b, h, i) if hint else ""))
        raise AssertionError(msg)
    return float(ratio.max())


def uniform_hint(out, P, lens, H, Hkv, Nq, causal, S):
    def hint(b, h, i):
        name, res = locate_uniform(out[b, h, i], P, lens, H, Hkv, Nq, causal, S, b, h, i)
        return f"closest one-fault hypothesis: {name} (residual {res:.2e})"
    return hint


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
