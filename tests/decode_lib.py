"""What the decode-attention test modules share (tests/test_abi_cpu_decode*.py, tests/test_gpu_decode*.py); not a test module and not a conftest:
nothing here is collected.  Four parts: the inputs, truth and row check of the contiguous call with the pinned construction; the paged cache
(`paginate`, `gather`, the page-seam inputs); the fp8 cache (e4m3 tables, `quantize`, `dequant`, the float64 reference); the exact-input classes
of tests/test_*_decode_exact.py — and one copy of what the modules repeat around a call: the library handle, the oracle, kv_len on the device, a
call under a forced split, the knob reset, the name calls.  The test functions, and the proofs that these inputs have teeth, stay in their modules.

The modules use two cache capacities, on purpose: NCAP_RAGGED = 1000 (tests/test_gpu_decode.py) and NCAP_POW2 = 1024 (paged, fp8, exact)."""
import ctypes as C
import functools

import numpy as np
import torch

from leetcuda_amd import capi
from tests import tol
from tests.test_gpu_attn_exact import STEP_C, V8, V16, _draw, _pm1, ulp

NCAP_RAGGED = 1000   # tests/test_gpu_decode.py: the last tile is ragged
NCAP_POW2 = 1024     # the paged, fp8 and exact-input modules: whole pages of every size
GRID_SHAPES = [(3, 8, 2), (2, 4, 1), (2, 4, 4)]                     # (B, H, Hkv)
GRID_LENS = {3: (NCAP_RAGGED, 129, 65), 2: (65, NCAP_RAGGED)}                      # per-batch kv_len of the grid test, by B (B = 2 with Hkv = 4: reversed)
GRID_NQ = (1, 4, 5, 16)
SCORE = 12.0      # natural units: the dominant key of a pinned row (the construction of tests/test_gpu_causal_mask.py)
TEETH = 20.0
PIN_SHAPE = (3, 8, 2)
PIN_NQ = 5
PIN_LENS = (777, 129, 65)       # all < NCAP_RAGGED: position L_b exists, so "the first invisible key" does for every row
PLACES = ("last", "first_invisible", "key0", "tile_seam", "range_seam")


def decode_inputs(B, H, Hkv, Nq, Ncap, D, seed):
    """fp16 randn q [B,H,Nq,D], k, v [B,Hkv,Ncap,D] on the CPU (the GPU tests move them over: CPU and GPU modules test the same inputs)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, Nq, D, generator=g).half(), torch.randn(B, Hkv, Ncap, D, generator=g).half(),
            torch.randn(B, Hkv, Ncap, D, generator=g).half())


def visible(L, Nq, Ncap, causal, i):
    """number of keys query i of a batch entry with kv_len L sees: keys 0 .. visible - 1 (lc_abi.h: bottom-right aligned)"""
    L = min(max(int(L), 0), Ncap)
    return max(0, L - Nq + i + 1) if causal else L


def rt_of(H, Hkv, Nq):
    R = (H // Hkv) * Nq
    return 1 if R <= 16 else 2 if R <= 32 else 4


def decode_truth(oracle, q, k, v, lens, causal, nk_of=None, kv_head=None, kv_batch=None):
    """(truth fp32 [B,H,Nq,D], nk int [B,Nq]): the oracle on every row.  lens: per-batch kv_len (None: Ncap).  The keyword arguments restate a
    WRONG kernel for the tests of the inputs: nk_of(b, i) -> visible keys, kv_head(h) -> K / V head, kv_batch(b) -> batch entry read."""
    B, H, Nq, D = q.shape
    Hkv, Ncap = k.shape[1], k.shape[2]
    G = H // Hkv
    heads = [kv_head(h) if kv_head else h // G for h in range(H)]
    truth = np.zeros((B, H, Nq, D), np.float32)
    nks = np.zeros((B, Nq), np.int64)
    for b in range(B):
        L = Ncap if lens is None else lens[b]
        for i in range(Nq):
            nks[b, i] = nk_of(b, i) if nk_of else visible(L, Nq, Ncap, causal, i)
        bb = kv_batch(b) if kv_batch else b
        kb, vb = k[bb][heads], v[bb][heads]                     # [H, Ncap, D]: expanded to the query heads
        for nk in sorted(set(int(x) for x in nks[b])):
            rows = [i for i in range(Nq) if nks[b, i] == nk]
            if nk == 0:
                continue                                        # no visible key: exactly 0
            o = oracle.attn_rows(q[b][:, rows].contiguous(), kb[:, :nk].contiguous(), vb[:, :nk].contiguous(), H, len(rows), nk, D)
            truth[b][:, rows] = o
    return truth, nks


def check_decode(out, truth, nks, what=""):
    """every row under tol.attn_close with N = the row's visible keys; rows without a visible key are exactly 0.  Returns the worst
    |err| / bound (for the docstrings)."""
    out = np.asarray(out, np.float32)
    worst = 0.0
    B, H, Nq, D = truth.shape
    for b in range(B):
        for i in range(Nq):
            nk = int(nks[b, i])
            o, t = out[b, :, i], truth[b, :, i]
            if nk == 0:
                assert (o == 0).all(), (what, "row without a visible key is not 0", b, i, float(np.abs(o).max()))
                continue
            assert np.isfinite(o).all(), (what, "non-finite", b, i)
            ok, err, excess = tol.attn_close(o, t, N=nk)
            bound = tol.attn_max_abs(nk) + tol.ATTN_RTOL_F16 * np.abs(t.astype(np.float64))
            worst = max(worst, float((np.abs(o.astype(np.float64) - t) / bound).max()))
            assert ok, (what, f"batch {b} query {i} nk {nk}: max |err| {err:.3e}, excess over the bound {excess:.3e}")
    return worst


def pin_target(place, L, Nq, Ncap, causal, r, split):
    """the key that scores SCORE for row r = g Nq + i of a K / V head (None: the row keeps a random query)"""
    i = r % Nq
    lim = visible(L, Nq, Ncap, causal, i)
    if place == "last":
        return lim - 1 if lim >= 1 else None
    if place == "first_invisible":
        return lim if lim < Ncap else None
    if place == "key0":
        return 0 if lim >= 1 else None
    if place == "tile_seam":                        # either side of the last tile seam below the row's limit
        p = 64 * ((lim - 1) // 64) if lim >= 1 else 0
        if p == 0:
            return None
        return p - 1 if r % 2 == 0 else p
    if place == "range_seam":                       # either side of a seam between two KV ranges of the kernel's partition (split ranges)
        T = (L + 63) // 64
        seams = sorted({64 * (s * T // split) for s in range(1, split)} - {0})
        seams = [p for p in seams if p < lim]
        if not seams:
            return None
        p = seams[(r // 2) % len(seams)]
        return p - 1 if r % 2 == 0 else p
    raise KeyError(place)


@functools.lru_cache(maxsize=16)
def pinned_inputs(D, place, causal, split=3):
    """(q, k, v, lens): per row ONE key outweighs the rest — K random +-1, Q_row = (SCORE / sqrt(D)) K[target], V randn; the target of
    `first_invisible` carries a large distinctive V row (+-8).  Rows without a target (no visible key, no seam below the limit) keep randn."""
    B, H, Hkv = PIN_SHAPE
    Nq, G = PIN_NQ, PIN_SHAPE[1] // PIN_SHAPE[2]
    g = torch.Generator().manual_seed(7919 * D + 31 * PLACES.index(place) + int(causal))
    k = (torch.randint(0, 2, (B, Hkv, NCAP_RAGGED, D), generator=g) * 2 - 1).float()
    v = torch.randn(B, Hkv, NCAP_RAGGED, D, generator=g)
    q = torch.randn(B, H, Nq, D, generator=g)
    big = torch.tensor([8.0, -8.0]).repeat(D // 2)
    for b in range(B):
        for h in range(H):
            kvh, gq = h // G, h % G
            for i in range(Nq):
                t = pin_target(place, PIN_LENS[b], Nq, NCAP_RAGGED, causal, gq * Nq + i, split)
                if t is None:
                    continue
                q[b, h, i] = (SCORE / D ** 0.5) * k[b, kvh, t]
                if place == "first_invisible":
                    v[b, kvh, t] = big
    return q.half(), k.half(), v.half(), PIN_LENS


def auto_split(groups, ncap, cus):
    """the documented rule, restated: the smallest S that gives every CU a workgroup, >= 4 tiles of Ncap per range, <= 64"""
    tiles = (ncap + 63) // 64
    return max(1, min(-(-cus // groups), tiles // 4, 64))


def _moved(truth, nks, wrong):
    """[B, H, Nq]: largest |wrong - truth| / bound over a row's columns, the bound being that of the row's visible keys"""
    atol = np.array([[tol.attn_max_abs(int(n)) for n in row] for row in nks]).reshape(nks.shape[0], 1, nks.shape[1], 1)
    bound = atol + tol.ATTN_RTOL_F16 * np.abs(truth.astype(np.float64))
    return (np.abs(wrong.astype(np.float64) - truth) / bound).max(axis=-1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the paged cache

def paginate(k, v, lens, page_size, seed, spare=3, fill=float("nan")):
    """(k_pool, v_pool [P,Hkv,page_size,D], table int32 [B,max_pages]) of a contiguous [B,Hkv,Ncap,D] cache, P = B max_pages + spare.
    Pages are placed by a seeded random permutation of the pool: a sequence's pages are scattered, non-monotone and interleaved with the other
    batch entries'.  Every pool row of a logical position >= L_b is `fill` (NaN), every table entry at a position >= ceil(L_b / page_size) names
    a spare page that is `fill` throughout — a valid id: nothing here feeds an out-of-range page."""
    B, Hkv, Ncap, D = k.shape
    assert Ncap % page_size == 0 and spare >= 1
    mp = Ncap // page_size
    P = B * mp + spare
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    pools = [torch.full((P, Hkv, page_size, D), fill, dtype=k.dtype) for _ in range(2)]
    table = torch.empty(B, mp, dtype=torch.int32)
    tail = torch.arange(Ncap).view(1, 1, Ncap, 1) >= torch.tensor([min(max(int(x), 0), Ncap) for x in lens]).view(B, 1, 1, 1)
    for pool, x in zip(pools, (k, v)):
        x = x.masked_fill(tail, fill)
        for b in range(B):
            for p in range(mp):
                pool[perm[b * mp + p]] = x[b, :, p * page_size:(p + 1) * page_size]
    for b in range(B):
        used = -(-min(max(int(lens[b]), 0), Ncap) // page_size)
        for p in range(mp):
            table[b, p] = perm[b * mp + p] if p < used else perm[B * mp + (b + p) % spare]
    return pools[0], pools[1], table


def gather(pool, table, batch_of=None, page_of=None, head_of=None, row_of=None):
    """the contiguous [B,Hkv,Ncap,D] view a kernel sees through `table`.  The keyword arguments restate a WRONG kernel: batch_of(b) -> table row,
    page_of(b, p) -> pool page of logical page p (instead of table[b][p]), head_of(h) -> K / V head slab, row_of(j) -> row inside the page"""
    B, mp = table.shape
    P, Hkv, ps, D = pool.shape
    rows = torch.tensor([row_of(j) if row_of else j for j in range(ps)])
    heads = torch.tensor([head_of(h) if head_of else h for h in range(Hkv)])
    out = torch.empty(B, Hkv, mp * ps, D, dtype=pool.dtype)
    for b in range(B):
        tb = batch_of(b) if batch_of else b
        for p in range(mp):
            pid = page_of(b, p) if page_of else int(table[tb, p])
            out[b, :, p * ps:(p + 1) * ps] = pool[pid][heads][:, rows]
    return out


def seam_target(L, Nq, Ncap, causal, r):
    """the key that scores SCORE for row r = g Nq + i of a K / V head: one key before (r even) or at (r odd) a 16-key page boundary below the
    row's limit, the boundary varying with r.  Boundaries are 16 j with j % 4 in {2, 3}: both sides of each have an offset >= 16 inside a
    64-key page, where "offset modulo 16" loses them.  None: no such boundary below the limit."""
    lim = visible(L, Nq, Ncap, causal, r % Nq)
    seams = [16 * j for j in range(1, (lim + 15) // 16) if j % 4 in (2, 3) and 16 * j < lim]
    if not seams:
        return None
    p = seams[(7 * (r // 2) + 3) % len(seams)]
    return p - 1 if r % 2 == 0 else p


@functools.lru_cache(maxsize=8)
def seam_inputs(D, causal):
    """(q, k, v, lens) at Ncap = 1024: K random +-1, Q_row = (SCORE / sqrt(D)) K[target], V randn — the construction of pinned_inputs"""
    B, H, Hkv = PIN_SHAPE
    Nq, G = PIN_NQ, H // Hkv
    g = torch.Generator().manual_seed(104729 * D + int(causal))
    k = (torch.randint(0, 2, (B, Hkv, NCAP_POW2, D), generator=g) * 2 - 1).float()
    v = torch.randn(B, Hkv, NCAP_POW2, D, generator=g)
    q = torch.randn(B, H, Nq, D, generator=g)
    for b in range(B):
        for h in range(H):
            for i in range(Nq):
                t = seam_target(PIN_LENS[b], Nq, NCAP_POW2, causal, (h % G) * Nq + i)
                if t is not None:
                    q[b, h, i] = (SCORE / D ** 0.5) * k[b, h // G, t]
    return q.half(), k.half(), v.half(), PIN_LENS


def _wrong_kernel(oracle, q, kw, vw, lens, causal, truth, nks):
    """[B, H, Nq] ratio of a kernel that sees the cache (kw, vw).  A row whose visible keys hold a non-finite K or V row gets inf: the kernel's
    score or P V product is NaN there, which check_decode refuses outright (the oracle is only asked about finite inputs)."""
    B, H, Nq, _ = q.shape
    G = H // kw.shape[1]
    poisoned = np.zeros((B, H, Nq), bool)
    for b in range(B):
        bad = ~(torch.isfinite(kw[b]).all(dim=-1) & torch.isfinite(vw[b]).all(dim=-1))       # [Hkv, Ncap]
        first_bad = [int(torch.nonzero(bad[kh])[0]) if bad[kh].any() else NCAP_POW2 for kh in range(kw.shape[1])]
        for h in range(H):
            for i in range(Nq):
                poisoned[b, h, i] = first_bad[h // G] < nks[b, i]
    clean = lambda x: torch.where(torch.isfinite(x), x, torch.zeros_like(x))      # noqa: E731
    wrong, _ = decode_truth(oracle, q, clean(kw), clean(vw), lens, causal)
    ratio = _moved(truth, nks, wrong)
    ratio[poisoned] = np.inf
    return ratio


# ------------------------------------------------------------------------------------------------------------------------------------
# the fp8 (e4m3) cache

NAN_BYTE = 0x7F


def _e4m3_table(bias, nan_codes):
    """float32 [256]: the value of every code of a 1-4-3 format with this exponent bias"""
    out = np.zeros(256, np.float32)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        mag = m * 2.0 ** (1 - bias - 3) if e == 0 else (1 + m / 8) * 2.0 ** (e - bias)
        out[c] = -mag if c & 0x80 else mag
    for c in nan_codes:
        out[c] = np.nan
    return torch.from_numpy(out)


OCP = _e4m3_table(7, (0x7F, 0xFF))        # OCP e4m3fn: what the kernel decodes (torch.float8_e4m3fn)
FNUZ = _e4m3_table(8, (0x80,))            # e4m3fnuz: what gfx942-era code decodes; half the value of every normal code, 0x80 = NaN
FINITE_CODES = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)

# power-of-two scales, 2^-5 .. 2^2, different between K / V heads and between K and V (the first Hkv of each are used)
K_SCALES = (2.0 ** -3, 2.0 ** -1, 2.0 ** -4, 2.0 ** -2)
V_SCALES = (2.0 ** -2, 2.0 ** -4, 2.0 ** 0, 2.0 ** -3)


def scales(values, Hkv):
    return torch.tensor(values[:Hkv], dtype=torch.float32)


def _per_head(scale, x):
    """a float or a float32 [Hkv] tensor, broadcast over [*, Hkv, rows, D]"""
    return scale.view(1, -1, 1, 1) if torch.is_tensor(scale) else scale


def quantize(x_fp16, scale):
    """uint8, the shape of x: the e4m3fn bytes of x / scale (round to nearest even, saturating at +-448)"""
    y = (x_fp16.float() / _per_head(scale, x_fp16)).clamp(-448.0, 448.0)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def dequant(codes, scale, table=OCP):
    """fp16: value(code) x scale.  Exact for a power-of-two scale in 2^-5 .. 2^2 (test_dequant_is_exact_...)"""
    return (table[codes.long()] * _per_head(scale, codes)).half()


def dequant64(codes, scale):
    """float64: value(code) x scale with the scale as the kernel holds it (float32), the product exact"""
    s = scale.view(1, -1, 1, 1).double() if torch.is_tensor(scale) else float(np.float32(scale))
    return OCP[codes.long()].double() * s


def softmax64(q, k64, v64, lens, causal):
    """(out float64 [B,H,Nq,D], nk int [B,Nq]): the definition in float64 on the logical cache k64, v64 [B,Hkv,Ncap,D]; decode_truth's mask"""
    B, H, Nq, D = q.shape
    Hkv, Ncap = k64.shape[1], k64.shape[2]
    G = H // Hkv
    out = np.zeros((B, H, Nq, D))
    nks = np.zeros((B, Nq), np.int64)
    for b in range(B):
        for i in range(Nq):
            nk = nks[b, i] = visible(lens[b], Nq, Ncap, causal, i)
            if nk == 0:
                continue
            for h in range(H):
                s = (k64[b, h // G, :nk] @ q[b, h, i].double()) / D ** 0.5
                p = torch.softmax(s, dim=0)
                out[b, h, i] = (p @ v64[b, h // G, :nk]).numpy()
    return out, nks


PIN_K_SCALES = (2.0, 4.0)           # K = +-1 is +-0.5 / +-0.25 in e4m3: a lost or foreign k_scale FLATTENS the softmax (12 -> 6, 3, 1.5 ...)
PIN_V_SCALES = (2.0 ** -2, 2.0 ** -3)


@functools.lru_cache(maxsize=8)
def seam_inputs_kv8(D, causal):
    """(q, k8, v8, k_scale, v_scale, lens): seam_inputs with the cache quantised.  K = +-1 is exact in
    e4m3 under PIN_K_SCALES, so the dominant score stays SCORE; V is randn rounded to e4m3"""
    q, k, v, lens = seam_inputs(D, causal)
    ks, vs = scales(PIN_K_SCALES, PIN_SHAPE[2]), scales(PIN_V_SCALES, PIN_SHAPE[2])
    k8, v8 = quantize(k, ks), quantize(v, vs)
    assert torch.equal(dequant(k8, ks), k)
    return q, k8, v8, ks, vs, lens


# ------------------------------------------------------------------------------------------------------------------------------------
# what the test modules of the three decode families repeat around a call

def _capi():
    capi.require_production()
    return capi


def _oracle():
    from tests import oracle_lib
    return oracle_lib.load()


def _dev_lens(lens):
    """kv_len on the GPU: None stays None (the contiguous call's "all of Ncap"), a tensor stays itself"""
    return lens if lens is None or torch.is_tensor(lens) else torch.tensor(list(lens), dtype=torch.int32, device="cuda")


def _cuda(*xs):
    return tuple(x if x is None or x.is_cuda else x.cuda() for x in xs)


def _lens_of(B, Hkv):
    lens = GRID_LENS[B]
    return tuple(reversed(lens)) if (B, Hkv) == (2, 4) else lens


def forced_split(split, call):
    """call() under "attn_decode_split" = split; the knob is back at 0 whatever happens"""
    capi.tune("attn_decode_split", split)
    try:
        return call()
    finally:
        capi.tune("attn_decode_split", 0)


def _run_split(split, q, o, call):
    """one decode call(q on the GPU, O) under a forced split, synchronised; returns O (NaN-prefilled unless given)"""
    qg, = _cuda(q)
    if o is None:
        o = torch.full_like(qg, float("nan"))
    forced_split(split, lambda: call(qg, o))
    torch.cuda.synchronize()
    return o


def run_flat(capi, q, k, v, lens, causal, split=0, workspace=None, o=None):
    """capi.attn_decode under a forced split"""
    kg, vg = _cuda(k, v)
    return _run_split(split, q, o, lambda qg, o: capi.attn_decode(qg, kg, vg, o, _dev_lens(lens), causal=causal, workspace=workspace))


def run_paged(capi, q, kp, vp, table, lens, causal, split=0, workspace=None, o=None):
    """capi.attn_decode_paged under a forced split"""
    kg, vg, tg = _cuda(kp, vp, table)
    return _run_split(split, q, o, lambda qg, o: capi.attn_decode_paged(qg, kg, vg, o, tg, _dev_lens(lens), causal=causal, workspace=workspace))


def run_kv8(capi, q, kp8, vp8, table, lens, ks, vs, causal, split=0, workspace=None, o=None):
    """capi.attn_decode_paged_kv8 under a forced split"""
    kg, vg, tg, ksg, vsg = _cuda(kp8, vp8, table, ks, vs)
    return _run_split(split, q, o,
                      lambda qg, o: capi.attn_decode_paged_kv8(qg, kg, vg, o, tg, _dev_lens(lens), ksg, vsg, causal=causal, workspace=workspace))


def reset_knobs():
    """the body of the CPU modules' `knobs` fixture: the library loaded, and the two knobs the tests move back at their defaults afterwards"""
    capi.load()
    yield
    capi.tune("attn_decode_split", 0)
    capi.tune("rule_cus", 0)


def _rc_name(symbol, *args):
    buf = C.create_string_buffer(128)
    rc = getattr(capi.load(), symbol)(*args, buf, 128)
    return rc, buf.value.decode()


def name_flat(B, H, Hkv, Nq, Ncap, D, flags=0):
    """(status, name) of lc_attn_decode_kernel_name"""
    return _rc_name("lc_attn_decode_kernel_name", B, H, Hkv, Nq, Ncap, D, flags)


def name_paged(B, H, Hkv, Nq, ps, mp, D, flags=0):
    return _rc_name("lc_attn_decode_paged_kernel_name", B, H, Hkv, Nq, ps, mp, D, flags)


def name_kv8(B, H, Hkv, Nq, ps, mp, D, flags=0):
    return _rc_name("lc_attn_decode_paged_kv8_kernel_name", B, H, Hkv, Nq, ps, mp, D, flags)


# ------------------------------------------------------------------------------------------------------------------------------------
# the exact-input classes (tests/test_abi_cpu_decode_exact.py proves their teeth, tests/test_gpu_decode_exact.py runs them)

DS = (64, 128)
LENS = (1024, 1000, 577, 130, 65, 64, 33, 32, 31, 16, 1, 0)
GRID = ((2, 2, 1), (8, 1, 1), (6, 2, 5), (2, 2, 17), (8, 2, 8), (6, 2, 11), (8, 2, 9), (6, 1, 8), (7, 1, 9), (2, 2, 64))      # (H, Hkv, Nq)
ROW_SHAPES = ((8, 1, 1), (2, 2, 17), (8, 2, 9), (7, 1, 9), (2, 2, 64))                # R, RT = (8, 1), (17, 2), (36, 4), (63, 4), (64, 4)
EXACT_PIN_LENS = (1000, 577, 130, 65, 33)
STEP_LENS = (1024, 1000, 577, 130)
EXACT_PLACES = ("last", "first_invisible", "key0", "tile_seam", "step_seam", "range_seam")
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
    return np.array([[visible(L, Nq, NCAP_POW2, causal, i) for i in range(Nq)] for L in lens], np.int64)


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
    vis = torch.arange(NCAP_POW2).view(1, 1, 1, NCAP_POW2) < torch.from_numpy(nks).view(B, 1, Nq, 1)
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
    k = torch.zeros(B, Hkv, NCAP_POW2, D)
    v = torch.zeros(B, Hkv, NCAP_POW2, D)
    for b in range(B):
        for kvh in range(Hkv):
            g = torch.Generator().manual_seed(_seed("uniform", D, H, Hkv, Nq, b, kvh))
            v[b, kvh] = _draw(g, V16, (NCAP_POW2, D))
            if kvh % 2 == 0:
                k[b, kvh] = _pm1(g, (NCAP_POW2, D))
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
    n = np.clip(nks, 0, NCAP_POW2)
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
        return pin_target(place, L, Nq, NCAP_POW2, causal, r, split)
    lim = visible(L, Nq, NCAP_POW2, causal, r % Nq)
    if lim < 33:
        return None                                     # no tile holds keys 31 and 32 of it below the limit
    t = (lim - 33) // 64
    return 64 * t + (31 if r % 2 == 0 else 32)


@functools.lru_cache(maxsize=4)
def exact_pinned_inputs(D, place, causal, H, Hkv, Nq, split=3, lens=EXACT_PIN_LENS):
    """(q, k, v, targets): fp16 CPU tensors and targets[b][h][i] (None: the row keeps its random query)"""
    B, G = len(lens), H // Hkv
    q = torch.empty(B, H, Nq, D)
    k = torch.empty(B, Hkv, NCAP_POW2, D)
    v = torch.empty(B, Hkv, NCAP_POW2, D)
    targets = [[[None] * Nq for _ in range(H)] for _ in range(B)]
    for b in range(B):
        for kvh in range(Hkv):
            g = torch.Generator().manual_seed(_seed("pinned", D, H, Hkv, Nq, b, kvh, 1 + 2 * EXACT_PLACES.index(place) + int(causal)))
            k[b, kvh] = _pm1(g, (NCAP_POW2, D))
            v[b, kvh] = torch.randn(NCAP_POW2, D, generator=g)
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
    q, k, v, _ = exact_pinned_inputs(D, place, causal, H, Hkv, Nq, split)
    return truth64(q, k, v, EXACT_PIN_LENS, causal)


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
    k = torch.zeros(B, Hkv, NCAP_POW2, D)
    v = torch.empty(B, Hkv, NCAP_POW2, D)
    c = torch.tensor(STEP_C)[torch.arange(G * Nq) % 3].view(G, Nq, 1)
    tiles = []
    for b, L in enumerate(STEP_LENS):
        tiles.append([])
        for kvh in range(Hkv):
            g = torch.Generator().manual_seed(_seed("step", D, H, Hkv, Nq, b, kvh))
            v[b, kvh] = _draw(g, V8, (NCAP_POW2, D))
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
    s = s.masked_fill(torch.arange(NCAP_POW2).view(1, -1) >= lims.view(-1, 1), ninf)
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
    kvh, L = h // G, min(max(int(lens[b]), 0), NCAP_POW2)
    nk = visible(L, Nq, NCAP_POW2, causal, i)
    tot = P[b, kvh, nk]

    def mean(x, n):
        return x / n if n > 0 else np.zeros_like(x)

    if nk >= 1:
        yield "limit one key short", mean(P[b, kvh, nk - 1], nk - 1)
    if nk < NCAP_POW2:
        yield "limit one key long", mean(P[b, kvh, nk + 1], nk + 1)
    for d in (-1, 1):
        n2 = min(visible(L, Nq, NCAP_POW2, causal, i + d), NCAP_POW2)
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
