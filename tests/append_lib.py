"""What the append-to-cache test modules share (tests/test_abi_cpu_kv_append.py, tests/test_gpu_kv_append.py); not a test module and not a
conftest: nothing here is collected.  The CPU reference `append_ref` (proved against decode_lib.paginate in the CPU module), `append_model` —
the reference on K and V together, or ONE wrong kernel restated — and the inputs of the GPU tests, built on the CPU so that the CPU module can
prove that they have teeth: the grid, the length edges, the table with bad and foreign page ids, every fp16 value."""
import functools

import torch

from tests.decode_lib import K_SCALES, V_SCALES, quantize, scales

B, HKV, NCAP = 3, 2, 1024
LENS = (777, 129, 65)                    # the lengths AFTER the append
DS = (64, 128)
PAGE_SIZES = (16, 64, 256)
GRID_NQ = (1, 4, 5, 16, 100)
KINDS = ("f16", "kv8", "kv8_null")       # fp16 pools; fp8 pools under K_SCALES / V_SCALES; fp8 pools with NULL scales (= 1.0)
SENT16 = 0x7BCD                          # what a pool holds before a call: a finite fp16 no randn input reaches (63904.0) ...
SENT8 = 0x5A                             # ... and a finite e4m3 code
GUARD = 4096                             # elements of sentinel either side of a pool on the GPU (a multiple of 16 bytes)
EDGE_NQ = 20
EDGE_LENS = (0, -5, 1, EDGE_NQ - 1, EDGE_NQ, EDGE_NQ + 1, 512, 511, 513, NCAP - 1, NCAP, NCAP + 7)      # 512: a page boundary of every page size
BAD_IDS = (-1, None, 2 ** 31 - 1)        # None: num_pages, the first id behind the pool
ALL_K_SCALES = (1.0, 2.0 ** -3, 4.0, 0.3)            # per head, test 4 (every fp16 value)
ALL_V_SCALES = (3.0, 2.0 ** 2, 1.7 / 448, 2.0 ** -5)
FAULTS = ("kv_swapped", "scales_swapped", "head0_scale", "reciprocal", "fnuz", "no_clamp", "len_before", "clamped_page", "row_mod16")


def append_ref(pool, new, table, lens, scale=None):
    """pool [P,Hkv,ps,D] (written in place and returned); new [B,Hkv,Nq,D] fp16; lens = the lengths AFTER the append; scale: None (fp16 pool) or
    a float / float32 [Hkv] tensor (uint8 pool of e4m3fn codes)"""
    P, Hkv, ps, D = pool.shape
    B, _, Nq, _ = new.shape
    mp = table.shape[1]
    src = new if scale is None else quantize(new, scale)
    for b in range(B):
        L = min(max(int(lens[b]), 0), mp * ps)
        for i in range(Nq):
            p = L - Nq + i
            if p < 0:
                continue
            pid = int(table[b, p // ps])
            if 0 <= pid < P:
                pool[pid, :, p % ps] = src[b, :, i]
    return pool


def _codes(x, scale, fault):
    """uint8 codes of fp16 x under a per-head scale, as the kernel (fault None) or one wrong kernel makes them"""
    s = scale.view(1, -1, 1, 1) if torch.is_tensor(scale) else torch.tensor(float(scale))
    if fault == "reciprocal":
        y = x.float() * (1.0 / s.float())                       # a rounded fp32 reciprocal, then a multiplication
    else:
        y = x.float() / s
    if fault == "fnuz":
        return y.clamp(-240.0, 240.0).to(torch.float8_e4m3fnuz).view(torch.uint8)
    if fault != "no_clamp":
        y = y.clamp(-448.0, 448.0)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def append_model(k_pool, v_pool, k_new, v_new, table, lens, k_scale=None, v_scale=None, fault=None):
    """(k_pool, v_pool) after one call, in place.  uint8 pools: the fp8 call (a scale of None = 1.0).  fault None: append_ref on both pools;
    otherwise ONE wrong kernel (FAULTS)."""
    kv8 = k_pool.dtype == torch.uint8
    P, Hkv, ps, D = k_pool.shape
    Bn, _, Nq, _ = k_new.shape
    mp = table.shape[1]
    ks = 1.0 if k_scale is None else k_scale
    vs = 1.0 if v_scale is None else v_scale
    if fault is None:
        append_ref(k_pool, k_new, table, lens, ks if kv8 else None)
        append_ref(v_pool, v_new, table, lens, vs if kv8 else None)
        return k_pool, v_pool
    if fault == "kv_swapped":
        k_new, v_new = v_new, k_new
    if fault == "scales_swapped":
        ks, vs = vs, ks
    if fault == "head0_scale":
        ks, vs = ks[:1].expand(Hkv), vs[:1].expand(Hkv)
    code_fault = fault if fault in ("reciprocal", "fnuz", "no_clamp") else None
    srcs = (_codes(k_new, ks, code_fault), _codes(v_new, vs, code_fault)) if kv8 else (k_new, v_new)
    for pool, src in zip((k_pool, v_pool), srcs):
        for b in range(Bn):
            L = min(max(int(lens[b]), 0), mp * ps)
            for i in range(Nq):
                p = L + i if fault == "len_before" else L - Nq + i
                if p < 0 or p >= mp * ps:
                    continue
                pid = int(table[b, p // ps])
                if fault == "clamped_page":
                    pid = min(max(pid, 0), P - 1)
                if 0 <= pid < P:
                    pool[pid, :, p % 16 if fault == "row_mod16" else p % ps] = src[b, :, i]
    return k_pool, v_pool


def sentinel_pools(P, Hkv, ps, D, kv8):
    """two pools [P,Hkv,ps,D] that hold the sentinel throughout: int16 bits viewed as fp16, or uint8"""
    if kv8:
        return tuple(torch.full((P, Hkv, ps, D), SENT8, dtype=torch.uint8) for _ in range(2))
    return tuple(torch.full((P, Hkv, ps, D), SENT16, dtype=torch.int16).view(torch.half) for _ in range(2))


def bits(pool):
    """the raw bits of a pool or an fp16 tensor, for torch.equal (NaN == NaN, -0 != 0)"""
    return pool.view(torch.int16) if pool.dtype == torch.half else pool.view(torch.uint8)


def make_table(Bn, mp, seed, spare=3):
    """(table int32 [Bn, mp], P): logical page p of entry b is pool page perm[b mp + p] of P = Bn mp + spare — a sequence's pages are
    scattered, non-monotone and interleaved with the other entries' (decode_lib.paginate's placement)"""
    P = Bn * mp + spare
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    return perm[:Bn * mp].view(Bn, mp).to(torch.int32).contiguous(), P


def kind_scales(kind, Hkv=HKV):
    """(k_scale, v_scale) float32 [Hkv] tensors, or (None, None)"""
    return (scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)) if kind == "kv8" else (None, None)


def new_rows(Bn, Hkv, Nq, D, seed):
    """(k_new, v_new) fp16 randn [Bn,Hkv,Nq,D], different from each other"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bn, Hkv, Nq, D, generator=g).half(), torch.randn(Bn, Hkv, Nq, D, generator=g).half()


@functools.lru_cache(maxsize=64)
def grid_inputs(D, ps, Nq):
    """(k_new, v_new, table, P, lens) of the grid test; shared, never written to"""
    k_new, v_new = new_rows(B, HKV, Nq, D, seed=1009 * D + 31 * ps + Nq)
    table, P = make_table(B, NCAP // ps, seed=ps + Nq)
    return k_new, v_new, table, P, LENS


@functools.lru_cache(maxsize=16)
def edge_inputs(D, ps):
    """(k_new, v_new, table, P, lens): twelve batch entries, one per length edge, EDGE_NQ tokens each"""
    Bn = len(EDGE_LENS)
    k_new, v_new = new_rows(Bn, HKV, EDGE_NQ, D, seed=7 * D + ps)
    table, P = make_table(Bn, NCAP // ps, seed=3 * ps + D + 1)
    return k_new, v_new, table, P, EDGE_LENS


def needed_pages(L, Nq, ps, mp):
    """the logical pages that hold a position of the Nq newest tokens of a sequence of length L"""
    L = min(max(int(L), 0), mp * ps)
    return sorted({p // ps for p in range(max(L - Nq, 0), L)})


@functools.lru_cache(maxsize=16)
def table_inputs(D, ps, Nq=100):
    """(k_new, v_new, table, P, lens, dropped): the grid's table with (a) a bad page id (-1, P, 2^31 - 1: one per batch entry) on the middle one
    of the pages each entry needs and (b) in every entry that holds none of the Nq positions the id of a page ANOTHER entry writes.
    dropped[b]: the positions of entry b that must stay unwritten."""
    k_new, v_new = new_rows(B, HKV, Nq, D, seed=11 * D + ps)
    mp = NCAP // ps
    good, P = make_table(B, mp, seed=5 * ps + D)
    table = good.clone()
    need = [needed_pages(LENS[b], Nq, ps, mp) for b in range(B)]
    written = [[int(good[b, p]) for p in need[b]] for b in range(B)]
    dropped = []
    for b in range(B):
        others = [pid for bb in range(B) if bb != b for pid in written[bb]]
        for p in range(mp):
            if p not in need[b]:
                table[b, p] = others[(7 * p + b) % len(others)]
        bad_page = need[b][len(need[b]) // 2]
        bad = BAD_IDS[b]
        table[b, bad_page] = P if bad is None else bad
        dropped.append([p for p in range(max(LENS[b] - Nq, 0), LENS[b]) if p // ps == bad_page])
    return k_new, v_new, table, P, LENS, dropped


@functools.lru_cache(maxsize=1)
def all_values_inputs():
    """(k_new, v_new [1,4,512,128] fp16, table, P, lens, k_scale, v_scale): every head's 65 536 elements are ALL fp16 bit patterns, shuffled; K and
    V use different shuffles; the per-head scales are ALL_K_SCALES / ALL_V_SCALES"""
    Hkv, Nq, D, ps = 4, 512, 128, 64
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16)          # (wraps: all 2^16 patterns)
    g = torch.Generator().manual_seed(65536)
    k_new = torch.stack([every[torch.randperm(65536, generator=g)] for _ in range(Hkv)]).view(1, Hkv, Nq, D).view(torch.half)
    v_new = torch.stack([every[torch.randperm(65536, generator=g)] for _ in range(Hkv)]).view(1, Hkv, Nq, D).view(torch.half)
    table, P = make_table(1, NCAP // ps, seed=64)
    return k_new, v_new, table, P, (Nq,), torch.tensor(ALL_K_SCALES), torch.tensor(ALL_V_SCALES)


def left_padded(x, lens, Nq):
    """[B,Hkv,Nq,D]: rows 0 .. L_b - 1 of x[b] ([B,Hkv,Ncap,D]) at the END of entry b's Nq tokens, a distinctive filler in front of them"""
    Bn, Hkv, _, D = x.shape
    out = torch.full((Bn, Hkv, Nq, D), -7.0, dtype=x.dtype)
    for b in range(Bn):
        L = int(lens[b])
        assert 0 <= L <= Nq
        if L:
            out[b, :, Nq - L:] = x[b, :, :L]
    return out
