"""What the chunked-prefill test modules share (tests/test_abi_cpu_chunk.py, tests/test_gpu_chunk.py); not a test module and not a conftest: nothing
here is collected.  The inputs, the truth and the row check are tests/decode_lib.py's (decode_inputs, decode_truth, check_decode, paginate, gather,
quantize / dequant, scales, pin_target, forced_split): a chunk call is a decode call with R = (H / Hkv) x Nq > 64, and is held to the same bound.
New here: the shapes at which a row-block kernel can go wrong, the restatement of the plan (row blocks, L_blk, the split rule), the calls under a
forced split, pinned inputs at those shapes and the wrong row-block kernels they are meant to catch."""
import ctypes as C
import functools

import numpy as np
import torch

from leetcuda_amd import capi
from tests import decode_lib as dl
from tests.decode_lib import SCORE, _cuda, _dev_lens, decode_inputs, decode_truth, forced_split, gather, paginate, pin_target, visible

NCAP = dl.NCAP_RAGGED            # the contiguous cache: 1000 keys, a ragged last tile
NCAP_PAGED = dl.NCAP_POW2        # the paged caches: whole pages of every size; the logical contents are the contiguous cache's
LENS = (1000, 129, 65)           # B = 3
DS = (64, 128)
# (H, Hkv, Nq): R = 65 (a one-row last block, the 63 / 64 seam); 128 (aligned, two blocks in one head); 96 (block 0 straddles a head boundary, block 1
# is trimmed); 68 (G = 4, Nq divides nothing); 260 (five blocks, one straddling, a four-row tail); MQA, R = 128
SHAPES = ((2, 2, 65), (2, 2, 128), (4, 2, 48), (8, 2, 17), (2, 1, 130), (64, 1, 2))
SHORT_SHAPE, SHORT_LENS = (2, 1, 130), (40, 0, 130)      # kv_len < Nq: rows, and whole row blocks, without a visible key
SPLITS = (1, 3, 0)               # forced 1, forced 3, auto
PIN_SHAPES = ((4, 2, 48), (2, 1, 130))
PIN_LENS = (777, 300, 131)       # all >= Nq + 1 and < NCAP: every row has a visible and an invisible key
PIN_PLACES = ("last", "first_invisible")


def rows_of(H, Hkv, Nq):
    return (H // Hkv) * Nq


def rb_of(H, Hkv, Nq):
    """row blocks of 64 query rows per (batch, K / V head)"""
    return -(-rows_of(H, Hkv, Nq) // 64)


def i_max(H, Hkv, Nq, rb):
    """the last token a row of block rb holds: Nq - 1 where the block straddles a head boundary"""
    first, last = 64 * rb, min(rows_of(H, Hkv, Nq), 64 * rb + 64) - 1
    return Nq - 1 if first // Nq != last // Nq else last % Nq


def l_blk(L, H, Hkv, Nq, rb, causal, ncap):
    """the keys block rb walks"""
    L = min(max(int(L), 0), ncap)
    return min(max(L - Nq + i_max(H, Hkv, Nq, rb) + 1, 0), L) if causal else L


def auto_split(B, H, Hkv, Nq, ncap, cus):
    """the decode rule with B x Hkv x RB groups"""
    return dl.auto_split(B * Hkv * rb_of(H, Hkv, Nq), ncap, cus)


def seed_of(D, H, Hkv, Nq):
    return ((D * 131 + H) * 17 + Hkv) * 1009 + Nq


# ------------------------------------------------------------------------------------------------------------------------------------
# the grid: one set of inputs and one truth per (D, shape, causal, lens), shared by every test and never written to

@functools.lru_cache(maxsize=None)
def grid_inputs(D, shape, lens=LENS):
    """(q [B,H,Nq,D], k, v [B,Hkv,1024,D]) fp16 on the CPU; the contiguous call reads the first 1000 keys of k, v"""
    H, Hkv, Nq = shape
    return decode_inputs(len(lens), H, Hkv, Nq, NCAP_PAGED, D, seed=seed_of(D, H, Hkv, Nq) + sum(lens))


@functools.lru_cache(maxsize=None)
def grid_truth(D, shape, causal, lens=LENS):
    q, k, v = grid_inputs(D, shape, lens)
    return decode_truth(dl._oracle(), q, k[:, :, :NCAP].contiguous(), v[:, :, :NCAP].contiguous(), lens, causal)


@functools.lru_cache(maxsize=None)
def grid_flat(D, shape, lens=LENS):
    """(k, v [B,Hkv,1000,D]) on the GPU"""
    _, k, v = grid_inputs(D, shape, lens)
    return _cuda(k[:, :, :NCAP].contiguous(), v[:, :, :NCAP].contiguous())


@functools.lru_cache(maxsize=None)
def grid_pool(D, shape, ps, lens=LENS):
    """(k_pool, v_pool, table, gathered k, gathered v) on the GPU: NaN at every position >= L_b and in the spare pages"""
    _, k, v = grid_inputs(D, shape, lens)
    kp, vp, table = paginate(k, v, lens, ps, seed=ps + shape[2])
    return _cuda(kp, vp, table, gather(kp, table), gather(vp, table))


@functools.lru_cache(maxsize=None)
def grid_kv8(D, shape, ps, lens=LENS):
    """(k_pool8, v_pool8, table, k_scale, v_scale, dequantised k_pool, v_pool) on the GPU: the cache quantised under the power-of-two scales, then
    paged; the NaN code 0x7f at every position >= L_b and in the spare pages — NaN in the dequantised fp16 pools"""
    Hkv = shape[1]
    _, k, v = grid_inputs(D, shape, lens)
    ks, vs = dl.scales(dl.K_SCALES, Hkv), dl.scales(dl.V_SCALES, Hkv)
    kp8, vp8, table = paginate(dl.quantize(k, ks), dl.quantize(v, vs), lens, ps, seed=ps + shape[2], fill=dl.NAN_BYTE)
    return _cuda(kp8, vp8, table, ks, vs, dl.dequant(kp8, ks), dl.dequant(vp8, vs))


@functools.lru_cache(maxsize=None)
def grid_truth_kv8(D, shape, causal, lens=LENS):
    """the oracle on the DEQUANTISED cache (what the fp8 call is defined on)"""
    Hkv = shape[1]
    q, k, v = grid_inputs(D, shape, lens)
    ks, vs = dl.scales(dl.K_SCALES, Hkv), dl.scales(dl.V_SCALES, Hkv)
    kd, vd = dl.dequant(dl.quantize(k, ks), ks), dl.dequant(dl.quantize(v, vs), vs)
    return decode_truth(dl._oracle(), q, kd[:, :, :NCAP].contiguous(), vd[:, :, :NCAP].contiguous(), lens, causal)


# ------------------------------------------------------------------------------------------------------------------------------------
# the calls, under a forced split (0 = auto)

def run_flat(q, k, v, lens, causal, split=0, workspace=None, o=None):
    kg, vg = _cuda(k, v)
    return dl._run_split(split, q, o, lambda qg, o: capi.attn_chunk(qg, kg, vg, o, _dev_lens(lens), causal=causal, workspace=workspace))


def run_paged(q, kp, vp, table, lens, causal, split=0, workspace=None, o=None):
    kg, vg, tg = _cuda(kp, vp, table)
    return dl._run_split(split, q, o, lambda qg, o: capi.attn_chunk_paged(qg, kg, vg, o, tg, _dev_lens(lens), causal=causal, workspace=workspace))


def run_kv8(q, kp8, vp8, table, lens, ks, vs, causal, split=0, workspace=None, o=None):
    kg, vg, tg, ksg, vsg = _cuda(kp8, vp8, table, ks, vs)
    return dl._run_split(split, q, o,
                         lambda qg, o: capi.attn_chunk_paged_kv8(qg, kg, vg, o, tg, _dev_lens(lens), ksg, vsg, causal=causal, workspace=workspace))


def _rc_name(symbol, *args):
    buf = C.create_string_buffer(128)
    rc = getattr(capi.load(), symbol)(*args, buf, 128)
    return rc, buf.value.decode()


def name_flat(B, H, Hkv, Nq, Ncap, D, flags=0):
    """(status, name) of lc_attn_chunk_kernel_name"""
    return _rc_name("lc_attn_chunk_kernel_name", B, H, Hkv, Nq, Ncap, D, flags)


def name_paged(B, H, Hkv, Nq, ps, mp, D, flags=0):
    return _rc_name("lc_attn_chunk_paged_kernel_name", B, H, Hkv, Nq, ps, mp, D, flags)


def name_kv8(B, H, Hkv, Nq, ps, mp, D, flags=0):
    return _rc_name("lc_attn_chunk_paged_kv8_kernel_name", B, H, Hkv, Nq, ps, mp, D, flags)


def want_name(kind, H, Hkv, Nq, D, split):
    """kind: "", "_paged", "_paged_kv8".  R <= 64: the decode kernel's name"""
    base = f"attn_chunk{kind}_kernel<{D}>" if rows_of(H, Hkv, Nq) > 64 else f"attn_decode{kind}_kernel<{D},{dl.rt_of(H, Hkv, Nq)}>"
    return base + (f" x{split}" if split > 1 else "")


# ------------------------------------------------------------------------------------------------------------------------------------
# pinned inputs at row-block shapes, and the wrong row-block kernels

@functools.lru_cache(maxsize=8)
def pinned_inputs(D, shape, place, causal=True, lens=PIN_LENS):
    """(q, k, v): decode_lib.pinned_inputs' construction at a chunk shape, Ncap = 1000 — K random +-1, Q_row = (SCORE / sqrt(D)) K[target of the
    row] (decode_lib.pin_target), V randn; under `first_invisible` the target carries V = 8 K[target], a row no blend of other keys resembles"""
    H, Hkv, Nq = shape
    B, G = len(lens), H // Hkv
    g = torch.Generator().manual_seed(seed_of(D, H, Hkv, Nq) * 7 + PIN_PLACES.index(place) * 2 + int(causal))
    k = (torch.randint(0, 2, (B, Hkv, NCAP, D), generator=g) * 2 - 1).float()
    v = torch.randn(B, Hkv, NCAP, D, generator=g)
    q = torch.randn(B, H, Nq, D, generator=g)
    for b in range(B):
        for h in range(H):
            kvh, gq = h // G, h % G
            for i in range(Nq):
                t = pin_target(place, lens[b], Nq, NCAP, causal, gq * Nq + i, 3)
                if t is None:
                    continue
                q[b, h, i] = (SCORE / D ** 0.5) * k[b, kvh, t]
                if place == "first_invisible":
                    v[b, kvh, t] = 8.0 * k[b, kvh, t]
    return q.half(), k.half(), v.half()


def truth_by_row(oracle, q, k, v, lens, causal, nk_row=None):
    """(out fp32 [B,H,Nq,D], nk int [B,H,Nq]) with the visible keys of a row stated per ROW r = g Nq + i of its K / V head: nk_row(b, r) -> keys
    (None: the right mask).  One decode_truth call per query head — its nk_of hook is per token."""
    B, H, Nq, D = q.shape
    G = H // k.shape[1]
    out = np.zeros((B, H, Nq, D), np.float32)
    nks = np.zeros((B, H, Nq), np.int64)
    for h in range(H):
        kvh, g = h // G, h % G
        hook = (lambda b, i, g=g: nk_row(b, g * Nq + i)) if nk_row else None
        t, n = decode_truth(oracle, q[:, h:h + 1].contiguous(), k[:, kvh:kvh + 1].contiguous(), v[:, kvh:kvh + 1].contiguous(), lens, causal, nk_of=hook)
        out[:, h], nks[:, h] = t[:, 0], n
    return out, nks


def wrong_limits(shape, lens, causal=True, ncap=NCAP):
    """name -> nk_row(b, r) of a wrong row-block kernel (the limit it gives row r of a K / V head)"""
    H, Hkv, Nq = shape
    right = lambda b, r: visible(lens[b], Nq, ncap, causal, r % Nq)          # noqa: E731

    def local_row(b, r):            # lim from the block-local row index
        return visible(lens[b], Nq, ncap, causal, (r % 64) % Nq)

    def blk_for_all(b, r):          # L_blk used as every row's limit
        return l_blk(lens[b], H, Hkv, Nq, r // 64, causal, ncap)

    def last_row_imax(b, r):        # i_max taken from the block's last row although the block straddles: the walk ends early
        last = min(rows_of(H, Hkv, Nq), 64 * (r // 64) + 64) - 1
        L = min(max(int(lens[b]), 0), ncap)
        short = min(max(L - Nq + last % Nq + 1, 0), L) if causal else L
        return min(right(b, r), short)

    return {"lim from the block-local row": local_row, "L_blk as every row's limit": blk_for_all,
            "i_max from the last row of a straddling block": last_row_imax}, right


def block0_queries(q, Hkv):
    """the Q a kernel reads whose every block loads block 0's rows: row r of a K / V head's [R, D] matrix is row r % 64"""
    B, H, Nq, D = q.shape
    R = (H // Hkv) * Nq
    m = q.reshape(B, Hkv, R, D)
    return m[:, :, torch.arange(R) % 64].reshape(B, H, Nq, D).contiguous()
