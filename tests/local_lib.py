"""What the sliding-window / attention-sink test modules share (tests/test_abi_cpu_local.py, tests/test_gpu_local.py); not a test module and not a
conftest: nothing here is collected.  Built on tests/decode_lib.py (inputs, paginate, quantize / dequant, forced_split, SCORE): a local call is a
chunk call with a lower edge and one more term in the denominator.  New here: the float64 reference `local64` with its per-row count of visible keys,
the restatement of the plan (tile_lo, the split rule with a window), the three calls under a forced split, and the pinned inputs of the low edge."""
import ctypes as C
import functools

import numpy as np
import torch

from leetcuda_amd import capi
from tests import decode_lib as dl
from tests.decode_lib import SCORE, _cuda, _dev_lens, forced_split

DS = (64, 128)
NCAP = dl.NCAP_POW2
KINDS = ("flat", "paged", "kv8")


def span(L, Nq, Ncap, causal, window, i):
    """(lo, hi): query i of a batch entry with kv_len L sees keys lo .. hi - 1 (include/lc_abi.h: p - W < j <= p, clipped at key 0)"""
    hi = dl.visible(L, Nq, Ncap, causal, i)
    lo = max(0, hi - window) if window > 0 else 0
    return min(lo, hi), hi


def tile_lo(L, Nq, Ncap, window, i_min=0):
    """the first 64-key tile a workgroup whose lowest token is i_min walks"""
    L = min(max(int(L), 0), Ncap)
    return max(0, L - Nq + i_min + 1 - window) // 64 if window > 0 else 0


def auto_split(groups, ncap, Nq, window, cus):
    """decode_lib.auto_split with the tiles of min(Ncap, window + Nq - 1 + 63) keys when there is a window"""
    return dl.auto_split(groups, min(ncap, window + Nq - 1 + 63) if window > 0 else ncap, cus)


def local64(q, k64, v64, lens, causal, window=0, sinks=None):
    """(out float64 [B,H,Nq,D] numpy, nvis int [B,Nq]): the definition in float64 on the logical cache k64, v64 [B,Hkv,Ncap,D] — softmax64 with a
    low edge and, per query head, exp(sinks[h] - max) more in the denominator (sinks: None or a [H] tensor, natural units, never scaled)"""
    B, H, Nq, D = q.shape
    Hkv, Ncap = k64.shape[1], k64.shape[2]
    heads = torch.arange(H) // (H // Hkv)
    out = np.zeros((B, H, Nq, D))
    nvis = np.zeros((B, Nq), np.int64)
    j = torch.arange(Ncap).view(1, 1, Ncap)
    for b in range(B):
        lohi = [span(lens[b], Nq, Ncap, causal, window, i) for i in range(Nq)]
        nvis[b] = [hi - lo for lo, hi in lohi]
        lo = torch.tensor([x[0] for x in lohi]).view(1, Nq, 1)
        hi = torch.tensor([x[1] for x in lohi]).view(1, Nq, 1)
        k, v = torch.nan_to_num(k64[b].double())[heads], torch.nan_to_num(v64[b].double())[heads]      # (never-visible rows may hold NaN)
        s = (q[b].double() @ k.transpose(-2, -1)) / D ** 0.5                                            # [H, Nq, Ncap]
        s = s.masked_fill((j < lo) | (j >= hi), -float("inf"))
        if sinks is not None:
            s = torch.cat([s, sinks.double().view(H, 1, 1).expand(H, Nq, 1)], dim=-1)
        mx = s.max(dim=-1, keepdim=True).values
        p = torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
        l = p.sum(-1, keepdim=True)
        w = torch.where(l > 0, p / l.clamp(min=1e-300), torch.zeros_like(p))[..., :Ncap]
        out[b] = (w @ v).numpy()
    return out, nvis


def check_rows(out, truth, nvis, extra=0, what=""):
    """every row under tol.attn_close with N = the row's visible keys + extra (1: the sink term); a row without a visible key is exactly 0.
    Returns the worst |err| / bound."""
    from tests import tol
    out = np.asarray(out, np.float64)
    worst = 0.0
    B, H, Nq, D = truth.shape
    for b in range(B):
        for i in range(Nq):
            o, t = out[b, :, i], truth[b, :, i]
            if nvis[b, i] == 0:
                assert (o == 0).all(), (what, "row without a visible key is not 0", b, i)
                continue
            assert np.isfinite(o).all(), (what, "non-finite", b, i)
            N = int(nvis[b, i]) + extra
            ok, err, excess = tol.attn_close(o, t, N=N)
            bound = tol.attn_max_abs(N) + tol.ATTN_RTOL_F16 * np.abs(t)
            worst = max(worst, float((np.abs(o - t) / bound).max()))
            assert ok, (what, f"batch {b} query {i} nvis {N}: max |err| {err:.3e}, excess over the bound {excess:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# the calls

def _sinks_dev(sinks):
    return None if sinks is None else (sinks if sinks.is_cuda else sinks.cuda())


def run_flat(q, k, v, lens, causal, window=0, sinks=None, split=0, workspace=None):
    kg, vg = _cuda(k, v)
    return dl._run_split(split, q, None, lambda qg, o: capi.attn_local(qg, kg, vg, o, _dev_lens(lens), causal=causal, window=window,
                                                                      sinks=_sinks_dev(sinks), workspace=workspace))


def run_paged(q, kp, vp, table, lens, causal, window=0, sinks=None, split=0, workspace=None):
    kg, vg, tg = _cuda(kp, vp, table)
    return dl._run_split(split, q, None, lambda qg, o: capi.attn_local_paged(qg, kg, vg, o, tg, _dev_lens(lens), causal=causal, window=window,
                                                                            sinks=_sinks_dev(sinks), workspace=workspace))


def run_kv8(q, kp8, vp8, table, lens, ks, vs, causal, window=0, sinks=None, split=0, workspace=None):
    kg, vg, tg, ksg, vsg = _cuda(kp8, vp8, table, ks, vs)
    return dl._run_split(split, q, None, lambda qg, o: capi.attn_local_paged_kv8(qg, kg, vg, o, tg, _dev_lens(lens), ksg, vsg, causal=causal,
                                                                                window=window, sinks=_sinks_dev(sinks), workspace=workspace))


class Cache:
    """One logical cache [B,Hkv,NCAP,D] held the three ways: run(kind, q, lens, ...) calls the local entry of that kind, logical(kind) is the
    float64 cache that kind's kernel sees (kv8: the dequantised codes)."""

    def __init__(self, k, v, lens, ps=16, seed=5, k_scales=dl.K_SCALES, v_scales=dl.V_SCALES):
        Hkv = k.shape[1]
        self.k, self.v, self.lens, self.ps = k, v, lens, ps
        self.kp, self.vp, self.table = dl.paginate(k, v, lens, ps, seed=seed)
        self.ks, self.vs = dl.scales(k_scales, Hkv), dl.scales(v_scales, Hkv)
        self.k8, self.v8 = dl.quantize(k, self.ks), dl.quantize(v, self.vs)
        self.kp8, self.vp8, self.table8 = dl.paginate(self.k8, self.v8, lens, ps, seed=seed + 1, fill=dl.NAN_BYTE)

    def logical(self, kind):
        if kind == "kv8":
            return dl.dequant64(self.k8, self.ks), dl.dequant64(self.v8, self.vs)
        return self.k.double(), self.v.double()

    def run(self, kind, q, lens, causal, window=0, sinks=None, split=0):
        if kind == "flat":
            return run_flat(q, self.k, self.v, lens, causal, window, sinks, split)
        if kind == "paged":
            return run_paged(q, self.kp, self.vp, self.table, lens, causal, window, sinks, split)
        return run_kv8(q, self.kp8, self.vp8, self.table8, lens, self.ks, self.vs, causal, window, sinks, split)


# ------------------------------------------------------------------------------------------------------------------------------------
# the name calls

def _rc_name(symbol, *args):
    buf = C.create_string_buffer(128)
    rc = getattr(capi.load(), symbol)(*args, buf, 128)
    return rc, buf.value.decode()


def name(kind, B, H, Hkv, Nq, D, window, flags, ncap=NCAP, ps=16):
    """(status, name) of the name call of a cache kind ("flat", "paged", "kv8") at a capacity of ncap keys"""
    if kind == "flat":
        return _rc_name("lc_attn_local_kernel_name", B, H, Hkv, Nq, ncap, D, window, flags)
    sym = "lc_attn_local_paged_kernel_name" if kind == "paged" else "lc_attn_local_paged_kv8_kernel_name"
    return _rc_name(sym, B, H, Hkv, Nq, ps, ncap // ps, D, window, flags)


def nbytes(kind, B, H, Hkv, Nq, D, window, ncap=NCAP, ps=16):
    lib = capi.load()
    if kind == "flat":
        return lib.lc_attn_local_workspace_bytes(B, H, Hkv, Nq, ncap, D, window)
    sym = "lc_attn_local_paged_workspace_bytes" if kind == "paged" else "lc_attn_local_paged_kv8_workspace_bytes"
    return getattr(lib, sym)(B, H, Hkv, Nq, ps, ncap // ps, D, window)


def want_name(kind, H, Hkv, Nq, D, S, local=True):
    R = (H // Hkv) * Nq
    mid = {"flat": "", "paged": "_paged", "kv8": "_paged_kv8"}[kind]
    if R > 64:
        base = f"attn_local_chunk{mid}_kernel<{D}>" if local else f"attn_chunk{mid}_kernel<{D}>"
    else:
        base = f"attn_{'local' if local else 'decode'}{mid}_kernel<{D},{dl.rt_of(H, Hkv, Nq)}>"
    return base + (f" x{S}" if S > 1 else "")


# ------------------------------------------------------------------------------------------------------------------------------------
# the low edge, pinned: per row ONE key outweighs the rest (decode_lib's construction), placed either side of the row's low edge

EDGE_LENS = (1000, 936)      # (entry 1: every edge one tile lower, a ragged last tile of another length, other range seams)
# place -> (the lowest key token 0 of batch entry 0 sees, forced split).  Later tokens' edges follow one key apart, so a shape with Nq > 1 has
# rows either side of the seam a place names; token 0's own dominant key below the edge lies in a tile that is never loaded.
#   inside a tile; ON a 64-key tile seam (the key below it: the last of a tile that is not walked) and straddling one; straddling the 32-key
#   step seam of <128,4>; straddling the seam between ranges 0 and 1 of 8 (tile_lo = 6 of T = 16: ranges start at tiles 6, 7, 8, 9, 11 ...);
#   straddling a 16-key page seam that is no tile seam; W >= L: the edge is clipped at key 0
EDGE_PLACES = {"inside": (300, 3), "tile_seam": (320, 3), "tile_straddle": (317, 3), "step_straddle": (349, 1), "range_straddle": (445, 8),
               "page_straddle": (333, 3), "clipped": (None, 3)}


def edge_window(place, Nq):
    e0, split = EDGE_PLACES[place]
    L = EDGE_LENS[0]
    return (L + 5 if e0 is None else L - Nq + 1 - e0), split


@functools.lru_cache(maxsize=None)
def edge_inputs(D, shape, place, below):
    """(q, k, v, window, split): K random +-1, V randn, Q_row = (SCORE / sqrt(D)) K[target]; below: the target is p - W, the first key BELOW the
    row's window, and carries a large distinctive V row — else p - W + 1, its lowest key (clipped: key 0).  A row whose target does not exist
    (below key 0) keeps a random query."""
    H, Hkv, Nq = shape
    G, B = H // Hkv, len(EDGE_LENS)
    window, split = edge_window(place, Nq)
    g = torch.Generator().manual_seed(6151 * D + 97 * H + 13 * Nq + 2 * list(EDGE_PLACES).index(place) + int(below))
    k = (torch.randint(0, 2, (B, Hkv, NCAP, D), generator=g) * 2 - 1).float()
    v = torch.randn(B, Hkv, NCAP, D, generator=g)
    q = torch.randn(B, H, Nq, D, generator=g)
    big = torch.tensor([8.0, -8.0]).repeat(D // 2)
    for b, L in enumerate(EDGE_LENS):
        for i in range(Nq):
            lo, hi = span(L, Nq, NCAP, True, window, i)
            t = hi - window - 1 if below else lo
            if hi == 0 or t < 0:
                continue
            for h in range(H):
                q[b, h, i] = (SCORE / D ** 0.5) * k[b, h // G, t]
            if below:
                v[b, :, t] = big
    return q.half(), k.half(), v.half(), window, split
