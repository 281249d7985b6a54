"""What the ragged-batch test modules share (tests/test_abi_cpu_varlen.py, tests/test_gpu_varlen.py); not a test module and not a conftest: nothing
here is collected.  Built on tests/local_lib.py (Cache, local64, check_rows' bound) and tests/decode_lib.py: a ragged call is the local call of
every sequence on its own rows of a token-major [T,H,D] buffer.  New here: the restatement of the clamps and of the plan (RB, the groups of
the split rule), the float64 reference `ragged64`, and the calls under a forced split."""
import ctypes as C

import numpy as np
import torch

from leetcuda_amd import capi
from tests import decode_lib as dl
from tests import local_lib as ll
from tests.decode_lib import _cuda, forced_split

DS = (64, 128)
NCAP = ll.NCAP
KINDS = ("paged", "kv8")
SENTINEL = -1234.0          # an fp16 value no output row holds


def cu_of(nqs):
    """cu_q of a well-formed batch: [0, Nq_0, Nq_0 + Nq_1, ...]"""
    cu = [0]
    for n in nqs:
        cu.append(cu[-1] + int(n))
    return cu


def owned(cu, T, max_nq):
    """[(q0, Nq_b)] per sequence under the clamps of include/lc_abi.h: q0 = clamp(cu[b], 0, T), Nq_b = clamp(cu[b+1] - q0, 0, min(max_nq, T - q0))"""
    out = []
    for b in range(len(cu) - 1):
        q0 = min(max(int(cu[b]), 0), T)
        out.append((q0, min(max(int(cu[b + 1]) - q0, 0), min(max_nq, T - q0))))
    return out


def rb_of(H, Hkv, max_nq):
    return ((H // Hkv) * max_nq + 63) // 64


def groups(B, H, Hkv, T, max_nq):
    """the groups of the rule of S: Hkv x min(B RB, ceil(G T / 64) + B)"""
    G = H // Hkv
    return Hkv * min(B * rb_of(H, Hkv, max_nq), (G * T + 63) // 64 + B)


def auto_split(B, H, Hkv, T, max_nq, ncap, window, cus):
    return dl.auto_split(groups(B, H, Hkv, T, max_nq), min(ncap, window + max_nq - 1 + 63) if window > 0 else ncap, cus)


def want_name(kind, H, Hkv, max_nq, D, S):
    mid = {"paged": "_paged", "kv8": "_paged_kv8"}[kind]
    if (H // Hkv) * max_nq > 64:
        base = f"attn_varlen_chunk{mid}_kernel<{D}>"
    else:
        base = f"attn_varlen{mid}_kernel<{D},{dl.rt_of(H, Hkv, max_nq)}>"
    return base + (f" x{S}" if S > 1 else "")


def _rc_name(symbol, *args):
    buf = C.create_string_buffer(128)
    rc = getattr(capi.load(), symbol)(*args, buf, 128)
    return rc, buf.value.decode()


def name(kind, B, H, Hkv, T, max_nq, D, window, flags, ncap=NCAP, ps=16):
    sym = "lc_attn_varlen_paged_kernel_name" if kind == "paged" else "lc_attn_varlen_paged_kv8_kernel_name"
    return _rc_name(sym, B, H, Hkv, T, max_nq, ps, ncap // ps, D, window, flags)


def nbytes(kind, B, H, Hkv, T, max_nq, D, window, ncap=NCAP, ps=16):
    sym = "lc_attn_varlen_paged_workspace_bytes" if kind == "paged" else "lc_attn_varlen_paged_kv8_workspace_bytes"
    return getattr(capi.load(), sym)(B, H, Hkv, T, max_nq, ps, ncap // ps, D, window)


def to_tokens(q):
    """[B,H,Nq,D] -> token-major [B Nq, H, D]"""
    B, H, Nq, D = q.shape
    return q.permute(0, 2, 1, 3).reshape(B * Nq, H, D).contiguous()


def from_tokens(x, B, Nq):
    """token-major [B Nq, H, D] -> [B,H,Nq,D]"""
    _, H, D = x.shape
    return x.view(B, Nq, H, D).permute(0, 2, 1, 3).contiguous()


def ragged64(q_tok, k64, v64, cu, lens, max_nq, causal, window=0, sinks=None):
    """(out float64 [T,H,D] numpy, nvis int [T], -1: a row nobody owns): local_lib.local64 applied per sequence on its own rows"""
    T, H, D = q_tok.shape
    out = np.zeros((T, H, D))
    nvis = np.full((T,), -1, np.int64)
    for b, (q0, n) in enumerate(owned(cu, T, max_nq)):
        if n == 0:
            continue
        qb = q_tok[q0:q0 + n].permute(1, 0, 2).unsqueeze(0)                                  # [1,H,n,D]
        o, nv = ll.local64(qb, k64[b:b + 1], v64[b:b + 1], (lens[b],), causal, window=window, sinks=sinks)
        out[q0:q0 + n] = o[0].transpose(1, 0, 2)
        nvis[q0:q0 + n] = nv[0]
    return out, nvis


def check_rows(out, truth, nvis, extra=0, what=""):
    """every owned row under tol.attn_close with N = the row's visible keys + extra; a row without a visible key is exactly 0"""
    from tests import tol
    out = np.asarray(out, np.float64)
    worst = 0.0
    for t in range(truth.shape[0]):
        if nvis[t] < 0:
            continue
        if nvis[t] == 0:
            assert (out[t] == 0).all(), (what, "row without a visible key is not 0", t)
            continue
        assert np.isfinite(out[t]).all(), (what, "non-finite", t)
        N = int(nvis[t]) + extra
        ok, err, excess = tol.attn_close(out[t], truth[t], N=N)
        bound = tol.attn_max_abs(N) + tol.ATTN_RTOL_F16 * np.abs(truth[t])
        worst = max(worst, float((np.abs(out[t] - truth[t]) / bound).max()))
        assert ok, (what, f"token {t} nvis {N}: max |err| {err:.3e}, excess over the bound {excess:.3e}")
    return worst


def dev_i32(x):
    return x if torch.is_tensor(x) and x.is_cuda else torch.tensor([int(v) for v in x], dtype=torch.int32, device="cuda")


def run(kind, c, q_tok, cu, lens, max_nq, causal=True, window=0, sinks=None, split=0, o=None, seqs=None, workspace=None):
    """the ragged call of a cache kind on ll.Cache c under a forced split, synchronised.  seqs: the batch entries the call holds (their table rows
    and lengths; default all) — cu then has len(seqs) + 1 entries.  Returns O on the GPU (SENTINEL-prefilled unless given)."""
    seqs = list(range(len(lens))) if seqs is None else list(seqs)
    qg, = _cuda(q_tok)
    if o is None:
        o = torch.full_like(qg, SENTINEL)
    L = dev_i32([lens[b] for b in seqs])
    cug = dev_i32(cu)
    sk = None if sinks is None else (sinks if sinks.is_cuda else sinks.cuda())
    if kind == "paged":
        kp, vp, t = _cuda(c.kp, c.vp, c.table[seqs].contiguous())
        forced_split(split, lambda: capi.attn_varlen_paged(qg, kp, vp, o, cug, t, L, max_nq, causal=causal, window=window, sinks=sk,
                                                           workspace=workspace))
    else:
        kp, vp, t, ks, vs = _cuda(c.kp8, c.vp8, c.table8[seqs].contiguous(), c.ks, c.vs)
        forced_split(split, lambda: capi.attn_varlen_paged_kv8(qg, kp, vp, o, cug, t, L, max_nq, ks, vs, causal=causal, window=window, sinks=sk,
                                                               workspace=workspace))
    torch.cuda.synchronize()
    return o
