"""What the bfloat16 ragged-batch test modules share (tests/test_abi_cpu_varlen_bf16.py, tests/test_gpu_varlen_bf16.py); not a test module and
not a conftest: nothing here is collected.  The references are the dtype-agnostic ones that exist — varlen_lib.ragged64, local_lib.local64 / Cache,
rope_lib.rope_ref, decode_lib.paginate / gather / quantize / OCP: each decodes its inputs with .double() / .float(), whatever their 16-bit
type — and what is added is what was fp16-specific: bf16 inputs and pools, the half ulp of a bf16 value, the row check under the project's
bf16 bound (tol.attn_close(bf16=True)), the names of the bf16 kernels and the ragged calls under a forced split."""
import numpy as np
import torch

from leetcuda_amd import capi
from tests import decode_lib as dl
from tests import local_lib as ll
from tests import varlen_lib as vl
from tests.decode_lib import _cuda, forced_split

BF = torch.bfloat16
DS = vl.DS
NCAP = vl.NCAP
KINDS = vl.KINDS
H, HKV = 8, 2
HEADS = torch.arange(H) // (H // HKV)
SENTINEL = -1232.0          # a bf16 value (77 x 16) no output row holds
SENT16 = 0x7BCD             # what a 16-bit pool holds before a rope call: a finite bf16 (2.13e36) no input reaches ...
SENT8 = 0x5A                # ... and a finite e4m3 code
ALL_V_SCALES = (1.0, 2.0 ** -3, 0.3, 1.7 / 448)       # per head, the all-patterns test: exact, a power of two, and two that are neither


def bits(x):
    """the raw bits of a 16-bit or 8-bit tensor, for torch.equal (NaN == NaN, -0 != 0)"""
    x = x.cpu()
    return x.view(torch.int16) if x.element_size() == 2 else x.view(torch.uint8)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def half_ulp_bf16(a):
    """2^(max(floor(log2 a), -126) - 8) for a >= 0 (float64): half the spacing of the bf16 values around a — 8 significand bits, fp32's exponent
    range; a = 0: the half ulp of the denormals, 2^-134"""
    _, ex = torch.frexp(a)                                                # a = m 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    fl = torch.where(a > 0, ex - 1, torch.full_like(ex, -126)).clamp(min=-126)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (fl - 8).double())


def rope_violations(got, exact, e):
    """bool, got's shape: where a stored bf16 value leaves |got - exact| <= e + half_ulp_bf16(|exact| + e) (rope_lib's derivation with the
    bf16 rounding in place of the fp16 one; a NaN leaves it)"""
    return ~((got.double() - exact).abs() <= e + half_ulp_bf16(exact.abs() + e))


def check_rows(out, truth, nvis, what=""):
    """every owned row under tol.attn_close(bf16=True) with N = the row's visible keys: |out - truth| <= tol.attn_max_abs(N, True) +
    tol.ATTN_RTOL_BF16 |truth|; a row without a visible key is exactly 0.  Returns the worst |err| / bound."""
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
        N = int(nvis[t])
        ok, err, excess = tol.attn_close(out[t], truth[t], N=N, bf16=True)
        bound = tol.attn_max_abs(N, True) + tol.ATTN_RTOL_BF16 * np.abs(truth[t])
        worst = max(worst, float((np.abs(out[t] - truth[t]) / bound).max()))
        assert ok, (what, f"token {t} nvis {N}: max |err| {err:.3e}, excess over the bound {excess:.3e}")
    return worst


def want_name(kind, Hq, Hkv, max_nq, D, S):
    """the fp16 plan's name with the bf16 kernel in it"""
    return vl.want_name(kind, Hq, Hkv, max_nq, D, S).replace("_kernel<", "_bf16_kernel<")


def dequant_bf16(codes, scale):
    """bf16: value(code) x scale — exact for a power-of-two scale (every e4m3 value has 4 significand bits)"""
    return (dl.OCP[codes.long()] * dl._per_head(scale, codes)).to(BF)


def bf16_cache(k, v, lens, ps=16, seed=5, **kw):
    """local_lib.Cache of a bf16 logical cache: bf16 pools (kp, vp, table) and, quantised from the bf16 values, e4m3 pools (kp8, vp8, table8)"""
    assert k.dtype == BF and v.dtype == BF
    return ll.Cache(k, v, lens, ps=ps, seed=seed, **kw)


def run(kind, c, q_tok, cu, lens, max_nq, causal=True, window=0, sinks=None, split=0, o=None, seqs=None, workspace=None):
    """varlen_lib.run on the bf16 entries: the ragged call of a cache kind on Cache c under a forced split, synchronised.  Returns O on the
    GPU (SENTINEL-prefilled unless given)."""
    seqs = list(range(len(lens))) if seqs is None else list(seqs)
    qg, = _cuda(q_tok)
    if o is None:
        o = torch.full_like(qg, SENTINEL)
    L = vl.dev_i32([lens[b] for b in seqs])
    cug = vl.dev_i32(cu)
    sk = None if sinks is None else (sinks if sinks.is_cuda else sinks.cuda())
    if kind == "paged":
        kp, vp, t = _cuda(c.kp, c.vp, c.table[seqs].contiguous())
        forced_split(split, lambda: capi.attn_varlen_paged_bf16(qg, kp, vp, o, cug, t, L, max_nq, causal=causal, window=window, sinks=sk,
                                                                workspace=workspace))
    else:
        kp, vp, t, ks, vs = _cuda(c.kp8, c.vp8, c.table8[seqs].contiguous(), c.ks, c.vs)
        forced_split(split, lambda: capi.attn_varlen_paged_kv8_bf16(qg, kp, vp, o, cug, t, L, max_nq, ks, vs, causal=causal, window=window,
                                                                    sinks=sk, workspace=workspace))
    torch.cuda.synchronize()
    return o


def token_positions(cu, lens, T, max_nq):
    """(seq int [T], pos int [T]): the sequence that owns token t (-1: nobody) and its position kv_len[b] - Nq_b + i"""
    seq = torch.full((T,), -1, dtype=torch.int64)
    pos = torch.zeros(T, dtype=torch.int64)
    for b, (q0, n) in enumerate(vl.owned(cu, T, max_nq)):
        seq[q0:q0 + n] = b
        pos[q0:q0 + n] = int(lens[b]) - n + torch.arange(n)
    return seq, pos


def pool_rows(pool, table, seq, pos):
    """[T,Hkv,D]: the pool row of every token (seq, pos as token_positions gives them; a token nobody owns or at a negative position: row 0 of
    page 0, to be masked by the caller)"""
    ps = pool.shape[2]
    ok = (seq >= 0) & (pos >= 0)
    pid = torch.where(ok, table[seq.clamp(min=0), (pos.clamp(min=0) // ps)].long(), torch.zeros_like(pos))
    return pool[pid, :, torch.where(ok, pos % ps, torch.zeros_like(pos))]


def written_mask(pool, table, seq, pos):
    """bool [P,Hkv,ps]: the pool rows the step owns"""
    ps = pool.shape[2]
    w = torch.zeros(pool.shape[:3], dtype=torch.bool)
    for t in range(len(seq)):
        if seq[t] >= 0 and pos[t] >= 0:
            w[int(table[seq[t], pos[t] // ps]), :, int(pos[t] % ps)] = True
    return w
