"""What the log-sum-exp / state-merge test modules share (tests/test_abi_cpu_varlen_lse.py, tests/test_gpu_varlen_lse.py);
not a test module and not a conftest: nothing here is collected.  Built on tests/varlen_lib.py (owned, ragged64, run's conventions),
tests/bf16_lib.py (bits, the bf16 row check) and tests/local_lib.py (span, Cache) without editing them.  New here: the float64 log-sum-exp of a
ragged call with the quantities its error bound needs, that bound, an fp32 emulation of the kernel's arithmetic, the float64 merge `merge64`,
the names of the LSE kernels and the calls under a forced split."""
import functools
import math

import numpy as np
import torch

from leetcuda_amd import capi
from tests import bf16_lib as bl
from tests import local_lib as ll
from tests import varlen_lib as vl
from tests.decode_lib import _cuda, forced_split

BF = torch.bfloat16
DS = vl.DS
KINDS = vl.KINDS
NCAP = vl.NCAP
H, HKV = 8, 2
LN2_32 = np.float32(0.6931471805599453)
LOG2E_32 = np.float32(1.4426950408889634)
LSE_SENTINEL = -4321.5       # a float no log-sum-exp here reaches
U = 2.0 ** -24               # the unit roundoff of fp32

# the ragged batch of the GPU module's tests 1, 4 and 5 and of the CPU module's emulation: prompts of 37 / 70 / 5 tokens next to two decoding
# sequences; rows 114 .. 116 are nobody's
NQS = (37, 70, 5, 1, 1)
LENS = (100, 70, 260, 333, 64)
T_RAGGED = sum(NQS) + 3
MAX_NQ = 70                                                     # G max_nq = 280 rows: five row blocks
SINKS = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.5, -0.5, 0.25, 3.0])


def el_of(bf16):
    return BF if bf16 else torch.half


@functools.lru_cache(maxsize=None)
def cache(D, bf16, lens, seed=0):
    """local_lib.Cache of randn k, v [B,HKV,NCAP,D] in the element type (shared, never written to)"""
    g = torch.Generator().manual_seed(1009 * D + 31 * sum(lens) + 7 * seed + int(bf16))
    k, v = (torch.randn(len(lens), HKV, NCAP, D, generator=g).to(el_of(bf16)) for _ in range(2))
    return ll.Cache(k, v, lens, ps=16, seed=D + len(lens) + seed)


@functools.lru_cache(maxsize=None)
def tokens(D, bf16, T, seed=0):
    return torch.randn(T, H, D, generator=torch.Generator().manual_seed(77 * D + T + 13 * seed)).to(el_of(bf16))


def o_sentinel(dtype):
    return bl.SENTINEL if dtype == BF else vl.SENTINEL


def ulp32(x):
    """the spacing of the fp32 values at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def lse_name(twin):
    """the twin plan's name with `_lse` in the kernel's name: "..._kernel<" -> "..._lse_kernel<", "..._bf16_kernel<" -> "..._lse_bf16_kernel<" """
    return twin.replace("_bf16_kernel<", "_LSEBF<").replace("_kernel<", "_lse_kernel<").replace("_LSEBF<", "_lse_bf16_kernel<")


def want_name(kind, bf16, Hq, Hkv, max_nq, D, S):
    return lse_name((bl.want_name if bf16 else vl.want_name)(kind, Hq, Hkv, max_nq, D, S))


# ------------------------------------------------------------------------------------------------------------------------------------
# references

def lse64(q_tok, k64, cu, lens, max_nq, causal, window=0, sinks=None):
    """(lse float64 [T,H], A float64 [T,H], nvis int [T]) of a ragged call on the logical cache k64 [B,Hkv,Ncap,D] (float64):
    lse = ln(sum over the row's visible keys of exp(q.k / sqrt(D)) + exp(sink)), -inf for a row that sees nothing; A = max over the visible keys
    of sum_d |q_d k_jd| / sqrt(D), what bounds the rounding error of a score; nvis as varlen_lib.ragged64 (-1: a row nobody owns, lse NaN)."""
    T, Hq, D = q_tok.shape
    Hkv, Ncap = k64.shape[1], k64.shape[2]
    heads = torch.arange(Hq) // (Hq // Hkv)
    lse = np.full((T, Hq), np.nan)
    A = np.zeros((T, Hq))
    nvis = np.full((T,), -1, np.int64)
    for b, (q0, n) in enumerate(vl.owned(cu, T, max_nq)):
        for i in range(n):
            lo, hi = ll.span(lens[b], n, Ncap, causal, window, i)
            t = q0 + i
            nvis[t] = hi - lo
            k = torch.nan_to_num(k64[b].double())[heads][:, lo:hi]                      # [H, nk, D]
            prod = q_tok[t].double().unsqueeze(1) * k
            s = prod.sum(-1) / D ** 0.5
            if hi > lo:
                A[t] = (prod.abs().sum(-1) / D ** 0.5).max(dim=-1).values.numpy()
            if sinks is not None:
                s = torch.cat([s, sinks.double().view(Hq, 1)], dim=-1)
            lse[t] = torch.logsumexp(s, dim=-1).numpy() if s.shape[-1] else -np.inf
    return lse, A, nvis


def lse_bound(A, lse, nvis, D, sink=0.0):
    """The bound on |lse_gpu - lse64| of a row, derived, not tuned.  In units of u = 2^-24, natural-log domain:
      (D + 3) A       the fp32 accumulation of the D exact products of a score (first order, any order of summation) and the three roundings
                      of its scale: fl(log2 e / sqrt(D)), x k_scale, x the score.  A log-sum-exp moves by at most the largest score error
      2 |sink|        the sink's logit x fl(log2 e)
      n_vis + 26      the running sum l: one rounding per key (a sequential sum is the worst order), the rescales by alpha, the lane and wave
                      merges (<= 18 roundings), and at S > 1 the combine kernel's weights and sum (<= 8)
      2 + 2 ln(n_vis + 1)   v_exp_f32 and v_log_f32, one ulp each: 2 u relative on every term of l, 2 u relative on |log2 l| <= log2(n_vis + 1)
      2 |lse|         the roundings of m + log2 l and of the product with fl(ln 2)
    times a safety factor of 2 for the second-order terms and the subtraction x - m inside the exponentials."""
    nv = np.maximum(np.asarray(nvis, np.float64), 0.0)
    fin = np.where(np.isfinite(lse), np.abs(lse), 0.0)
    return 2.0 * U * ((D + 3) * A + 2.0 * abs(sink) + nv + 26.0 + 2.0 + 2.0 * np.log(nv + 1.0) + 2.0 * fin)


def emulate_lse32(q_tok, k, cu, lens, max_nq, causal, window=0, sinks=None, k_scale=None, only=None):
    """float64 [T,H] (NaN: a row nobody owns): the kernel's arithmetic for lse in numpy float32, one rounding where the kernel has one — the score
    as a sequential fp32 sum of the exact products, x fl(fl(log2 e / sqrt(D)) k_scale), m = the maximum (with the sink x fl(log2 e)), l = the
    sequential fp32 sum of fl(exp2(x - m)), lse = fl(fl(m + fl(log2 l)) fl(ln 2)).  k: the cache in the numbers the MFMA multiplies (codes for an
    fp8 pool, with k_scale float32 [Hkv]).  only: the tokens to compute (the others stay NaN)."""
    T, Hq, D = q_tok.shape
    Hkv, Ncap = k.shape[1], k.shape[2]
    G = Hq // Hkv
    out = np.full((T, Hq), np.nan)
    sl2 = np.float32(np.float32(1.0 / math.sqrt(D)) * LOG2E_32)      # (1 / sqrt(D) is exact for D = 64, rounded once for 128)
    qf = q_tok.float().numpy()
    kf = torch.nan_to_num(k.float()).numpy()
    for b, (q0, n) in enumerate(vl.owned(cu, T, max_nq)):
        for i in range(n):
            lo, hi = ll.span(lens[b], n, Ncap, causal, window, i)
            t = q0 + i
            if only is not None and t not in only:
                continue
            for h in range(Hq):
                kvh = h // G
                sc2 = sl2 if k_scale is None else np.float32(sl2 * np.float32(k_scale[kvh]))
                acc = np.zeros(hi - lo, np.float32)
                for d in range(D):
                    acc = (acc + kf[b, kvh, lo:hi, d] * qf[t, h, d]).astype(np.float32)
                x = (acc * sc2).astype(np.float32)
                terms = x
                if sinks is not None:
                    terms = np.concatenate([np.array([np.float32(sinks[h]) * LOG2E_32], np.float32), x])
                if terms.size == 0:
                    out[t, h] = -np.inf
                    continue
                m = terms.max()
                l = np.float32(0)
                for p in np.exp2((terms - m).astype(np.float32)).astype(np.float32):
                    l = np.float32(l + p)
                out[t, h] = np.float32(np.float32(m + np.float32(np.log2(l))) * LN2_32)
    return out


def merge64(oa, la, ob, lb):
    """(O float64 [..., D], lse float64 [...]) of two states over disjoint key sets: m = max(la, lb), w = exp(l - m),
    O = (wa Oa + wb Ob) / (wa + wb), lse = m + ln(wa + wb); both -inf: O = 0, lse = -inf"""
    oa, ob = np.asarray(oa, np.float64), np.asarray(ob, np.float64)
    la, lb = np.asarray(la, np.float64), np.asarray(lb, np.float64)
    m = np.maximum(la, lb)
    mu = np.where(np.isinf(m), 0.0, m)
    wa, wb = np.exp(la - mu), np.exp(lb - mu)
    ws = wa + wb
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where((ws > 0)[..., None], (wa[..., None] * oa + wb[..., None] * ob) / np.where(ws > 0, ws, 1.0)[..., None], 0.0)
        lse = np.where(ws > 0, m + np.log(np.where(ws > 0, ws, 1.0)), -np.inf)
    return o, lse


def attend64(q_row, k64, v64):
    """(O float64 [D], lse float64) of one query row over explicit float64 keys / values [n, D]: the direct softmax merge64 is checked against"""
    s = k64 @ q_row / math.sqrt(q_row.shape[0])
    if s.size == 0:
        return np.zeros(v64.shape[1]), -np.inf
    m = s.max()
    p = np.exp(s - m)
    return (p @ v64) / p.sum(), m + math.log(p.sum())


# the merge kernel's lse against merge64 on fp32 inputs: in units of u = 2^-24 — d = la - m and d x fl(log2 e): 2.5 u |t|
# on the exponent t, so <= 0.92 u on w = exp2(t) weighted by w (|t| 2^-|t| <= 0.531); v_exp_f32 one ulp: <= 1 u on ln(1 + w); the sum 1 + w: 1 u;
# v_log_f32 one ulp and the product with fl(ln 2): <= 2.43 u on a value <= ln 2 — 5.4 u, stated as 6 — and the final sum m + ...: half an ulp of lse
MERGE_LSE_ABS = 6 * U


def merge_lse_bound(lse):
    return MERGE_LSE_ABS + 0.5 * ulp32(np.where(np.isfinite(lse), lse, 0.0))


# ------------------------------------------------------------------------------------------------------------------------------------
# the calls

def run(kind, bf16, c, q_tok, cu, lens, max_nq, causal=True, window=0, sinks=None, split=0, o=None, lse=None, seqs=None, workspace=None,
        table=None):
    """the LSE ragged call of a cache kind and element type on ll.Cache c under a forced split, synchronised.  Returns (O, lse) on the GPU, both
    sentinel-prefilled unless given.  seqs: as varlen_lib.run; table: an explicit block table [len(seqs), pages] instead of c's rows."""
    seqs = list(range(len(lens))) if seqs is None else list(seqs)
    qg, = _cuda(q_tok)
    if o is None:
        o = torch.full_like(qg, o_sentinel(qg.dtype))
    if lse is None:
        lse = torch.full(tuple(qg.shape[:2]), LSE_SENTINEL, dtype=torch.float32, device="cuda")
    L = vl.dev_i32([lens[b] for b in seqs])
    cug = vl.dev_i32(cu)
    sk = None if sinks is None else (sinks if sinks.is_cuda else sinks.cuda())
    if kind == "paged":
        kp, vp, t = _cuda(c.kp, c.vp, (c.table[seqs] if table is None else table).contiguous())
        fn = capi.attn_varlen_paged_lse_bf16 if bf16 else capi.attn_varlen_paged_lse
        forced_split(split, lambda: fn(qg, kp, vp, o, cug, t, L, max_nq, lse=lse, causal=causal, window=window, sinks=sk, workspace=workspace))
    else:
        kp, vp, t, ks, vs = _cuda(c.kp8, c.vp8, (c.table8[seqs] if table is None else table).contiguous(), c.ks, c.vs)
        fn = capi.attn_varlen_paged_kv8_lse_bf16 if bf16 else capi.attn_varlen_paged_kv8_lse
        forced_split(split, lambda: fn(qg, kp, vp, o, cug, t, L, max_nq, lse=lse, k_scale=ks, v_scale=vs, causal=causal, window=window,
                                       sinks=sk, workspace=workspace))
    torch.cuda.synchronize()
    return o, lse


def run_twin(kind, bf16, *a, **kw):
    """the non-LSE twin: varlen_lib.run / bf16_lib.run"""
    return (bl.run if bf16 else vl.run)(kind, *a, **kw)


def inputs(B, T, D, seed, bf16, ncap=NCAP):
    """(q_tok [T,H,D], k, v [B,HKV,ncap,D]) randn in the element type"""
    g = torch.Generator().manual_seed(seed)
    el = BF if bf16 else torch.half
    return (torch.randn(T, H, D, generator=g).to(el), torch.randn(B, HKV, ncap, D, generator=g).to(el),
            torch.randn(B, HKV, ncap, D, generator=g).to(el))


def check_o(bf16, out, truth, nvis, extra=0, what=""):
    """the project's row check of the element type (varlen_lib.check_rows / bf16_lib.check_rows), unwidened"""
    if bf16:
        return bl.check_rows(out, truth, nvis, what=what)
    return vl.check_rows(out, truth, nvis, extra=extra, what=what)


def check_lse(got, want, A, nvis, D, sink=0.0, what=""):
    """every owned row of lse under lse_bound; a row that sees nothing is -inf.  Returns the worst |err| / bound."""
    got = np.asarray(got, np.float64)
    worst = 0.0
    for t in range(want.shape[0]):
        if nvis[t] < 0:
            continue
        inf = np.isinf(want[t])
        assert (got[t][inf] == -np.inf).all(), (what, "a row that sees nothing must have lse = -inf", t, got[t])
        if inf.all():
            continue
        err = np.abs(got[t][~inf] - want[t][~inf])
        bound = lse_bound(A[t][~inf], want[t][~inf], nvis[t], D, sink)
        assert np.isfinite(got[t][~inf]).all(), (what, "non-finite lse", t)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (what, f"token {t}: max |err| {err.max():.3e} over the bound {bound.min():.3e}")
    return worst
