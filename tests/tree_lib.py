"""What the tree-speculation test modules share (tests/test_abi_cpu_tree.py, tests/test_gpu_varlen_tree.py); not a test module
and not a conftest: nothing here is collected.  Built on tests/lse_lib.py (caches, tokens, the lse bound, the row checks), tests/varlen_lib.py
(owned), tests/local_lib.py (span), tests/bf16_lib.py (token_positions, pool_rows) and tests/rope_lib.py (rope_ref) without editing them.
New here: random forests, the brute-force builders of the look-back words and of the rotary positions, the float64 reference `tree64`, which
takes visibility from the `parents` arrays and the definition — a token sees the prefix and, among the new tokens, itself and its ancestors —
and NEVER from the mask words, and the calls under a forced split."""
import numpy as np
import torch

from leetcuda_amd import capi
from tests import bf16_lib as bl
from tests import local_lib as ll
from tests import lse_lib as sl
from tests import varlen_lib as vl
from tests.decode_lib import _cuda, forced_split

H, HKV, NCAP = sl.H, sl.HKV, sl.NCAP
ONES = -1                     # a word of all ones, as the int64 the wrappers take
M64 = (1 << 64) - 1


def signed(word):
    """a 64-bit pattern as the int64 that holds the same bits"""
    word &= M64
    return word - (1 << 64) if word >> 63 else word


def words(ws, device=None):
    """int64 [T] from python ints (bit patterns or already signed)"""
    t = torch.tensor([signed(int(w)) for w in ws], dtype=torch.int64)
    return t if device is None else t.to(device)


def random_parents(n, rng, chain=0.0):
    """parents of a random tree of n tokens: parents[i] uniform in -1 .. i - 1 (with probability `chain`: i - 1, deeper trees)"""
    return [int(i - 1 if rng.random() < chain else rng.integers(-1, i)) for i in range(n)]


def ancestors(par, i):
    """the set {i} + the ancestors of token i"""
    out = set()
    while i >= 0:
        out.add(i)
        i = par[i]
    return out


def brute_mask(parents, cu):
    """python ints (bit patterns) [cu[-1]]: bit d of row i, straight from the definition, one (i, d) at a time"""
    out = [M64] * cu[-1]
    for b, par in enumerate(parents):
        if par is None:
            continue
        for i in range(len(par)):
            anc = ancestors(par, i)
            w = 0
            for d in range(64):
                if d > i or (i - d) in anc:
                    w |= 1 << d
            out[cu[b] + i] = w
    return out


def brute_positions(parents, cu, lens):
    out = [0] * cu[-1]
    for b, par in enumerate(parents):
        n = cu[b + 1] - cu[b]
        for i in range(n):
            out[cu[b] + i] = lens[b] - n + (i if par is None else len(ancestors(par, i)) - 1)
    return out


def visible(par, L, n, i, window=0, ncap=NCAP):
    """bool numpy [ncap]: the keys token i of a sequence with kv_len L and n new tokens sees — the causal span (with its window, in cache slots)
    and, among the n new keys L - n .. L - 1, only token i itself and its ancestors (par None: all of them)"""
    lo, hi = ll.span(L, n, ncap, True, window, i)
    vis = np.zeros(ncap, bool)
    vis[lo:hi] = True
    if par is not None:
        Lc = min(max(int(L), 0), ncap)
        anc = ancestors(par, i)
        for a in range(n):
            if a not in anc and 0 <= Lc - n + a < ncap:
                vis[Lc - n + a] = False
    return vis


def tree64(q_tok, k64, v64, cu, lens, max_nq, parents, window=0, sinks=None):
    """(out float64 [T,H,D], lse float64 [T,H], A float64 [T,H], nvis int [T]) of a tree call on the logical cache k64, v64 [B,Hkv,Ncap,D]:
    the softmax over `visible`'s keys (+ the sink in the denominator); lse, A and nvis as lse_lib.lse64 gives them (-1: a row nobody owns)"""
    T, Hq, D = q_tok.shape
    Hkv, ncap = k64.shape[1], k64.shape[2]
    heads = torch.arange(Hq) // (Hq // Hkv)
    out = np.zeros((T, Hq, D))
    lse = np.full((T, Hq), np.nan)
    A = np.zeros((T, Hq))
    nvis = np.full((T,), -1, np.int64)
    for b, (q0, n) in enumerate(vl.owned(cu, T, max_nq)):
        kb, vb = torch.nan_to_num(k64[b].double())[heads], torch.nan_to_num(v64[b].double())[heads]     # [H, ncap, D]
        for i in range(n):
            t = q0 + i
            vis = torch.from_numpy(visible(parents[b], lens[b], n, i, window, ncap))
            nvis[t] = int(vis.sum())
            k, v = kb[:, vis], vb[:, vis]
            prod = q_tok[t].double().unsqueeze(1) * k
            s = prod.sum(-1) / D ** 0.5                                                                  # [H, nvis]
            if nvis[t]:
                A[t] = (prod.abs().sum(-1) / D ** 0.5).max(dim=-1).values.numpy()
            full = s if sinks is None else torch.cat([s, sinks.double().view(Hq, 1)], dim=-1)
            if full.shape[-1] == 0:
                lse[t] = -np.inf
                continue
            l = torch.logsumexp(full, dim=-1)
            lse[t] = l.numpy()
            out[t] = (torch.exp(s - l[:, None]).unsqueeze(1) @ v).squeeze(1).numpy()
    return out, lse, A, nvis


def want_name(kind, bf16, Hq, Hkv, max_nq, D, S):
    """the LSE plan's name with `tree` in place of `lse`"""
    return sl.want_name(kind, bf16, Hq, Hkv, max_nq, D, S).replace("_lse_", "_tree_")


def fn_of(kind, bf16):
    if kind == "paged":
        return capi.attn_varlen_paged_tree_bf16 if bf16 else capi.attn_varlen_paged_tree
    return capi.attn_varlen_paged_kv8_tree_bf16 if bf16 else capi.attn_varlen_paged_kv8_tree


def run(kind, bf16, c, q_tok, cu, lens, max_nq, mask, window=0, sinks=None, split=0, o=None, lse=None, workspace=None):
    """lse_lib.run on the tree entries (always causal): mask int64 [T] (CPU or GPU).  Returns (O, lse) on the GPU, sentinel-prefilled unless given."""
    qg, mg = _cuda(q_tok, mask)
    if o is None:
        o = torch.full_like(qg, sl.o_sentinel(qg.dtype))
    if lse is None:
        lse = torch.full(tuple(qg.shape[:2]), sl.LSE_SENTINEL, dtype=torch.float32, device="cuda")
    L, cug = vl.dev_i32(lens), vl.dev_i32(cu)
    sk = None if sinks is None else (sinks if sinks.is_cuda else sinks.cuda())
    if kind == "paged":
        kp, vp, t = _cuda(c.kp, c.vp, c.table.contiguous())
        forced_split(split, lambda: fn_of(kind, bf16)(qg, kp, vp, o, cug, t, L, max_nq, mg, lse=lse, window=window, sinks=sk, workspace=workspace))
    else:
        kp, vp, t, ks, vs = _cuda(c.kp8, c.vp8, c.table8.contiguous(), c.ks, c.vs)
        forced_split(split, lambda: fn_of(kind, bf16)(qg, kp, vp, o, cug, t, L, max_nq, mg, lse=lse, k_scale=ks, v_scale=vs, window=window,
                                                      sinks=sk, workspace=workspace))
    torch.cuda.synchronize()
    return o, lse


# ---- rotary embedding + append with per-token positions

def rope_fn(kv8, bf16, pos):
    name = "rope_append_varlen" + ("_pos" if pos else "") + ("_kv8" if kv8 else "") + ("_bf16" if bf16 else "")
    return getattr(capi, name)


def rope_call(kv8, bf16, q, k_new, v_new, pools, cs, cu, pos_ids, table, lens, max_nq, q_out, interleaved=False, scales=None):
    """the _pos_ rope call (pos_ids None: its twin) on GPU tensors, synchronised; returns q_out"""
    fn = rope_fn(kv8, bf16, pos_ids is not None)
    pos = () if pos_ids is None else (pos_ids,)
    out = fn(q, k_new, v_new, pools[0], pools[1], cs, vl.dev_i32(cu), *pos, table, vl.dev_i32(lens), max_nq, q_out=q_out, interleaved=interleaved,
             **(scales or {}))
    torch.cuda.synchronize()
    return out


def rope_exact(x_tok, pos, table, interleaved):
    """rope_lib.rope_ref on token-major rows x [T,heads,D] at per-token positions pos [T]: (exact, e) float64 [T,heads,D]"""
    from tests import rope_lib as rl
    exact, e = rl.rope_ref(x_tok.permute(1, 0, 2).unsqueeze(0), pos.view(1, -1), table, interleaved)
    return exact[0].permute(1, 0, 2), e[0].permute(1, 0, 2)


def rope_violations(bf16, got, exact, e):
    from tests import rope_lib as rl
    return bl.rope_violations(got, exact, e) if bf16 else rl.violations(got, exact, e)
