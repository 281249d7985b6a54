"""The float64 reference of lc_attn_mla_paged_* and the paged latent cache it reads (tests/test_mla_gpu.py; not a test module)."""
import numpy as np
import torch

DC, DR = 512, 64
SM_SCALE = 1.0 / (DC + DR) ** 0.5     # unit-variance scores on randn inputs: the regime tests/tol.py was set in


def paged(lens, page, seed, el):
    """(ckv_pool [P,page,512], kpe_pool [P,page,64], table [B,max_pages]): randn pools, three spare pages, shuffled table, unused entries -1"""
    g = torch.Generator().manual_seed(seed)
    need = [(L + page - 1) // page for L in lens]
    P = sum(need) + 3
    ids = torch.randperm(P, generator=g).tolist()
    table = torch.full((len(lens), max(need + [1])), -1, dtype=torch.int32)
    for b, n in enumerate(need):
        table[b, :n] = torch.tensor([ids.pop() for _ in range(n)], dtype=torch.int32)
    return torch.randn(P, page, DC, generator=g).to(el), torch.randn(P, page, DR, generator=g).to(el), table


def ref64(q_c, q_pe, ckv_pool, kpe_pool, cu, table, lens, max_nq, sm_scale, causal):
    """(O [T,H,512], lse [T,H], A [T,H], nvis [T]) in float64: the cache gathered through the table, the masked softmax and its log-sum-exp.
    A = max over visible keys of sm_scale sum_d |q_d k_d| (for lse_lib.lse_bound); nvis = -1 for a row nobody owns (O, lse NaN)."""
    T, H, _ = q_c.shape
    page = ckv_pool.shape[1]
    O, lse, A, nvis = np.full((T, H, DC), np.nan), np.full((T, H), np.nan), np.zeros((T, H)), np.full(T, -1)
    q = torch.cat([q_c, q_pe], -1).double()
    for b, L in enumerate(lens):
        n = min(cu[b + 1] - cu[b], max_nq)
        pages = table[b, :(L + page - 1) // page].long()
        kv = torch.cat([ckv_pool[pages].reshape(-1, DC), kpe_pool[pages].reshape(-1, DR)], -1).double()[:L]
        for i in range(n):
            t, vis = cu[b] + i, max(0, min(L, L - n + i + 1) if causal else L)
            nvis[t] = vis
            if vis == 0:
                O[t], lse[t] = 0.0, -np.inf
                continue
            prod = q[t][:, None, :] * kv[None, :vis]
            s = prod.sum(-1) * sm_scale
            A[t] = (prod.abs().sum(-1) * sm_scale).max(-1).values.numpy()
            lse[t] = torch.logsumexp(s, -1).numpy()
            O[t] = (torch.softmax(s, -1) @ kv[:vis, :DC]).numpy()
    return O, lse, A, nvis
