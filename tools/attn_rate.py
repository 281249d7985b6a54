#!/usr/bin/env python3
"""Sustained rate of the attention forward at arbitrary shapes, interleaved A/B over tuning knobs.
usage: attn_rate.py [--seconds S] [--rounds R] spec...
   spec = B,H,N,D[:q=Nq][:len=L][:dsplit=S][:page=P[:kv8][:append[:torch] | :rope[:torch]]] | B,H,N,D[:bf16][:zero][:vt][:causal][:sdpa][:kvh=K][:expand][:expanded][:nw=K][:walk=K][:split=K][:d512=K][:sched=K][:order=K]   (vt = V handed over as [B,H,D,N];
          causal = the causal mask (lc_attn_fwd_f16_ex); sdpa = torch.nn.functional.scaled_dot_product_attention on the same inputs
          instead of this library (context only); kvh = K: grouped-query attention, K / V tensors with K heads through lc_attn_fwd_f16_gqa
          (FLOPs counted as for the H query heads); kvh = K with expand: what a caller without that entry does — repeat_interleave K and V
          to H heads in every step, then the MHA call; kvh = K with expanded: the MHA call on K / V expanded once, outside the timing
          (the same values through the MHA kernel: the reference for the GQA kernel's time); knobs = lc_tune_set keys attn_nw / attn_walk / attn_split / attn_d512 /
          attn_w4i_sched / attn_causal_order)
   q = Nq: DECODE attention through lc_attn_decode_f16 — Nq query tokens per sequence against a KV cache of capacity N with kvh = K heads
          (default K = H); len = L: every batch entry's kv_len (default N); dsplit = S: "attn_decode_split"; causal: the bottom-right aligned
          mask; with sdpa: scaled_dot_product_attention on k[:, :, :L] / v[:, :, :L] (enable_gqa where this torch has it, else on K / V
          expanded once outside the timing; non-causal only: torch's is_causal is top-left aligned).  Decode rows report microseconds per
          call (median, best, worst over the rounds) and K / V GB/s = 2 B K L D 2 bytes / median time
          page = P (with q): the same logical cache scattered over a randomly permuted pool of N / P pages of P keys per sequence, through
          lc_attn_decode_paged_f16 and a block table (combinable with q, len, dsplit, causal; N % P == 0)
          kv8 (with page): that pool quantised to e4m3 with one scale per K / V head (amax / 448), through lc_attn_decode_paged_kv8; its
          K / V GB/s count one byte per element
          q = Nq with (H / K) x Nq > 64 rows per K / V head: the CHUNK calls (lc_attn_chunk_f16 / _paged_f16 / _paged_kv8) — same options; their sdpa
          arm takes causal too, as a boolean bottom-right mask built once outside the timing
          append (with page): instead of the decode call, the APPEND of the q = Nq newest tokens of every sequence (positions L - Nq .. L - 1)
          to that pool through lc_kv_append_paged_f16 (kv8: lc_kv_append_paged_kv8); append:torch: the same job in torch ops — an index_put_
          of the rows into the pool viewed as rows (indices computed outside the timing), preceded for kv8 by
          (x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn).  Their GB/s count the bytes read + written
          rope (with page): rotary embedding + append in ONE call — the q = Nq newest tokens of every sequence as a token-major projection
          output [B,Nq,(H + 2 K) D] through lc_rope_append_paged_f16 / _kv8 (LC_ROPE_PACKED_SRC, NeoX pairs, rot_dim = D, a base-10000 table
          of N rows): rotated Q [B,H,Nq,D] out, rotated K and V into the pool.  rope:torch: the same job in torch ops — split, transpose,
          positions from kv_len, gather the table rows, rotate Q and K in fp32 — followed by kv_append_paged(_kv8).  Their GB/s count the
          bytes read + written: (H + 2 K) D fp16 in, H D fp16 + 2 K D pool elements out per token
Every spec runs >= S seconds of back-to-back launches per round; R rounds interleave the specs (within-probe A/B,
cdna_hip_programming.md rule 24); prints the kernel name the dispatcher reports, median and best TFLOP/s (matmul FLOPs: 4 B H N^2 D;
causal: half of that, the flash-attn convention) and the median time per call."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from leetcuda_amd import capi, host  # noqa: E402

args = sys.argv[1:]
secs, rounds = 1.0, 3
while args and args[0].startswith("--"):
    if args[0] == "--seconds":
        secs = float(args[1])
    elif args[0] == "--rounds":
        rounds = int(args[1])
    else:
        raise SystemExit(f"unknown option {args[0]}")
    args = args[2:]
import os  # noqa: E402
if os.environ.get("LC_AB_LIB"):    # A/B of two builds on one box: point the ctypes view at another copy of the library
    capi.LIB_PATH = Path(os.environ["LC_AB_LIB"]).resolve()
    import ctypes  # noqa: E402
    other = ctypes.CDLL(str(capi.LIB_PATH))             # an older build lacks the entries added since: the specs that need one fail, the rest run
    for missing in [s for s in capi.SYMBOLS if not hasattr(other, s)]:
        del capi.SYMBOLS[missing]
capi.load()
KNOBS = {"bigd_stagger": "attn_bigd_stagger", "bigd_map": "attn_bigd_map", "nw": "attn_nw", "walk": "attn_walk", "d512": "attn_d512", "d1024": "attn_d1024", "sched": "attn_w4i_sched", "split": "attn_split",
         "order": "attn_causal_order", "dsplit": "attn_decode_split"}
cache = {}


def tensors(B, H, N, D, bf16, zero, kvh=0):
    key = (B, H, N, D, bf16, zero, kvh)
    if key not in cache:
        cache.clear()                                   # one shape resident at a time
        torch.manual_seed(0)
        dt = torch.bfloat16 if bf16 else torch.half
        mk = (lambda: torch.zeros(B, H, N, D, device="cuda", dtype=dt)) if zero else \
             (lambda: torch.randn(B, H, N, D, device="cuda").to(dt))
        cache[key] = (mk(), mk(), mk(), torch.zeros(B, H, N, D, device="cuda", dtype=dt))
        if kvh:                                         # K / V [B, kvh, N, D]: the first kvh heads of the same random data
            q, k, v, o = cache[key]
            cache[key] = (q, k[:, :kvh].contiguous(), v[:, :kvh].contiguous(), o)
    return cache[key]


def timed(step):
    """ms per call of `step` over >= secs seconds of back-to-back calls"""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        step()
    e1.record()
    torch.cuda.synchronize()
    n = max(5, int(secs / (e0.elapsed_time(e1) / 5 * 1e-3)))
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def opt_int(opts, key, default):
    return next((int(o.split("=")[1]) for o in opts if o.startswith(key + "=")), default)


def run_append(spec, shape, use_torch, kv8, pool, lens):
    """(name, bytes read + written in GB/s, ms per call) of appending the q = Nq newest tokens of every sequence to the spec's pools: through
    lc_kv_append_paged_f16 / _kv8, or (torch) an index_put_ of the rows into the pool viewed as rows — the row indices computed once, outside
    the timing — preceded for fp8 by the quantisation in torch ops"""
    B, kvh, nq, N, D, L, page = shape
    k_pool, v_pool, table, k_scale, v_scale = pool
    akey = ("append", B, kvh, nq, D)
    if akey not in cache:
        for old_key in [x for x in cache if x[0] == "append"]:
            del cache[old_key]
        g = torch.Generator(device="cuda").manual_seed(nq)
        cache[akey] = tuple(torch.randn(B, kvh, nq, D, device="cuda", generator=g).half() for _ in range(2))
    k_new, v_new = cache[akey]
    if use_torch:
        pos = torch.arange(L - nq, L, device="cuda")                                                          # [nq]
        pid = table.long()[:, pos // page]                                                                     # [B, nq]
        idx = ((pid.view(B, 1, nq) * kvh + torch.arange(kvh, device="cuda").view(1, kvh, 1)) * page + (pos % page).view(1, 1, nq)).reshape(-1)
        as_rows = (lambda x: x.view(torch.uint8).view(-1, D)) if kv8 else (lambda x: x.view(-1, D))
        k_rows, v_rows = as_rows(k_pool), as_rows(v_pool)
        if kv8:
            ks, vs = k_scale.view(1, kvh, 1, 1), v_scale.view(1, kvh, 1, 1)
            quant = lambda x, s: (x.float() / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).view(-1, D)  # noqa: E731

            def step():
                k_rows.index_put_((idx,), quant(k_new, ks))
                v_rows.index_put_((idx,), quant(v_new, vs))
        else:
            def step():
                k_rows.index_put_((idx,), k_new.view(-1, D))
                v_rows.index_put_((idx,), v_new.view(-1, D))
        name = "torch index_put_" + (" after quantise" if kv8 else "")
    else:
        name = capi.kv_append_paged_kernel_name(B, kvh, nq, page, N // page, D, kv8=kv8)
        if kv8:
            step = lambda: capi.kv_append_paged_kv8(k_new, v_new, k_pool, v_pool, table, lens, k_scale, v_scale)  # noqa: E731
        else:
            step = lambda: capi.kv_append_paged(k_new, v_new, k_pool, v_pool, table, lens)  # noqa: E731
    ms = timed(step)
    return name, 2.0 * B * kvh * nq * D * (2 + (1 if kv8 else 2)) / ms * 1e-6, ms


def run_rope(spec, shape, use_torch, kv8, pool, lens):
    """(name, bytes read + written in GB/s, ms per call) of rotating Q and K of the q = Nq newest tokens and appending K and V to the spec's
    pools: the fused call on a packed projection output, or (torch) the same job in torch ops followed by kv_append_paged(_kv8)"""
    B, H, kvh, nq, N, D, L, page = shape
    k_pool, v_pool, table, k_scale, v_scale = pool
    rkey = ("rope", B, H, kvh, nq, N, D)
    if rkey not in cache:
        for old_key in [x for x in cache if x[0] == "rope"]:
            del cache[old_key]
        g = torch.Generator(device="cuda").manual_seed(nq + 1)
        cache[rkey] = (torch.randn(B, nq, (H + 2 * kvh) * D, device="cuda", generator=g).half(), capi.rope_table(N, D).cuda(),
                       torch.empty(B, H, nq, D, device="cuda", dtype=torch.half))
    qkv, cs, q_out = cache[rkey]
    if use_torch:
        half = D // 2
        append = (lambda k, v: capi.kv_append_paged_kv8(k, v, k_pool, v_pool, table, lens, k_scale, v_scale)) if kv8 else \
                 (lambda k, v: capi.kv_append_paged(k, v, k_pool, v_pool, table, lens))

        def rotate(x, c, s):                                                         # x [B,heads,nq,D] fp16; c, s [B,1,nq,D/2] fp32
            x1, x2 = x[..., :half].float(), x[..., half:].float()
            return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).half()

        def step():
            parts = qkv.view(B, nq, H + 2 * kvh, D).transpose(1, 2)
            pos = (lens.long().view(B, 1) - nq + torch.arange(nq, device="cuda").view(1, nq)).clamp(0, N - 1)
            rows = cs[pos].view(B, 1, nq, D)
            c, s = rows[..., :half], rows[..., half:]
            q_out.copy_(rotate(parts[:, :H], c, s))
            append(rotate(parts[:, H:H + kvh], c, s), parts[:, H + kvh:].contiguous())
        name = "torch rope + " + capi.kv_append_paged_kernel_name(B, kvh, nq, page, N // page, D, kv8=kv8)
    else:
        name = capi.rope_append_paged_kernel_name(B, H, kvh, nq, page, N // page, D, D, N, kv8=kv8, src_row_stride=(H + 2 * kvh) * D)
        step = lambda: capi.rope_append_paged_qkv(qkv, H, kvh, k_pool, v_pool, cs, table, lens, q_out=q_out, k_scale=k_scale, v_scale=v_scale)  # noqa: E731
    ms = timed(step)
    return name, 1.0 * B * nq * D * ((H + 2 * kvh) * 2 + H * 2 + 2 * kvh * (1 if kv8 else 2)) / ms * 1e-6, ms


def run_decode(spec, shape, opts):
    """(name, K / V GB/s, ms per call) of one decode call"""
    B, H, N, D = shape
    nq, kvh, L, causal = opt_int(opts, "q", 1), opt_int(opts, "kvh", H), opt_int(opts, "len", N), "causal" in opts
    key = ("decode", B, H, N, D, kvh, nq)
    if key not in cache:
        cache.clear()
        torch.manual_seed(0)
        mk = lambda *s: torch.randn(*s, device="cuda").half()  # noqa: E731
        cache[key] = (mk(B, H, nq, D), mk(B, kvh, N, D), mk(B, kvh, N, D), torch.zeros(B, H, nq, D, device="cuda", dtype=torch.half))
    q, k, v, o = cache[key]
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    split = opt_int(opts, "dsplit", 0)
    page = opt_int(opts, "page", 0)
    kv8 = "kv8" in opts
    chunk = (H // kvh) * nq > 64
    if kv8 and not page:
        raise SystemExit(f"{spec}: kv8 needs page=P")
    if page:
        if N % page or "sdpa" in opts:
            raise SystemExit(f"{spec}: page needs N % page == 0 and this library")
        pkey = ("pool", page, kv8) + key
        if pkey not in cache:                           # (the contiguous cache stays resident: both arms of an A/B read the same values;
            for old_key in [x for x in cache if x[0] == "pool" and x[1] != page]:      # so do the fp16 and the fp8 pool of one page size)
                del cache[old_key]
            mp = N // page
            perm = torch.randperm(B * mp, device="cuda", generator=torch.Generator(device="cuda").manual_seed(page))
            pools = []
            for x in (k, v):
                pool = torch.empty(B * mp, kvh, page, D, device="cuda", dtype=torch.half)
                pool[perm] = x.view(B, kvh, mp, page, D).permute(0, 2, 1, 3, 4).reshape(B * mp, kvh, page, D)
                pools.append(pool)
            sc = [None, None]
            if kv8:                                     # per-head scales that map the head's largest magnitude onto e4m3's largest, 448
                sc = [(x.float().abs().amax(dim=(0, 2, 3)) / 448.0).contiguous() for x in (k, v)]
                pools = [(pool.float() / s.view(1, kvh, 1, 1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for pool, s in zip(pools, sc)]
            cache[pkey] = (pools[0], pools[1], perm.view(B, mp).to(torch.int32).contiguous(), sc[0], sc[1])
        k_pool, v_pool, table, k_scale, v_scale = cache[pkey]
    if "append" in opts and "rope" in opts:
        raise SystemExit(f"{spec}: append and rope are two arms, not one spec")
    if "append" in opts:
        if not page or L < nq or causal or "sdpa" in opts:
            raise SystemExit(f"{spec}: append needs page=P and len >= q, and takes neither causal nor sdpa")
        return run_append(spec, (B, kvh, nq, N, D, L, page), "torch" in opts, kv8, cache[pkey], lens)
    if "rope" in opts:
        if not page or L < nq or causal or "sdpa" in opts:
            raise SystemExit(f"{spec}: rope needs page=P and len >= q, and takes neither causal nor sdpa")
        return run_rope(spec, (B, H, kvh, nq, N, D, L, page), "torch" in opts, kv8, cache[pkey], lens)
    capi.tune("attn_decode_split", split)
    try:
        if "sdpa" in opts:
            if causal and not chunk:
                raise SystemExit(f"{spec}: the sdpa arm of a decode spec is non-causal")
            ks, vs = k[:, :, :L], v[:, :, :L]
            mask = None                                 # a chunk spec: query i sees keys j <= L - Nq + i (torch's is_causal is top-left aligned)
            if causal:
                mask = torch.arange(L, device="cuda").view(1, L) <= (L - nq + torch.arange(nq, device="cuda")).view(nq, 1)
            try:
                torch.nn.functional.scaled_dot_product_attention(q, ks, vs, attn_mask=mask, enable_gqa=True)
                name = "torch sdpa enable_gqa" + (" + mask" if causal else "")
                step = lambda: torch.nn.functional.scaled_dot_product_attention(q, ks, vs, attn_mask=mask, enable_gqa=True)  # noqa: E731
            except TypeError:
                ke, ve = ks.repeat_interleave(H // kvh, dim=1), vs.repeat_interleave(H // kvh, dim=1)
                name = "torch sdpa (K / V expanded)" + (" + mask" if causal else "")
                step = lambda: torch.nn.functional.scaled_dot_product_attention(q, ke, ve, attn_mask=mask)  # noqa: E731
        else:                                           # the cache kind of the spec -> (name function, its shape arguments, step)
            paged = (B, H, kvh, nq, page, N // max(page, 1), D)
            fam = "attn_chunk" if chunk else "attn_decode"      # more than 64 query rows per K / V head: the chunk entries
            call = lambda suffix: getattr(capi, fam + suffix)  # noqa: E731
            name_of, shape_args, step = {
                "kv8": (call("_paged_kv8_kernel_name"), paged, lambda: call("_paged_kv8")(q, k_pool, v_pool, o, table, lens, k_scale, v_scale, causal=causal)),
                "paged": (call("_paged_kernel_name"), paged, lambda: call("_paged")(q, k_pool, v_pool, o, table, lens, causal=causal)),
                "flat": (call("_kernel_name"), (B, H, kvh, nq, N, D), lambda: call("")(q, k, v, o, lens, causal=causal)),
            }["kv8" if kv8 else "paged" if page else "flat"]
            name = name_of(*shape_args, causal=causal)
        ms = timed(step)
    finally:
        capi.tune("attn_decode_split", 0)
    return name, 2.0 * B * kvh * L * D * (1 if kv8 else 2) / ms * 1e-6, ms


def run(spec):
    shape, *opts = spec.split(":")
    B, H, N, D = (int(x) for x in shape.split(","))
    if any(o.startswith("q=") for o in opts):
        return run_decode(spec, (B, H, N, D), opts)
    bf16, zero, vt, causal, sdpa = "bf16" in opts, "zero" in opts, "vt" in opts, "causal" in opts, "sdpa" in opts
    kvh = next((int(o.split("=")[1]) for o in opts if o.startswith("kvh=")), 0)
    expand = "expand" in opts
    if kvh and (bf16 or sdpa or H % kvh != 0):
        raise SystemExit(f"{spec}: kvh needs fp16, this library and H % kvh == 0")
    knobs = {KNOBS[o.split("=")[0]]: int(o.split("=")[1]) for o in opts if "=" in o and not o.startswith("kvh=")}
    q, k, v, o = tensors(B, H, N, D, bf16, zero, kvh)
    if vt:
        v = v.transpose(-2, -1).contiguous()
    for kk, vv in knobs.items():
        capi.tune(kk, vv)
    try:
        if sdpa:
            name = "torch sdpa" + (" is_causal" if causal else "")
            vv = v.transpose(-2, -1) if vt else v
            step = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, vv, is_causal=causal)  # noqa: E731
        elif kvh and expand:
            g = H // kvh
            name = "expand + " + capi.attn_kernel_name(N, D, vt, bh=B * H, causal=causal)
            step = lambda: capi.attn_fwd(q, k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1), o, v_transposed=vt, causal=causal)  # noqa: E731
        elif kvh and "expanded" in opts:
            ke, ve = k.repeat_interleave(H // kvh, dim=1).contiguous(), v.repeat_interleave(H // kvh, dim=1).contiguous()
            name = capi.attn_kernel_name(N, D, vt, bh=B * H, causal=causal)
            step = lambda: capi.attn_fwd(q, ke, ve, o, v_transposed=vt, causal=causal)  # noqa: E731
        elif kvh:
            name = capi.attn_kernel_name(N, D, vt, bh=B * H, causal=causal, group=H // kvh)
            step = lambda: capi.attn_fwd_gqa(q, k, v, o, v_transposed=vt, causal=causal)  # noqa: E731
        else:
            name = capi.attn_kernel_name(N, D, vt, bf16, bh=B * H, causal=causal)
            step = (lambda: capi.attn_fwd_bf16(q, k, v, o)) if bf16 else (lambda: capi.attn_fwd(q, k, v, o, v_transposed=vt, causal=causal))
        ms = timed(step)
    finally:
        for kk in knobs:
            capi.tune(kk, capi.tune_items()[kk][1])      # back to the library default
    return name, host.mha_matmul_flops(B, H, N, D) * (0.5 if causal else 1.0) / ms * 1e-9, ms


res = {s: [] for s in args}
times = {s: [] for s in args}
names = {}
for r in range(rounds):
    for s in args:
        names[s], tf, ms = run(s)
        res[s].append(tf)
        times[s].append(ms)
if any("causal" in s.split(":") for s in args):
    print("(causal TFLOP/s count half of 4 B H N^2 D: the flash-attn convention)", flush=True)
for s in args:
    v, t = sorted(res[s]), sorted(times[s])
    if any(o.startswith("q=") for o in s.split(":")):     # decode: res holds K / V GB/s
        print(f"RATE {s:40s} {names[s]:38s} median {t[len(t) // 2] * 1e3:8.1f} us  best {t[0] * 1e3:8.1f}  worst {t[-1] * 1e3:8.1f}  "
              f"{'R+W' if {'append', 'rope'} & set(s.split(':')) else 'K/V'} {v[len(v) // 2]:7.0f} GB/s", flush=True)
        continue
    print(f"RATE {s:34s} {names[s]:44s} median {v[len(v) // 2]:7.1f}  best {v[-1]:7.1f}  worst {v[0]:7.1f} TFLOP/s  {t[len(t) // 2] * 1e3:9.1f} us", flush=True)
