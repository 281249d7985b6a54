"""Time multi-head latent attention (attn_mla_paged) in one process and in alternating rounds:

    python tools/attn_mla_ab.py [--rounds 3] [--secs 0.3] [--bf16]

B = 64 decoding sequences over a paged latent cache with pages of 64 keys.  For H in {128, 16} and L in {4096, 32768}, one row each:
    mla Nq=1 / Nq=2, S auto / S=1   the MLA call (every sequence Nq new tokens)
    torch Nq=1                      the same computation in torch ops on the gathered cache: softmax(q kv^T scale) kv[:, :512]
and per L one yardstick row: lc_attn_varlen_paged_f16 at H = 16, Hkv = 1, D = 128, Nq = 1 over a cache of 2.25 L keys — the same number of
cache bytes (1152 a key here, 512 there).  Each line: the median, best and worst of the rounds' times (device events around >= --secs
seconds of back-to-back calls, after a warm-up), the kernel name, and the cache bytes per second of the median: B L 1152 bytes, the bytes the
algorithm needs once (the row blocks of H = 128 re-read them through the L2).  The rounds alternate the variants of a row.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402

B, PS, DC, DR = 64, 64, 512, 64


def timed(step, secs):
    """ms per call of `step` over >= secs seconds of back-to-back calls"""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        step()
    e1.record()
    torch.cuda.synchronize()
    n = max(3, int(secs / (e0.elapsed_time(e1) / 3 * 1e-3)))
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run_row(row, variants, nbytes, rounds, secs):
    """variants: {label: (step, kernel name)}"""
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            times[k].append(timed(variants[k][0], secs))
    for k, (_, name) in variants.items():
        t = sorted(times[k])
        med = t[len(t) // 2]
        print(f"AB {row:14s} {k:16s} {name:58s} median {med * 1e3:9.1f} us  best {t[0] * 1e3:9.1f}  worst {t[-1] * 1e3:9.1f}  "
              f"{nbytes / (med * 1e-3) / 1e12:6.3f} TB/s of cache", flush=True)


def forced(split, step):
    def f():
        capi.tune("attn_decode_split", split)
        try:
            step()
        finally:
            capi.tune("attn_decode_split", 0)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--secs", type=float, default=0.3)
    ap.add_argument("--bf16", action="store_true")
    a = ap.parse_args()
    el = torch.bfloat16 if a.bf16 else torch.half
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for L in (4096, 32768):
        pages = L // PS
        ckv = torch.randn(B * pages, PS, DC, generator=g, device=dev, dtype=torch.float32).to(el)
        kpe = torch.randn(B * pages, PS, DR, generator=g, device=dev, dtype=torch.float32).to(el)
        table = torch.randperm(B * pages, generator=g, device=dev).to(torch.int32).view(B, pages).contiguous()
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        nbytes = B * L * (DC + DR) * 2
        for H in (128, 16):
            scale = 1.0 / (DC + DR) ** 0.5
            variants = {}
            for nq in (1, 2):
                T = B * nq
                q_c = torch.randn(T, H, DC, generator=g, device=dev).to(el)
                q_pe = torch.randn(T, H, DR, generator=g, device=dev).to(el)
                o = torch.empty_like(q_c)
                cu = torch.arange(0, T + 1, nq, dtype=torch.int32, device=dev)

                def step(q_c=q_c, q_pe=q_pe, o=o, cu=cu, nq=nq):
                    capi.attn_mla_paged(q_c, q_pe, ckv, kpe, o, cu, table, lens, nq, scale, causal=True)

                variants[f"mla Nq={nq} auto"] = (step, capi.attn_mla_paged_kernel_name(B, H, T, nq, PS, pages, causal=True, bf16=a.bf16))
                variants[f"mla Nq={nq} S=1"] = (forced(1, step), "attn_mla_paged_kernel")
                if nq == 1:
                    kv = torch.cat([ckv[table.long()].view(B, L, DC), kpe[table.long()].view(B, L, DR)], -1)      # gathered once, outside the timing
                    q = torch.cat([q_c, q_pe], -1)

                    def ref(q=q, kv=kv):
                        p = torch.softmax(torch.bmm(q, kv.transpose(1, 2)).float() * scale, -1).to(el)
                        return torch.bmm(p, kv[:, :, :DC])

                    variants["torch Nq=1"] = (ref, "bmm, softmax, bmm on the gathered cache")
            run_row(f"H={H} L={L}", variants, nbytes, a.rounds, a.secs)
            del variants
        del ckv, kpe
        # the byte-rate yardstick: the ragged paged call at Hkv = 1, D = 128 over the same number of cache bytes
        L2 = L * (DC + DR) // (2 * 128)
        p2 = L2 // PS
        kp = torch.randn(B * p2, 1, PS, 128, generator=g, device=dev).half()
        vp = torch.randn(B * p2, 1, PS, 128, generator=g, device=dev).half()
        t2 = torch.randperm(B * p2, generator=g, device=dev).to(torch.int32).view(B, p2).contiguous()
        l2 = torch.full((B,), L2, dtype=torch.int32, device=dev)
        q = torch.randn(B, 16, 128, generator=g, device=dev).half()
        o = torch.empty_like(q)
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev)
        run_row(f"yardstick L={L}", {"varlen D=128": (lambda: capi.attn_varlen_paged(q, kp, vp, o, cu, t2, l2, 1, causal=True),
                                                     capi.attn_varlen_paged_kernel_name(B, 16, 1, B, 1, PS, p2, 128, causal=True))},
                nbytes, a.rounds, a.secs)
        del kp, vp


if __name__ == "__main__":
    main()
