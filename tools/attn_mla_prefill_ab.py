"""Time the non-absorbed MLA prefill attention (capi.attn_mla_prefill) against what a caller has without it, in one
process and in alternating rounds:

    python tools/attn_mla_prefill_ab.py [--rounds 5] [--secs 0.3] > profiles/attn_mla_prefill_ab.log

Shapes (fp16, H = 128, causal): B x N prompts of 2048 (B = 4) and 8192 (B = 1) tokens, operands as the projections leave them (q [T,128,192]
dense, k_nope / v the halves of one [T,128,256] buffer, k_pe [T,64]); and one 2048-token chunk behind 8192 context keys: the chunk over the
context (no mask) and over its own keys (causal), merged by capi.attn_merge_states.  Per prompt shape:
  prefill     capi.attn_mla_prefill
  sdpa        torch scaled_dot_product_attention (causal) on [B,H,N,192] / [B,H,N,128] tensors that already exist
  copies      what sdpa needs first: cat(k_nope, k_pe.expand) and the three transposes to [B,H,N,D], made contiguous — timed on its own
  fwd d128    this library's tuned lc_attn_fwd_f16_ex, causal, D = 128 on the same (B H, N): a DIFFERENT problem (0.8 x the FLOPs a key: no
              rope dims), shown only to place the new kernel against the tuned one
Each line: the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls after a warm-up) and
TFLOP/s counting 2 (192 + 128) FLOPs a visible (query, key) pair — for `fwd d128` too, which therefore reads high by 1.25 x against its own
work.  The rounds alternate the variants, each round starting with another one.  No pass mark.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402
from tools.attn_varlen_ab import i32, timed  # noqa: E402

H, SCALE = 128, 192 ** -0.5


def report(label, names, variants, pairs, rounds, secs, base):
    times, order = {k: [] for k in variants}, list(variants)
    for r in range(rounds):
        s = r % len(order)
        for k in order[s:] + order[:s]:
            times[k].append(timed(variants[k], secs))
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    print(f"AB {label}: {names}", flush=True)
    for k, t in times.items():
        print(f"AB   {k:9s} median {med[k] * 1e3:9.1f} us  best {min(t) * 1e3:9.1f}  worst {max(t) * 1e3:9.1f}  "
              f"{2 * 320 * pairs / med[k] * 1e-9:7.1f} TFLOP/s  x{med[k] / med[base]:6.2f} of {base}", flush=True)


def operands(Tq, Tk):
    q, kv = torch.randn(Tq, H, 192, device="cuda").half(), torch.randn(Tk, H, 256, device="cuda").half()
    return q, kv[:, :, :128], torch.randn(Tk, 64, device="cuda").half(), kv[:, :, 128:], torch.empty(Tq, H, 128, device="cuda", dtype=torch.half)


def prompts(B, N, rounds, secs):
    T = B * N
    q, kn, kpe, v, o = operands(T, T)
    cu = i32(range(0, T + 1, N))
    q4 = q.view(B, N, H, 192).transpose(1, 2).contiguous()
    k4, v4 = torch.empty_like(q4), torch.empty(B, H, N, 128, device="cuda", dtype=torch.half)
    qd, kd, od = (torch.randn(B, H, N, 128, device="cuda").half() for _ in range(3))

    def copies():
        q4.copy_(q.view(B, N, H, 192).transpose(1, 2))
        k4.copy_(torch.cat([kn, kpe[:, None, :].expand(-1, H, -1)], -1).view(B, N, H, 192).transpose(1, 2))
        v4.copy_(v.reshape(B, N, H, 128).transpose(1, 2))

    variants = {"prefill": lambda: capi.attn_mla_prefill(q, kn, kpe, v, o, cu, cu, N, SCALE),
                "sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, is_causal=True, scale=SCALE),
                "copies": copies, "fwd d128": lambda: capi.attn_fwd(qd, kd, kd, od, causal=True)}
    copies()
    names = f"{capi.attn_mla_prefill_kernel_name(B, H, T, N)} | {capi.attn_kernel_name(N, 128, bh=B * H, causal=True)}"
    report(f"prompts B{B} N{N} H{H}", names, variants, B * H * N * (N + 1) // 2, rounds, secs, "prefill")


def chunk(Nq, Nctx, rounds, secs):
    q, kn, kpe, v, o = operands(Nq, Nctx + Nq)
    o2, la, lb = torch.empty_like(o), torch.empty(Nq, H, device="cuda"), torch.empty(Nq, H, device="cuda")
    cu_q, ctx, own, both = i32([0, Nq]), i32([0, Nctx]), i32([Nctx, Nctx + Nq]), i32([0, Nctx + Nq])

    def chunked():
        capi.attn_mla_prefill(q, kn, kpe, v, o, cu_q, ctx, Nq, SCALE, lse=la, causal=False)
        capi.attn_mla_prefill(q, kn, kpe, v, o2, cu_q, own, Nq, SCALE, lse=lb, causal=True)
        capi.attn_merge_states(o, la, o2, lb, out=o, lse_out=la)

    variants = {"chunk": chunked, "one call": lambda: capi.attn_mla_prefill(q, kn, kpe, v, o, cu_q, both, Nq, SCALE)}
    report(f"chunk Nq{Nq} behind {Nctx} H{H}", "two calls + attn_merge_states | one causal call over all keys", variants,
           H * (Nq * Nctx + Nq * (Nq + 1) // 2), rounds, secs, "chunk")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.3)
    a = ap.parse_args()
    capi.load()
    capi.require_production()
    torch.manual_seed(0)
    prompts(4, 2048, a.rounds, a.secs)
    prompts(1, 8192, a.rounds, a.secs)
    chunk(2048, 8192, a.rounds, a.secs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
