"""Time the fp8 index logits (capi.mla_index_logits_fp8) against the 16-bit entry (capi.mla_index_logits, section 4.3u)
on the dequantised pool and queries, and the quantising append, in one process and in alternating rounds:

    python tools/mla_index_fp8_ab.py [--rounds 5] [--secs 0.4] > profiles/mla_index_fp8_ab.log

The shapes of tools/mla_index_ab.py (page 64, causal): a decode step B = 64, Nq = 1 at L = 32 768 and 65 536, and a prefill chunk of T = 1024
tokens of one sequence behind L = 32 768.  randn keys and queries are quantised per row at amax / 448 (power-of-two scales); `fp16`: the parent's
entry on the fp16 pool and queries holding code x scale — what a caller ran before, dequantising not counted.  Each line: the median, best and
worst of the rounds' times (device events around >= --secs seconds of back-to-back calls after a warm-up), the bytes of the key pool the step
needs (every key of every sequence once: 128 + 4 bytes a key for fp8, 256 for fp16) over the median, and the products' FLOP (2 x 64 x 128 per
visible (token, key)) over the median.  The rounds alternate the variants, each round starting with another one.  Then the append
(capi.mla_index_append_fp8, fp16 sources, pow2) at T = 64 and T = 1024, one token a sequence.  No pass mark.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402
from tools.attn_varlen_ab import i32, timed  # noqa: E402

PS, HI, DI, F8 = 64, 64, 128, torch.float8_e4m3fn


def quantise(x):   # (codes uint8, power-of-two scales) per row of the last dim
    s = torch.exp2(torch.ceil(torch.log2(x.abs().amax(-1).clamp_min(1e-4) / 448)))
    return (x / s[..., None]).to(F8).view(torch.uint8), s


def medians(variants, rounds, secs):
    times, order = {k: [] for k in variants}, list(variants)
    for r in range(rounds):
        k0 = r % len(order)
        for k in order[k0:] + order[:k0]:
            times[k].append(timed(variants[k], secs))
    return times, {k: sorted(t)[len(t) // 2] * 1e-3 for k, t in times.items()}   # ms per round, median seconds


def row(label, B, nq, L, rounds, secs):
    dev = "cuda"
    T, mp = B * nq, L // PS
    q8, sq = quantise(torch.randn(T, HI, DI, device=dev))
    k8, ks = quantise(torch.randn(B * mp, PS, DI, device=dev))
    w8 = torch.randn(T, HI, device=dev) * HI ** -0.5
    q16, w16 = q8.view(F8).half(), w8.clone()                                          # (codes are exact in fp16; the query scale stays in w)
    w8 = w8 * sq
    w16 = w16 * sq
    k16 = (k8.view(F8).float() * ks[..., None]).half()
    table = torch.arange(B * mp, device=dev, dtype=torch.int32).view(B, mp).contiguous()
    cu, lens = i32(range(0, T + 1, nq)), i32([L] * B)
    lg8, lg16 = torch.empty(T, L, device=dev), torch.empty(T, L, device=dev)
    seen = (L - nq + 1 + torch.arange(nq, device=dev)).repeat(B)                       # n_t
    variants = {"fp8": lambda: capi.mla_index_logits_fp8(q8, w8, k8, ks, lg8, cu, table, lens, nq),
                "fp16": lambda: capi.mla_index_logits(q16, w16, k16, lg16, cu, table, lens, nq)}
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    vis = torch.arange(L, device=dev)[None, :] < seen[:, None]
    diff = ((lg8 - lg16).abs() * vis).amax(1).div((lg16.abs() * vis).amax(1)).max().item()   # against the row's largest logit
    times, med = medians(variants, rounds, secs)
    print(f"AB {label} B{B} Nq{nq} L{L}: {capi.mla_index_logits_fp8_kernel_name(B, T, nq, B * mp, PS, mp)} | "
          f"{capi.mla_index_logits_kernel_name(B, T, nq, B * mp, PS, mp)}; worst |fp8 - fp16| over the row's largest |logit| {diff:.2e}", flush=True)
    flop = 2.0 * HI * DI * seen.sum().item()
    for k, t in times.items():
        keyb = B * L * (DI + 4 if k == "fp8" else 2 * DI)
        print(f"AB   {k:5s} median {med[k] * 1e6:9.1f} us  best {min(t) * 1e3:9.1f}  worst {max(t) * 1e3:9.1f}  {keyb / med[k] * 1e-12:6.3f} TB/s of key pool  "
              f"{flop / med[k] * 1e-12:7.1f} TFLOP/s", flush=True)
    print(f"AB   fp16 / fp8 = {med['fp16'] / med['fp8']:5.2f}", flush=True)


def append_row(T, rounds, secs):
    dev, L = "cuda", 4096
    mp = L // PS
    new = torch.randn(T, DI, device=dev).half()
    pool, scale = torch.zeros(T * mp, PS, DI, dtype=torch.uint8, device=dev), torch.zeros(T * mp, PS, device=dev)
    table = torch.arange(T * mp, device=dev, dtype=torch.int32).view(T, mp).contiguous()
    cu, lens = i32(range(T + 1)), i32([L] * T)
    times, med = medians({"append": lambda: capi.mla_index_append_fp8(new, pool, scale, cu, table, lens, 1)}, rounds, secs)
    t = times["append"]
    print(f"AB append T{T}: {capi.mla_index_append_fp8_kernel_name(T, T, 1, T * mp, PS, mp)} median {med['append'] * 1e6:7.2f} us  "
          f"best {min(t) * 1e3:7.2f}  worst {max(t) * 1e3:7.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.4)
    a = ap.parse_args()
    capi.load()
    capi.require_production()
    torch.manual_seed(0)
    row("decode", 64, 1, 32768, a.rounds, a.secs)
    row("decode", 64, 1, 65536, a.rounds, a.secs)
    row("prefill chunk", 1, 1024, 32768, a.rounds, a.secs)
    append_row(64, a.rounds, a.secs)
    append_row(1024, a.rounds, a.secs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
