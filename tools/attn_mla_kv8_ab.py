"""Time MLA decode over an fp8 latent cache (attn_mla_paged_kv8) beside the 16-bit entry, in one process and in
alternating rounds:

    python tools/attn_mla_kv8_ab.py [--rounds 3] [--secs 0.3] [--bf16]

The shapes of tools/attn_mla_ab.py's table: B = 64 decoding sequences (Nq = 1, causal), pages of 64 keys, H in {128, 16}, L in {4096, 32768};
per shape four variants, alternated over the rounds: the 16-bit and the fp8 call, each with the automatic split and under S = 1.  The fp8 pool
holds the 16-bit pool's values quantised under a scale of 1 / 64 (randn stays inside +-448), so both calls compute the same attention; their
outputs are compared once per shape before anything is timed (largest |difference| printed: the quantisation error, not a tolerance test).
Each line: median, best and worst of the rounds (device events around >= --secs seconds of back-to-back calls, after a warm-up), the kernel
name, TB/s of the cache bytes the call needs once (B L 1152 for the 16-bit pools, B L 640 for fp8 codes + 16-bit rope keys), and for the fp8
lines the ratio of its median to the 16-bit call's of the same split (the byte ratio 640 / 1152 = 0.56 is the floor), with the S = 1 time per
64-key tile.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from attn_mla_ab import B, DC, DR, PS, forced, timed  # noqa: E402  (puts the repository root on sys.path)
from leetcuda_amd import capi  # noqa: E402

SCALE = 1.0 / 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--secs", type=float, default=0.3)
    ap.add_argument("--bf16", action="store_true")
    a = ap.parse_args()
    el = torch.bfloat16 if a.bf16 else torch.half
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    sm = 1.0 / (DC + DR) ** 0.5
    scale = torch.tensor([SCALE], dtype=torch.float32, device=dev)
    for L in (4096, 32768):
        pages = L // PS
        ckv = torch.randn(B * pages, PS, DC, generator=g, device=dev, dtype=torch.float32).to(el)
        kpe = torch.randn(B * pages, PS, DR, generator=g, device=dev, dtype=torch.float32).to(el)
        codes = (ckv.float() / SCALE).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        table = torch.randperm(B * pages, generator=g, device=dev).to(torch.int32).view(B, pages).contiguous()
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev)
        for H in (128, 16):
            q_c = torch.randn(B, H, DC, generator=g, device=dev).to(el)
            q_pe = torch.randn(B, H, DR, generator=g, device=dev).to(el)
            o16, o8 = torch.empty_like(q_c), torch.empty_like(q_c)

            def f16():
                capi.attn_mla_paged(q_c, q_pe, ckv, kpe, o16, cu, table, lens, 1, sm, causal=True)

            def f8():
                capi.attn_mla_paged_kv8(q_c, q_pe, codes, kpe, o8, cu, table, lens, 1, sm, ckv_scale=scale, causal=True)

            f16(), f8()
            torch.cuda.synchronize()
            print(f"AB H={H} L={L}: max |O fp8 - O 16-bit| {float((o8.float() - o16.float()).abs().max()):.3e} "
                  f"(max |O 16-bit| {float(o16.float().abs().max()):.3e})", flush=True)
            names = (capi.attn_mla_paged_kernel_name(B, H, B, 1, PS, pages, causal=True, bf16=a.bf16),
                     capi.attn_mla_paged_kv8_kernel_name(B, H, B, 1, PS, pages, causal=True, bf16=a.bf16))
            variants = {"16-bit auto": (f16, names[0], 1152), "fp8 auto": (f8, names[1], 640),
                        "16-bit S=1": (forced(1, f16), names[0].split(" + ")[0], 1152), "fp8 S=1": (forced(1, f8), names[1].split(" + ")[0], 640)}
            order, times = list(variants), {k: [] for k in variants}
            for r in range(a.rounds):
                for k in order[r % 4:] + order[:r % 4]:
                    times[k].append(timed(variants[k][0], a.secs))
            med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
            for k, (_, name, row_bytes) in variants.items():
                t = sorted(times[k])
                tail = ""
                if k.startswith("fp8"):
                    tail = f"  x{med[k] / med[k.replace('fp8', '16-bit')]:.3f} of 16-bit"
                if k.endswith("S=1"):
                    tail += f"  {med[k] * 1e3 / (L // 64):.2f} us a tile"
                print(f"AB H={H:<3d} L={L:<5d} {k:12s} {name:64s} median {med[k] * 1e3:9.1f} us  best {t[0] * 1e3:9.1f}  worst {t[-1] * 1e3:9.1f}  "
                      f"{B * L * row_bytes / (med[k] * 1e-3) / 1e12:6.3f} TB/s of cache{tail}", flush=True)
        del ckv, kpe, codes


if __name__ == "__main__":
    main()
