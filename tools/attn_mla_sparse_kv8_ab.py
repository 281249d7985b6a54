"""Time the sparse latent attention over an fp8 latent pool (capi.attn_mla_sparse_kv8) against the path a caller is
forced onto without it and against the dense fp8 entry, in one process and in alternating rounds:

    python tools/attn_mla_sparse_kv8_ab.py [--rounds 5] [--secs 0.4] > profiles/attn_mla_sparse_kv8_ab.log

Shapes (topk = 2048, every token's slots drawn without replacement from a pool of 65536 slots): H 16 and 128, a decode step (T = 64 tokens)
and a prefill chunk (T = 1024) — the shapes of tools/attn_mla_sparse_ab.py —, fp16, and the two H = 128 shapes in bfloat16.  Per shape three
variants:
  sparse kv8   capi.attn_mla_sparse_kv8 on the code pool, the 16-bit rope pool and the slots
  sparse 16    the unchanged capi.attn_mla_sparse on a 16-bit pool of the DEQUANTISED values with the same slots: what a caller without the
               new entry runs, the cost of dequantising the pool not counted
  dense kv8    capi.attn_mla_paged_kv8 over 2048 CONTIGUOUS keys, one sequence per token, each with a cache region of its own (page 64): the
               same arithmetic without the gather
Each line: the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls after a warm-up), the
bytes the variant's job needs — every selected pool row and slot once per token, Q and O once — over the median, and the ratio of its median to
the new entry's.  The rounds alternate the variants, each round starting with another one; the distance between a variant's best and worst
round is the run-to-run spread a difference has to beat.  The first line of a shape also states the largest |O - O16| of the two sparse
variants, which run the same slots on the same values.  No pass mark.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402
from tools.attn_varlen_ab import i32, timed  # noqa: E402

TOPK, NSLOTS, PS, SCALE, CKV_SCALE = 2048, 65536, 64, 576 ** -0.5, 2.0 ** -5


def row(label, T, H, el, rounds, secs):
    dev = "cuda"
    q_c, q_pe = torch.randn(T, H, 512, device=dev).to(el), torch.randn(T, H, 64, device=dev).to(el)
    codes = (torch.randn(NSLOTS, 512, device=dev) / CKV_SCALE).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    ckv16, kpe = (codes.float() * CKV_SCALE).to(el), torch.randn(NSLOTS, 64, device=dev).to(el)
    codes, scale = codes.view(torch.uint8), torch.tensor([CKV_SCALE], dtype=torch.float32, device=dev)
    slots = torch.stack([torch.randperm(NSLOTS, device=dev)[:TOPK] for _ in range(T)]).to(torch.int32).contiguous()
    o, o16 = torch.empty_like(q_c), torch.empty_like(q_c)
    # the dense call's cache: token t owns pages t * 32 .. t * 32 + 31
    mp = TOPK // PS
    codes_seq = codes[torch.randint(NSLOTS, (T * mp * PS,), device=dev)].view(T * mp, PS, 512).contiguous()
    kpe_seq = torch.randn(T * mp, PS, 64, device=dev).to(el)
    table = torch.arange(T * mp, device=dev, dtype=torch.int32).view(T, mp).contiguous()
    cu, lens = i32(range(T + 1)), i32([TOPK] * T)

    def sparse_kv8():
        capi.attn_mla_sparse_kv8(q_c, q_pe, codes, kpe, o, slots, SCALE, ckv_scale=scale)

    def sparse_16():
        capi.attn_mla_sparse(q_c, q_pe, ckv16, kpe, o16, slots, SCALE)

    def dense_kv8():
        capi.attn_mla_paged_kv8(q_c, q_pe, codes_seq, kpe_seq, o16, cu, table, lens, 1, SCALE, ckv_scale=scale)

    sparse_kv8(), sparse_16()
    torch.cuda.synchronize()
    diff = float((o.float() - o16.float()).abs().max())
    variants = {"sparse kv8": sparse_kv8, "sparse 16": sparse_16, "dense kv8": dense_kv8}
    key_bytes = {"sparse kv8": 512 + 128 + 4, "sparse 16": 1024 + 128 + 4, "dense kv8": 512 + 128}
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(rounds):
        for k in order[r % 3:] + order[:r % 3]:
            times[k].append(timed(variants[k], secs))
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    bf = el == torch.bfloat16
    print(f"AB {label} T{T} H{H} {'bf16' if bf else 'f16'}: {capi.attn_mla_sparse_kv8_kernel_name(T, H, TOPK, bf16=bf)} | "
          f"{capi.attn_mla_sparse_kernel_name(T, H, TOPK, bf16=bf)} | {capi.attn_mla_paged_kv8_kernel_name(T, H, T, 1, PS, mp, bf16=bf)} | "
          f"max |O - O16| {diff:.3e}", flush=True)
    for k, t in times.items():
        nbytes = T * (TOPK * key_bytes[k] + H * (576 + 512) * 2)
        print(f"AB   {k:11s} median {med[k] * 1e3:9.1f} us  best {min(t) * 1e3:9.1f}  worst {max(t) * 1e3:9.1f}  {nbytes / med[k] * 1e-9:7.3f} TB/s"
              f"  x{med[k] / med['sparse kv8']:6.2f} of sparse kv8", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.4)
    a = ap.parse_args()
    capi.load()
    capi.require_production()
    torch.manual_seed(0)
    for label, T in (("decode", 64), ("prefill chunk", 1024)):
        for H in (16, 128):
            row(label, T, H, torch.half, a.rounds, a.secs)
    for label, T in (("decode", 64), ("prefill chunk", 1024)):
        row(label, T, 128, torch.bfloat16, a.rounds, a.secs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
