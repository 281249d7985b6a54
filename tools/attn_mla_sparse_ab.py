"""Time the sparse latent attention (capi.attn_mla_sparse) against the dense entry, in one process and in alternating
rounds:

    python tools/attn_mla_sparse_ab.py [--rounds 3] [--secs 0.4] > profiles/attn_mla_sparse_ab.log

Shapes (fp16, topk = 2048): H 16 and 128, a decode step (T = 64 tokens) and a prefill chunk (T = 1024).  Every token's slots are drawn without
replacement from a pool of 65536 slots.  Per shape three variants:
  sparse      capi.attn_mla_sparse on the pool and the slots
  dense       capi.attn_mla_paged over 2048 CONTIGUOUS keys, one sequence per token, each with a cache region of its own (page 64): the same
              arithmetic without the gather — the ceiling
  gather+dense   torch index_select of the 2048 latent and rope rows of every token into that scratch cache, then `dense`: what a caller does
              without the sparse entry (the int64 copy of the slots is made beforehand and not timed)
Each line: the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls after a warm-up) and
the bytes the sparse job needs — every selected pool row and slot once per token, Q and O once — over the median; for the other two the ratio of
their median to the sparse call's.  The rounds alternate the variants, each round starting with another one.  No pass mark.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402
from tools.attn_varlen_ab import i32, timed  # noqa: E402

TOPK, NSLOTS, PS, SCALE = 2048, 65536, 64, 576 ** -0.5


def row(label, T, H, rounds, secs):
    dev = "cuda"
    q_c, q_pe = torch.randn(T, H, 512, device=dev).half(), torch.randn(T, H, 64, device=dev).half()
    ckv, kpe = torch.randn(NSLOTS, 512, device=dev).half(), torch.randn(NSLOTS, 64, device=dev).half()
    slots = torch.stack([torch.randperm(NSLOTS, device=dev)[:TOPK] for _ in range(T)]).to(torch.int32).contiguous()
    flat = slots.view(-1).long()
    o = torch.empty_like(q_c)
    # the dense call's cache: token t owns pages t * 32 .. t * 32 + 31
    mp = TOPK // PS
    ckv_seq, kpe_seq = torch.randn(T * mp, PS, 512, device=dev).half(), torch.randn(T * mp, PS, 64, device=dev).half()
    table = torch.arange(T * mp, device=dev, dtype=torch.int32).view(T, mp).contiguous()
    cu, lens = i32(range(T + 1)), i32([TOPK] * T)

    def sparse():
        capi.attn_mla_sparse(q_c, q_pe, ckv, kpe, o, slots, SCALE)

    def dense():
        capi.attn_mla_paged(q_c, q_pe, ckv_seq, kpe_seq, o, cu, table, lens, 1, SCALE)

    def gather_dense():
        torch.index_select(ckv, 0, flat, out=ckv_seq.view(-1, 512))
        torch.index_select(kpe, 0, flat, out=kpe_seq.view(-1, 64))
        dense()

    variants = {"sparse": sparse, "dense": dense, "gather+dense": gather_dense}
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(rounds):
        for k in order[r % 3:] + order[:r % 3]:
            times[k].append(timed(variants[k], secs))
    nbytes = T * (TOPK * (576 * 2 + 4) + H * (576 + 512) * 2)
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    print(f"AB {label} T{T} H{H}: {capi.attn_mla_sparse_kernel_name(T, H, TOPK)} | {capi.attn_mla_paged_kernel_name(T, H, T, 1, PS, mp)}", flush=True)
    for k, t in times.items():
        print(f"AB   {k:13s} median {med[k] * 1e3:9.1f} us  best {min(t) * 1e3:9.1f}  worst {max(t) * 1e3:9.1f}  {nbytes / med[k] * 1e-9:7.3f} TB/s"
              f"  x{med[k] / med['sparse']:6.2f} of sparse", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--secs", type=float, default=0.4)
    a = ap.parse_args()
    capi.load()
    capi.require_production()
    torch.manual_seed(0)
    for label, T in (("decode", 64), ("prefill chunk", 1024)):
        for H in (16, 128):
            row(label, T, H, a.rounds, a.secs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
