"""Time the lightning indexer (capi.mla_index_logits, capi.mla_index_topk) against the torch ops it replaces, in one
process and in alternating rounds:

    python tools/mla_index_ab.py [--rounds 3] [--secs 0.4] > profiles/mla_index_ab.log

Shapes (fp16, topk = 2048, page 64, causal): a decode step B = 64, Nq = 1 at L = 32 768 and 65 536, and a prefill chunk of T = 1024 tokens of one
sequence behind L = 32 768.  Per shape three variants, timed separately:
  logits      capi.mla_index_logits
  topk        capi.mla_index_topk on the logits the first left
  torch       what a caller does without them: einsum of Qi with the (contiguous: the table is the identity, no gather is charged) keys into
              [T, 64, L], relu, the weighted sum over heads, the causal mask, torch.topk, a sort of the positions, the translation to slots
Each line: the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls after a warm-up).
logits: the bytes of the index-key pool the step needs (every key of every sequence once) over the median, and the products' FLOP (2 x 64 x 128
per visible (token, key)) over the median.  topk: microseconds a row (the call's time over T; the rows run side by side) and the passes
over the row (three histogram passes and the compaction).  The rounds alternate the variants, each round starting with another one.  No pass
mark.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402
from tools.attn_varlen_ab import i32, timed  # noqa: E402

TOPK, PS, HI, DI = 2048, 64, 64, 128


def row(label, B, nq, L, rounds, secs):
    dev = "cuda"
    T, mp = B * nq, L // PS
    q, w = torch.randn(T, HI, DI, device=dev).half(), torch.randn(T, HI, device=dev) * HI ** -0.5
    pool = torch.randn(B * mp, PS, DI, device=dev).half()
    table = torch.arange(B * mp, device=dev, dtype=torch.int32).view(B, mp).contiguous()
    cu, lens = i32(range(0, T + 1, nq)), i32([L] * B)
    logits = torch.empty(T, L, device=dev)
    slots = torch.empty(T, TOPK, dtype=torch.int32, device=dev)
    keys = pool.view(B, L, DI)
    seen = (L - nq + 1 + torch.arange(nq, device=dev)).repeat(B)                       # n_t
    hidden = torch.arange(L, device=dev)[None, :] >= seen[:, None]
    base = (torch.arange(B, device=dev) * L).repeat_interleave(nq)[:, None]

    def run_logits():
        capi.mla_index_logits(q, w, pool, logits, cu, table, lens, nq)

    def run_topk():
        capi.mla_index_topk(logits, slots, cu, table, lens, nq, page_size=PS, num_pages=B * mp)

    def run_torch():
        s = torch.einsum("bihd,bld->bihl", q.view(B, nq, HI, DI), keys).view(T, HI, L)
        lg = (s.relu_().float() * w[:, :, None]).sum(1).masked_fill_(hidden, float("-inf"))
        pos = lg.topk(TOPK, dim=1).indices.sort(dim=1).values
        return (pos + base).to(torch.int32)                                            # (identity table: slot = b L + position)

    run_logits()
    run_topk()
    ref = run_torch()[:64]                                                             # (fp16 einsum against fp32 logits: the threshold's neighbours differ)
    same = (slots[:64, :, None] == ref[:, None, :]).any(-1).float().mean().item()
    variants = {"logits": run_logits, "topk": run_topk, "torch": run_torch}
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(rounds):
        for k in order[r % 3:] + order[:r % 3]:
            times[k].append(timed(variants[k], secs))
    med = {k: sorted(t)[len(t) // 2] * 1e-3 for k, t in times.items()}                # seconds
    print(f"AB {label} B{B} Nq{nq} L{L}: {capi.mla_index_logits_kernel_name(B, T, nq, B * mp, PS, mp)} | "
          f"{capi.mla_index_topk_kernel_name(B, T, nq, B * mp, PS, mp, TOPK)}; {same:.4f} of the first 64 rows' slots are in torch's selection", flush=True)
    extra = {"logits": f"{B * L * DI * 2 / med['logits'] * 1e-12:6.3f} TB/s of key pool  {2.0 * HI * DI * seen.sum().item() / med['logits'] * 1e-12:7.1f} TFLOP/s",
             "topk": f"{med['topk'] / T * 1e6:7.3f} us a row, 4 passes over the row", "torch": ""}
    for k, t in times.items():
        print(f"AB   {k:7s} median {med[k] * 1e6:9.1f} us  best {min(t) * 1e3:9.1f}  worst {max(t) * 1e3:9.1f}  {extra[k]}", flush=True)
    print(f"AB   torch / (logits + topk) = {med['torch'] / (med['logits'] + med['topk']):5.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--secs", type=float, default=0.4)
    a = ap.parse_args()
    capi.load()
    capi.require_production()
    torch.manual_seed(0)
    row("decode", 64, 1, 32768, a.rounds, a.secs)
    row("decode", 64, 1, 65536, a.rounds, a.secs)
    row("prefill chunk", 1, 1024, 32768, a.rounds, a.secs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
