"""Time the latent-cache append (capi.mla_append_paged / _kv8) against the same job in torch ops, in one process and in
alternating rounds:

    python tools/mla_append_ab.py [--rounds 3] [--secs 0.5]

Shapes, each for the 16-bit and the fp8 latent pool (fp16 elements, page 64, gamma given, NeoX pairs): a decode step (B 64, Nq 1, H 128) and a
prefill of 8 x 1024 tokens at H 128 and H 16.  The sources are what a model has: views into a [T,576] kv_a projection output and into a
[T,H,192] q_b projection output.  The torch composition is RMSNorm in fp32, the rotation, the quantisation (a true division, clamp, e4m3fn) and
`index_put_` into the pools, with the pool rows and table rows of the tokens worked out beforehand and not timed — it gets the ragged
bookkeeping for nothing.  In the same run, as the yardstick of a byte rate: lc_rope_append_varlen_f16 on the prefill's tokens at H 32 / Hkv 8 /
D 128.  Each line: the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls after a
warm-up) and the bytes the job needs — every source and Qpe_out element once, the pool rows once, gamma and the table rows not counted — over
the median.  The rounds alternate the variants, each round starting with another one.  PASS: the library call's worst round is faster than the
torch composition's best.  Needs an MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402
from tools.attn_varlen_ab import cu_of, i32, timed  # noqa: E402

PS, MAX_POS, EPS, SCALE = 64, 4096, 1e-6, 0.0123


def run_row(row, variants, nbytes, rounds, secs):
    """variants: {label: step}, the first one the library call; returns whether it beat the others by more than the spread of the rounds"""
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            times[k].append(timed(variants[k], secs))
    ok = True
    for k, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        verdict = ""
        if k != order[0]:
            ok = ok and max(times[order[0]]) < t[0]
            verdict = f"  x{med / sorted(times[order[0]])[len(t) // 2]:7.2f} of {order[0]}  {'PASS' if max(times[order[0]]) < t[0] else 'FAIL'}"
        print(f"AB {row:24s} {k:12s} median {med * 1e3:9.1f} us  best {t[0] * 1e3:9.1f}  worst {t[-1] * 1e3:9.1f}  {nbytes / med * 1e-9:7.3f} TB/s{verdict}", flush=True)
    return ok


def mla_row(label, B, nq, H, kv8, rounds, secs):
    T, L = B * nq, 2048
    mp = L // PS
    kv, q = torch.randn(T, 576, device="cuda").half(), torch.randn(T, H, 192, device="cuda").half()
    ckv_new, kpe_new, q_pe = kv[:, :512], kv[:, 512:], q[:, :, 128:]
    gamma, cs = torch.randn(512, device="cuda"), capi.rope_table(MAX_POS, 64).cuda()
    ckv_pool = torch.zeros(B * mp, PS, 512, device="cuda", dtype=torch.uint8 if kv8 else torch.half)
    kpe_pool, q_out = torch.zeros(B * mp, PS, 64, device="cuda").half(), torch.empty(T, H, 64, device="cuda").half()
    table = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous()
    cu, lens, scale = i32(cu_of([nq] * B)), i32([L] * B), torch.tensor([SCALE], device="cuda")
    # what the torch composition is handed for nothing: every token's position and its row in the pools
    pos = (L - nq + torch.arange(nq, device="cuda")).repeat(B)
    rows = table.long()[torch.arange(B, device="cuda").repeat_interleave(nq), pos // PS] * PS + pos % PS

    def lib_step():
        if kv8:
            capi.mla_append_paged_kv8(ckv_new, kpe_new, q_pe, ckv_pool, kpe_pool, cs, cu, table, lens, nq, gamma=gamma, eps=EPS, q_pe_out=q_out, ckv_scale=scale)
        else:
            capi.mla_append_paged(ckv_new, kpe_new, q_pe, ckv_pool, kpe_pool, cs, cu, table, lens, nq, gamma=gamma, eps=EPS, q_pe_out=q_out)

    def rot(v, c, s):
        v1, v2 = v[..., :32].float(), v[..., 32:].float()
        return torch.cat([v1 * c - v2 * s, v2 * c + v1 * s], -1).half()

    def torch_step():
        x = ckv_new.float()
        y = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * gamma).half()
        if kv8:
            y = (y.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        ckv_pool.view(-1, 512).index_put_((rows,), y)
        c, s = cs[pos, :32], cs[pos, 32:]
        kpe_pool.view(-1, 64).index_put_((rows,), rot(kpe_new, c, s))
        q_out.copy_(rot(q_pe, c[:, None], s[:, None]))

    nbytes = T * (576 * 2 + 512 * (1 if kv8 else 2) + 64 * 2 + 2 * H * 64 * 2)
    name = capi.mla_append_paged_kernel_name(B, H, T, nq, PS, mp, MAX_POS, kv8=kv8)
    return run_row(f"{label} H{H} {'fp8' if kv8 else '16-bit'}", {name[:name.index("<")].replace("mla_append_paged_", ""): lib_step, "torch ops": torch_step},
                   nbytes, rounds, secs)


def yardstick(rounds, secs):
    B, nq, H, HKV, D, L = 8, 1024, 32, 8, 128, 2048
    T, mp = B * nq, L // PS
    qkv = torch.randn(T, (H + 2 * HKV) * D, device="cuda").half()
    q, k, v = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)
    kp, vp = (torch.zeros(B * mp, HKV, PS, D, device="cuda").half() for _ in range(2))
    table = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous()
    cs, cu, lens, q_out = capi.rope_table(MAX_POS, D).cuda(), i32(cu_of([nq] * B)), i32([L] * B), torch.empty(T, H, D, device="cuda").half()
    run_row("yardstick 8x1024 H32/8", {"rope_varlen": lambda: capi.rope_append_varlen(q, k, v, kp, vp, cs, cu, table, lens, nq, q_out=q_out)},
            T * (2 * H + 4 * HKV) * D * 2, rounds, secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--secs", type=float, default=0.5)
    a = ap.parse_args()
    capi.load()
    capi.require_production()
    torch.manual_seed(0)
    ok = True
    for label, B, nq, H in (("decode B64", 64, 1, 128), ("prefill 8x1024", 8, 1024, 128), ("prefill 8x1024", 8, 1024, 16)):
        for kv8 in (False, True):
            ok = mla_row(label, B, nq, H, kv8, a.rounds, a.secs) and ok
    yardstick(a.rounds, a.secs)
    print(f"AB verdict: the library call is {'faster' if ok else 'NOT faster'} than the torch composition at every shape by more than the spread", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
