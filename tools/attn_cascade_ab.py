"""Time the log-sum-exp ragged entries against their twins, and the shared-prefix (cascade) step against the single-level ragged call it replaces
(lc_attn_varlen_paged_lse_*, lc_attn_merge_states_*), in one process and in alternating rounds:

    python tools/attn_cascade_ab.py [--rounds 5] [--secs 0.3] [--rows ab]

H 32 / Hkv 8 / D 128, pages of 64 keys, every call the bare C entry on prepared arguments (tools/attn_varlen_ab.py's harness).  The rows:
    a  each LSE entry against its non-LSE twin on the same arguments, for both element types and both cache kinds: a decode step (B = 64, every
       Nq_b = 1, L = 4096) and a mixed step (63 decoding sequences + one 512-token chunk).  The yardstick of an LSE line is the twin's line of
       its row, in the same run
    b  pure decode behind a shared prefix, 256 private keys a sequence: the single-level ragged call on tables whose first pages are the shared
       ones, against [prefix call (one group of B tokens, non-causal) + suffix call + merge in place].  B = 64 behind 4096 and behind 1024
       shared keys, B = 8 behind 4096, and B = 1 behind 4096 — no sharing at all: what the two extra launches cost.  The yardstick is the
       single-level call of the same run; the line of the cascade names the prefix call's plan with its RB (row blocks per K / V head)
Each line: the median, best and worst of the rounds' times, the kernel name, and the ratio of the medians to the line's reference.  Needs an
MI355X."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from attn_varlen_ab import CAUSAL, D, H, HKV, PS, call, cu_of, i32, run_row  # noqa: E402
from leetcuda_amd import capi  # noqa: E402

BF = torch.bfloat16


def lse_rows(lib, stream, rounds, secs):
    """row a: the twin and the LSE entry on the same geometry and the same values"""
    for label, B, L, nqs, max_nq in (("decode", 64, 4096, [1] * 64, 1), ("mixed step", 64, 4096, [1] * 63 + [512], 512)):
        T, mp = sum(nqs), L // PS
        lens, cu = i32([L] * B), i32(cu_of(nqs))
        table = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous()
        q16 = torch.randn(T, H, D, device="cuda").half()
        kp16, vp16 = (torch.randn(B * mp, HKV, PS, D, device="cuda").half() for _ in range(2))
        kp8, vp8 = (torch.randint(0, 0x7E, (B * mp, HKV, PS, D), device="cuda", dtype=torch.uint8) for _ in range(2))      # finite e4m3 codes
        ks, vs = (torch.full((HKV,), 0.25, device="cuda") for _ in range(2))
        lse = torch.empty(T, H, device="cuda")
        for el in ("f16", "bf16"):
            q, kp, vp = (x if el == "f16" else x.to(BF) for x in (q16, kp16, vp16))
            o = torch.empty_like(q)
            for kind in ("paged", "kv8"):
                pk, pv = (kp, vp) if kind == "paged" else (kp8, vp8)
                sc = (ks.data_ptr(), vs.data_ptr()) if kind == "kv8" else ()
                tail = (*sc, B, H, HKV, T, max_nq, B * mp, PS, mp, D, 0, None, CAUSAL, None, 0, stream)
                twin = {("paged", "f16"): "lc_attn_varlen_paged_f16", ("kv8", "f16"): "lc_attn_varlen_paged_kv8",
                        ("paged", "bf16"): "lc_attn_varlen_paged_bf16", ("kv8", "bf16"): "lc_attn_varlen_paged_kv8_bf16"}[kind, el]
                sym = "lc_attn_varlen_paged_lse_" + {("paged", "f16"): "f16", ("kv8", "f16"): "kv8", ("paged", "bf16"): "bf16",
                                                     ("kv8", "bf16"): "kv8_bf16"}[kind, el]
                namer = capi.attn_varlen_paged_kernel_name if el == "f16" else capi.attn_varlen_paged_bf16_kernel_name
                variants = {
                    "twin": (call(getattr(lib, twin), q.data_ptr(), pk.data_ptr(), pv.data_ptr(), o.data_ptr(), cu.data_ptr(), table.data_ptr(),
                                  lens.data_ptr(), *tail), namer(B, H, HKV, T, max_nq, PS, mp, D, causal=True, kv8=kind == "kv8")),
                    "lse": (call(getattr(lib, sym), q.data_ptr(), pk.data_ptr(), pv.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(),
                                 table.data_ptr(), lens.data_ptr(), *tail),
                            capi.attn_varlen_paged_lse_kernel_name(B, H, HKV, T, max_nq, PS, mp, D, causal=True, kv8=kind == "kv8", bf16=el == "bf16"))}
                run_row(f"a {label} {el} {kind}", variants, "twin", rounds, secs)


def cascade_rows(lib, stream, rounds, secs):
    """row b: fp16, pure decode; one pool holds the shared prefix pages and 256 private keys a sequence"""
    SUF = 256
    for B, P in ((64, 4096), (64, 1024), (8, 4096), (1, 4096)):
        pp, sp = P // PS, SUF // PS
        npg = pp + B * sp
        kp, vp = (torch.randn(npg, HKV, PS, D, device="cuda").half() for _ in range(2))
        perm = torch.randperm(npg, device="cuda").to(torch.int32)
        ptab = perm[:pp].view(1, pp).contiguous()
        stab = perm[pp:].view(B, sp).contiguous()
        full = torch.cat([ptab.expand(B, pp), stab], dim=1).contiguous()
        q = torch.randn(B, H, D, device="cuda").half()
        o1, o, o_p = (torch.empty_like(q) for _ in range(3))
        lse, lse_p = (torch.empty(B, H, device="cuda") for _ in range(2))
        cu, cg = i32(range(B + 1)), i32([0, B])
        len_full, len_suf, len_p = i32([P + SUF] * B), i32([SUF] * B), i32([P])

        single = call(lib.lc_attn_varlen_paged_f16, q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o1.data_ptr(), cu.data_ptr(), full.data_ptr(),
                      len_full.data_ptr(), B, H, HKV, B, 1, npg, PS, pp + sp, D, 0, None, CAUSAL, None, 0, stream)
        prefix = call(lib.lc_attn_varlen_paged_lse_f16, q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o_p.data_ptr(), lse_p.data_ptr(), cg.data_ptr(),
                      ptab.data_ptr(), len_p.data_ptr(), 1, H, HKV, B, B, npg, PS, pp, D, 0, None, 0, None, 0, stream)
        suffix = call(lib.lc_attn_varlen_paged_lse_f16, q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(),
                      stab.data_ptr(), len_suf.data_ptr(), B, H, HKV, B, 1, npg, PS, sp, D, 0, None, CAUSAL, None, 0, stream)
        merge = call(lib.lc_attn_merge_states_f16, o.data_ptr(), lse.data_ptr(), o_p.data_ptr(), lse_p.data_ptr(), o.data_ptr(), lse.data_ptr(),
                     cu.data_ptr(), B, B, H, D, stream)

        def cascade():
            prefix()
            suffix()
            merge()

        # the two paths must agree before either is timed
        single()
        cascade()
        torch.cuda.synchronize()
        err = float((o.float() - o1.float()).abs().max())
        assert err < 2e-3, err
        rb = ((H // HKV) * B + 63) // 64
        pname = capi.attn_varlen_paged_lse_kernel_name(1, H, HKV, B, B, PS, pp, D)
        sname = capi.attn_varlen_paged_lse_kernel_name(B, H, HKV, B, 1, PS, sp, D, causal=True)
        variants = {"single level": (single, capi.attn_varlen_paged_kernel_name(B, H, HKV, B, 1, PS, pp + sp, D, causal=True)),
                    "cascade": (cascade, f"RB={rb} {pname} + {sname} + merge"),
                    "prefix call": (prefix, pname), "suffix call": (suffix, sname), "merge": (merge, "attn_merge_states_kernel<128>")}
        run_row(f"b B={B} P={P}", variants, "single level", rounds, secs)
        print(f"AB b B={B} P={P}: max |cascade - single level| = {err:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.3)
    ap.add_argument("--rows", default="ab")
    a = ap.parse_args()
    lib = capi.load()
    capi.require_production()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    if "a" in a.rows:
        lse_rows(lib, stream, a.rounds, a.secs)
    if "b" in a.rows:
        cascade_rows(lib, stream, a.rounds, a.secs)


if __name__ == "__main__":
    main()
