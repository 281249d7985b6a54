"""Time the tree-speculation entries against their twins (lc_attn_varlen_paged_tree_*, lc_rope_append_varlen_pos_*), in
one process and in alternating rounds, and write the lines to profiles/attn_tree_ab.log:

    python tools/attn_tree_ab.py [--rounds 5] [--secs 0.3] [--rows abc] [--out profiles/attn_tree_ab.log]

H 32 / Hkv 8 / D 128, L = 4096, pages of 64 keys, every call the bare C entry on prepared arguments (tools/attn_varlen_ab.py's harness).  The rows:
    a  what an all-ones mask costs: each tree entry with words of all ones against its LSE twin on the same arguments, for both element types
       and both cache kinds: a decode step (B = 64, every Nq_b = 1) and a mixed step (63 decoding sequences + one 512-token chunk).  The twin
       is timed TWICE in every round ("lse" and "lse again"): the second line's ratio to the first is the twin's own run-to-run spread, to be
       read next to the tree line's ratio
    b  a verify step: B = 64 random draft trees of 16 and of 64 tokens each, through the tree entry with the trees' masks, through the tree
       entry with all-ones words and through the LSE twin (a linear chain of the same shape).  The mask saves no tile loads — the workgroups
       walk the twin's tiles — so the line says what the mask COSTS
    c  the rope + append call with pos_ids against its twin on a's mixed step, both element types and both cache kinds
Each line: the median, best and worst of the rounds' times, the kernel name, and the ratio of the medians to the line's reference.  Needs an
MI355X."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import attn_varlen_ab as ab  # noqa: E402
from attn_varlen_ab import CAUSAL, D, H, HKV, PS, call, cu_of, i32  # noqa: E402
from leetcuda_amd import capi  # noqa: E402

BF = torch.bfloat16
L = 4096
SUFFIX = {("paged", "f16"): "f16", ("kv8", "f16"): "kv8", ("paged", "bf16"): "bf16", ("kv8", "bf16"): "kv8_bf16"}
CONFIGS = (("f16", "paged"), ("f16", "kv8"), ("bf16", "paged"), ("bf16", "kv8"))


class Tee:
    """print() to the terminal and into the log"""

    def __init__(self, path):
        self.out, self.file = sys.stdout, open(path, "w")

    def write(self, s):
        self.out.write(s)
        self.file.write(s)

    def flush(self):
        self.out.flush()
        self.file.flush()


def geometry(B, nqs):
    T, mp = sum(nqs), L // PS
    g = dict(B=B, T=T, mp=mp, lens=i32([L] * B), cu=i32(cu_of(nqs)),
             table=torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous(),
             q16=torch.randn(T, H, D, device="cuda").half(),
             kp16=torch.randn(B * mp, HKV, PS, D, device="cuda").half(), vp16=torch.randn(B * mp, HKV, PS, D, device="cuda").half(),
             kp8=torch.randint(0, 0x7E, (B * mp, HKV, PS, D), device="cuda", dtype=torch.uint8),      # finite e4m3 codes
             vp8=torch.randint(0, 0x7E, (B * mp, HKV, PS, D), device="cuda", dtype=torch.uint8),
             ks=torch.full((HKV,), 0.25, device="cuda"), vs=torch.full((HKV,), 0.25, device="cuda"),
             lse=torch.empty(T, H, device="cuda"))
    return g


def attn_steps(lib, stream, g, el, kind, max_nq, masks):
    """(the LSE twin's step, {label: the tree entry's step under that mask}, the two kernel names)"""
    q, kp, vp = (x if el == "f16" else x.to(BF) for x in (g["q16"], g["kp16"], g["vp16"]))
    pk, pv = (kp, vp) if kind == "paged" else (g["kp8"], g["vp8"])
    o = torch.empty_like(q)
    keep = (q, pk, pv, o)                                             # (the steps hold addresses, not tensors)
    sc = (g["ks"].data_ptr(), g["vs"].data_ptr()) if kind == "kv8" else ()
    B, T, mp = g["B"], g["T"], g["mp"]
    tail = (g["cu"].data_ptr(), g["table"].data_ptr(), g["lens"].data_ptr(), *sc, B, H, HKV, T, max_nq, B * mp, PS, mp, D, 0, None, CAUSAL, None, 0, stream)
    head = (q.data_ptr(), pk.data_ptr(), pv.data_ptr(), o.data_ptr(), g["lse"].data_ptr())
    twin = call(getattr(lib, "lc_attn_varlen_paged_lse_" + SUFFIX[kind, el]), *head, *tail)
    tree = {k: call(getattr(lib, "lc_attn_varlen_paged_tree_" + SUFFIX[kind, el]), *head, m.data_ptr(), *tail) for k, m in masks.items()}
    names = (capi.attn_varlen_paged_lse_kernel_name(B, H, HKV, T, max_nq, PS, mp, D, causal=True, kv8=kind == "kv8", bf16=el == "bf16"),
             capi.attn_varlen_paged_tree_kernel_name(B, H, HKV, T, max_nq, PS, mp, D, kv8=kind == "kv8", bf16=el == "bf16"))
    return twin, tree, names, keep


def ones_rows(lib, stream, rounds, secs):
    for label, nqs, max_nq in (("decode", [1] * 64, 1), ("mixed step", [1] * 63 + [512], 512)):
        g = geometry(64, nqs)
        ones = torch.full((g["T"],), -1, dtype=torch.int64, device="cuda")
        for el, kind in CONFIGS:
            twin, tree, (tname, sname), keep = attn_steps(lib, stream, g, el, kind, max_nq, {"ones": ones})
            ab.run_row(f"a {label} {el} {kind}", {"lse": (twin, tname), "lse again": (twin, tname), "tree all ones": (tree["ones"], sname)}, "lse",
                       rounds, secs)
    return g                                                          # the mixed step: row c's geometry


def verify_rows(lib, stream, rounds, secs):
    rng = np.random.default_rng(0)
    for n in (16, 64):
        B = 64
        g = geometry(B, [n] * B)
        parents = [[int(rng.integers(-1, i)) if rng.random() < 0.5 else i - 1 for i in range(n)] for _ in range(B)]
        masks = {"trees": capi.tree_mask(parents, cu_of([n] * B)).cuda(), "ones": torch.full((g["T"],), -1, dtype=torch.int64, device="cuda")}
        for el, kind in CONFIGS[:3]:
            twin, tree, (tname, sname), keep = attn_steps(lib, stream, g, el, kind, n, masks)
            ab.run_row(f"b verify {n} {el} {kind}", {"lse (a chain)": (twin, tname), "tree all ones": (tree["ones"], sname),
                                                     "tree masks": (tree["trees"], sname)}, "lse (a chain)", rounds, secs)


def rope_rows(lib, stream, rounds, secs, g):
    B, T, mp = g["B"], g["T"], g["mp"]
    cs = capi.rope_table(L, D).cuda()
    pos = torch.randint(0, L, (T,), device="cuda", dtype=torch.int32)
    for el, kind in CONFIGS:
        q, kp, vp = (x if el == "f16" else x.to(BF) for x in (g["q16"], g["kp16"], g["vp16"]))
        kt, vt = (torch.randn(T, HKV, D, device="cuda").to(q.dtype) for _ in range(2))
        qo = torch.empty_like(q)
        pk, pv = (kp, vp) if kind == "paged" else (g["kp8"], g["vp8"])
        sc = (g["ks"].data_ptr(), g["vs"].data_ptr()) if kind == "kv8" else ()
        head = (q.data_ptr(), kt.data_ptr(), vt.data_ptr(), qo.data_ptr(), pk.data_ptr(), pv.data_ptr(), cs.data_ptr(), g["cu"].data_ptr())
        tail = (g["table"].data_ptr(), g["lens"].data_ptr(), *sc, B, H, HKV, T, 512, B * mp, PS, mp, D, D, L, H * D, HKV * D, 0, stream)
        twin_sym = "lc_rope_append_varlen_" + SUFFIX[kind, el]
        namer = capi.rope_append_varlen_kernel_name if el == "f16" else capi.rope_append_varlen_bf16_kernel_name
        ab.run_row(f"c rope {el} {kind}",
                   {"twin": (call(getattr(lib, twin_sym), *head, *tail), namer(B, H, HKV, T, 512, PS, mp, D, D, L, kv8=kind == "kv8")),
                    "pos_ids": (call(getattr(lib, "lc_rope_append_varlen_pos_" + SUFFIX[kind, el]), *head, pos.data_ptr(), *tail),
                                capi.rope_append_varlen_pos_kernel_name(B, H, HKV, T, 512, PS, mp, D, D, L, kv8=kind == "kv8", bf16=el == "bf16"))},
                   "twin", rounds, secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.3)
    ap.add_argument("--rows", default="abc")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "attn_tree_ab.log"))
    a = ap.parse_args()
    lib = capi.load()
    capi.require_production()
    sys.stdout = Tee(a.out)
    print(f"# python tools/attn_tree_ab.py   (MI355X, one process, {a.rounds} alternating rounds, --secs {a.secs}; DESIGN.md section 4.3o).  H {H} / Hkv {HKV} / "
          f"D {D}, L {L}, page {PS}.  Row a: each tree entry with all-ones words against its LSE twin, the twin timed twice a round (decode: B 64, every "
          "Nq_b 1; mixed step: 63 x 1 + 512 tokens).  Row b: B 64 draft trees of 16 / 64 tokens through the LSE twin, the tree entry with all-ones "
          "words and the tree entry with the trees' masks.  Row c: the rope + append call with pos_ids against its twin on the mixed step", flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    mixed = None
    if "a" in a.rows:
        mixed = ones_rows(lib, stream, a.rounds, a.secs)
    if "b" in a.rows:
        verify_rows(lib, stream, a.rounds, a.secs)
    if "c" in a.rows:
        rope_rows(lib, stream, a.rounds, a.secs, mixed or geometry(64, [1] * 63 + [512]))


if __name__ == "__main__":
    main()
