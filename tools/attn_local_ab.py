"""Time attn_local_paged (sliding window) against the full-length paged decode call, per shape and in alternating rounds:

    python tools/attn_local_ab.py [--parent-lib PATH] [--rounds 5] [--secs 0.3] [--page 64]

Per shape "B,H,L,D:q=Nq:kvh=Hkv" (every sequence at kv_len = L = the capacity), one line each for
    full        attn_decode_paged of THIS library at full length
    parent      the same call of another build of the library (--parent-lib: the parent commit's libleetcuda_amd.so), if given
    W=128 / W=4096   attn_local_paged, causal, with that window
with the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls, after a warm-up), the kernel
name, and for the windows the ratio to `full` and the share of keys a workgroup may see, (W + Nq - 1) / L.  The rounds alternate the variants, so
that a drift of the machine lands on all of them.  Needs an MI355X."""
import argparse
import ctypes as C
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402

SHAPES = ["1,32,8192,128:q=1:kvh=8", "16,32,4096,128:q=1:kvh=8", "64,32,2048,128:q=1:kvh=8", "4,64,32768,128:q=1:kvh=8", "8,32,4096,128:q=4:kvh=8",
          "8,32,4096,64:q=1:kvh=32", "8,64,32768,64:q=1:kvh=8"]
WINDOWS = (128, 4096)


def timed(step, secs):
    """ms per call of `step` over >= secs seconds of back-to-back calls"""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        step()
    e1.record()
    torch.cuda.synchronize()
    n = max(5, int(secs / (e0.elapsed_time(e1) / 5 * 1e-3)))
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.3)
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("shapes", nargs="*", default=SHAPES)
    a = ap.parse_args()
    parent = None
    if a.parent_lib:   # its own symbols first (RTLD_DEEPBIND): two builds of one library in a process must not interpose each other
        parent =C.CDLL(a.parent_lib, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        parent.lc_attn_decode_paged_f16.restype, parent.lc_attn_decode_paged_f16.argtypes = capi.SYMBOLS["lc_attn_decode_paged_f16"]
    capi.load()
    capi.require_production()
    ps = a.page
    for spec in a.shapes:
        dims, *opts = spec.split(":")
        B, H, L, D = (int(x) for x in dims.split(","))
        Nq = next((int(o[2:]) for o in opts if o.startswith("q=")), 1)
        Hkv = next((int(o[4:]) for o in opts if o.startswith("kvh=")), H)
        mp = L // ps
        torch.manual_seed(0)
        q = torch.randn(B, H, Nq, D, device="cuda").half()
        kp, vp = (torch.randn(B * mp, Hkv, ps, D, device="cuda").half() for _ in range(2))
        table = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous()
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        o = torch.empty_like(q)
        stream = torch.cuda.current_stream().cuda_stream

        # every variant through the bare C call on prepared arguments: at these sizes a Python wrapper's checks cost as much as the kernel
        ptrs = (q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o.data_ptr(), table.data_ptr(), lens.data_ptr())
        geo = (B, H, Hkv, Nq, B * mp, ps, mp, D)
        tail = (capi.ATTN_CAUSAL, None, 0, stream)

        def call(fn, *args):
            def step():
                rc = fn(*args)
                assert rc == 0, rc
            return step

        lib = capi.load()
        variants = {"full": (call(lib.lc_attn_decode_paged_f16, *ptrs, *geo, *tail), capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=True))}
        if parent is not None:
            variants["parent"] = (call(parent.lc_attn_decode_paged_f16, *ptrs, *geo, *tail), "(the parent build's choice)")
        for w in WINDOWS:
            variants[f"W={w}"] = (call(lib.lc_attn_local_paged_f16, *ptrs, *geo, w, None, *tail),
                                  capi.attn_local_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=True, window=w))
        times = {k: [] for k in variants}
        order = list(variants)
        for r in range(a.rounds):
            for k in order[r % len(order):] + order[:r % len(order)]:      # (each round starts with another variant)
                times[k].append(timed(variants[k][0], a.secs))
        full = sorted(times["full"])[a.rounds // 2]
        for k, (_, name) in variants.items():
            t = sorted(times[k])
            med = t[len(t) // 2]
            tail = ""
            if k.startswith("W="):
                tail = f"  x{med / full:5.3f} of full  keys {min(1.0, (int(k[2:]) + Nq - 1) / L):5.3f} of L"
            print(f"AB {spec + ':page=' + str(ps):34s} {k:7s} {name:42s} median {med * 1e3:8.1f} us  best {t[0] * 1e3:8.1f}  worst {t[-1] * 1e3:8.1f}{tail}",
                  flush=True)


if __name__ == "__main__":
    main()
