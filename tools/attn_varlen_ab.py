"""Time the ragged-batch calls (attn_varlen_paged, rope_append_varlen) against the rectangular calls they replace, and the
existing decode / chunk / local / rope calls against another build of the library, in one process and in alternating rounds:

    python tools/attn_varlen_ab.py [--parent-lib PATH] [--rounds 5] [--secs 0.3] [--rows abcdefg] [--bf16]

H 32 / Hkv 8 / D 128, a paged fp16 cache with pages of 64 keys, every call the bare C entry on prepared arguments.  The rows:
    a  pure decode: B = 64, every Nq_b = 1, L = 4096 — the ragged call against lc_attn_decode_paged_f16 (same RT, same work: the price of VARLEN)
    b  mixed step: 63 decoding sequences + one 512-token chunk at L = 4096 — against lc_attn_chunk_paged_f16 with B = 64, Nq = 512, the
       left-padded call it replaces; the ragged call also under forced S = 1, 2, 4, 8 next to the automatic one, and with max_nq = 528 (row g)
    c  ragged prefill: eight prompts of 100 .. 2048 tokens (kv_len = the prompt) — against the same, left-padded to 2048
    d  empty grid: b with cu_q such that only the 63 decoding sequences hold tokens: what B x Hkv x RB x S mostly-empty workgroups cost
    e  rope: lc_rope_append_varlen_f16 on b and c against lc_rope_append_paged_f16 left-padded
    f  the existing decode, chunk, local and rope calls of THIS library against the same calls of --parent-lib (the parent commit's build)
    g  d again with max_nq = 496, 512 and 528 (RB = 31, 32, 33): the one live row block of every (sequence, K / V head) is workgroup
       (b Hkv + kvh) RB S of the 1-D grid, and consecutive workgroups go round the 8 XCDs — RB S a multiple of 8 puts all of them on one
    h  (--bf16, or --rows h) the bfloat16 entries against their fp16 twins on the SAME shapes, for both cache kinds: a's
       decode step, b's mixed step and c's eight prompts through lc_attn_varlen_paged_f16 / _bf16 and _kv8 / _kv8_bf16, and the mixed step's
       rope call through lc_rope_append_varlen_f16 / _bf16 and _kv8 / _kv8_bf16.  The yardstick of a bf16 line is the fp16 line of its row
Each line: the median, best and worst of the rounds' times (device events around >= --secs seconds of back-to-back calls, after a warm-up), the
kernel name, and the ratio of the medians to the line's reference.  The rounds alternate the variants of a row, each round starting with another
one, so that a drift of the machine lands on all of them.  Needs an MI355X."""
import argparse
import ctypes as C
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from leetcuda_amd import capi  # noqa: E402

H, HKV, D, PS = 32, 8, 128, 64
CAUSAL = capi.ATTN_CAUSAL


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


def call(fn, *args, split=None):
    """one C call, status checked; split: under a forced "attn_decode_split" (set and reset around the call: two atomic stores)"""
    def step():
        if split is not None:
            capi.tune("attn_decode_split", split)
        rc = fn(*args)
        if split is not None:
            capi.tune("attn_decode_split", 0)
        assert rc == 0, rc
    return step


def run_row(row, variants, ref, rounds, secs):
    """variants: {label: (step, kernel name)}; ref: the label the ratios are taken against"""
    times = {k: [] for k in variants}
    order = list(variants)
    for r in range(rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            times[k].append(timed(variants[k][0], secs))
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    for k, (_, name) in variants.items():
        t = sorted(times[k])
        ratio = f"  x{med[k] / med[ref]:6.3f} of {ref}" if k != ref else ""
        print(f"AB {row:16s} {k:18s} {name:46s} median {med[k] * 1e3:9.1f} us  best {t[0] * 1e3:9.1f}  worst {t[-1] * 1e3:9.1f}{ratio}", flush=True)


def pools(B, L):
    mp = L // PS
    kp, vp = (torch.randn(B * mp, HKV, PS, D, device="cuda").half() for _ in range(2))
    table = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous()
    return kp, vp, table, mp


def i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device="cuda")


def cu_of(nqs):
    cu = [0]
    for n in nqs:
        cu.append(cu[-1] + n)
    return cu


def bf16_rows(lib, stream, rounds, secs):
    """row h: per shape and cache kind, the fp16 and the bf16 entry on the same geometry and the same values (the 16-bit tensors of one are the
    other's converted; the fp8 pools and the tables are shared): the bytes moved and the number of instructions issued are the same"""
    BF = torch.bfloat16

    def both(x):
        return {"f16": x, "bf16": x.to(BF)}

    shapes = (("decode", 64, 4096, [1] * 64, 1), ("mixed step", 64, 4096, [1] * 63 + [512], 512),
              ("eight prompts", 8, 2048, [100 + (2048 - 100) * i // 7 for i in range(8)], 2048))
    cs = capi.rope_table(4096, D).cuda()
    for label, B, L, nqs, max_nq in shapes:
        T, mp = sum(nqs), L // PS
        lens = i32([L] * B if label != "eight prompts" else nqs)
        cu = i32(cu_of(nqs))
        table = torch.randperm(B * mp, device="cuda").to(torch.int32).view(B, mp).contiguous()
        q, kp = both(torch.randn(T, H, D, device="cuda").half()), both(torch.randn(B * mp, HKV, PS, D, device="cuda").half())
        vp = both(torch.randn(B * mp, HKV, PS, D, device="cuda").half())
        kp8, vp8 = (torch.randint(0, 0x7E, (B * mp, HKV, PS, D), device="cuda", dtype=torch.uint8) for _ in range(2))      # finite e4m3 codes
        ks, vs = (torch.full((HKV,), 0.25, device="cuda") for _ in range(2))
        o = {k: torch.empty_like(v) for k, v in q.items()}
        for kind in ("paged", "kv8"):
            variants = {}
            for el in ("f16", "bf16"):
                if kind == "paged":
                    fn = lib.lc_attn_varlen_paged_f16 if el == "f16" else lib.lc_attn_varlen_paged_bf16
                    step = call(fn, q[el].data_ptr(), kp[el].data_ptr(), vp[el].data_ptr(), o[el].data_ptr(), cu.data_ptr(), table.data_ptr(),
                                lens.data_ptr(), B, H, HKV, T, max_nq, B * mp, PS, mp, D, 0, None, CAUSAL, None, 0, stream)
                else:
                    fn = lib.lc_attn_varlen_paged_kv8 if el == "f16" else lib.lc_attn_varlen_paged_kv8_bf16
                    step = call(fn, q[el].data_ptr(), kp8.data_ptr(), vp8.data_ptr(), o[el].data_ptr(), cu.data_ptr(), table.data_ptr(), lens.data_ptr(),
                                ks.data_ptr(), vs.data_ptr(), B, H, HKV, T, max_nq, B * mp, PS, mp, D, 0, None, CAUSAL, None, 0, stream)
                namer = capi.attn_varlen_paged_kernel_name if el == "f16" else capi.attn_varlen_paged_bf16_kernel_name
                variants[el] = (step, namer(B, H, HKV, T, max_nq, PS, mp, D, causal=True, kv8=kind == "kv8"))
            run_row(f"h {label} {kind}", variants, "f16", rounds, secs)
        if label != "mixed step":
            continue
        kt, vt = both(torch.randn(T, HKV, D, device="cuda").half()), both(torch.randn(T, HKV, D, device="cuda").half())
        qo = {k: torch.empty_like(v) for k, v in q.items()}
        for kind in ("paged", "kv8"):
            variants = {}
            for el in ("f16", "bf16"):
                sym = {("paged", "f16"): "lc_rope_append_varlen_f16", ("paged", "bf16"): "lc_rope_append_varlen_bf16",
                       ("kv8", "f16"): "lc_rope_append_varlen_kv8", ("kv8", "bf16"): "lc_rope_append_varlen_kv8_bf16"}[kind, el]
                pk, pv = (kp[el], vp[el]) if kind == "paged" else (kp8, vp8)
                scale_ptrs = (ks.data_ptr(), vs.data_ptr()) if kind == "kv8" else ()
                step = call(getattr(lib, sym), q[el].data_ptr(), kt[el].data_ptr(), vt[el].data_ptr(), qo[el].data_ptr(), pk.data_ptr(), pv.data_ptr(),
                            cs.data_ptr(), cu.data_ptr(), table.data_ptr(), lens.data_ptr(), *scale_ptrs, B, H, HKV, T, max_nq, B * mp, PS, mp, D, D, 4096,
                            H * D, HKV * D, 0, stream)
                namer = capi.rope_append_varlen_kernel_name if el == "f16" else capi.rope_append_varlen_bf16_kernel_name
                variants[el] = (step, namer(B, H, HKV, T, max_nq, PS, mp, D, D, 4096, kv8=kind == "kv8"))
            run_row(f"h rope {kind}", variants, "f16", rounds, secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--secs", type=float, default=0.3)
    ap.add_argument("--rows", default="abcdefg")
    ap.add_argument("--bf16", action="store_true", help="time the bfloat16 entries against their fp16 twins (row h) and nothing else")
    a = ap.parse_args()
    if a.bf16:
        a.rows = "h"
    parent = None
    if a.parent_lib:   # its own symbols first (RTLD_DEEPBIND): two builds of one library in a process must not interpose each other
        parent = C.CDLL(a.parent_lib, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for sym in ("lc_attn_decode_paged_f16", "lc_attn_chunk_paged_f16", "lc_attn_local_paged_f16", "lc_rope_append_paged_f16"):
            getattr(parent, sym).restype, getattr(parent, sym).argtypes = capi.SYMBOLS[sym]
    lib = capi.load()
    capi.require_production()
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    ws_tail = (None, 0, stream)

    def varlen(q, o, kp, vp, cu, table, lens, B, T, max_nq, mp, split=None):
        return call(lib.lc_attn_varlen_paged_f16, q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o.data_ptr(), cu.data_ptr(), table.data_ptr(), lens.data_ptr(),
                    B, H, HKV, T, max_nq, kp.shape[0], PS, mp, D, 0, None, CAUSAL, *ws_tail, split=split)

    def vname(B, T, max_nq, mp, split=None):
        if split is not None:
            capi.tune("attn_decode_split", split)
        try:
            return capi.attn_varlen_paged_kernel_name(B, H, HKV, T, max_nq, PS, mp, D, causal=True)
        finally:
            capi.tune("attn_decode_split", 0)

    def rect(fn, q, o, kp, vp, table, lens, B, Nq, mp, *local):
        return call(fn, q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o.data_ptr(), table.data_ptr(), lens.data_ptr(), B, H, HKV, Nq, kp.shape[0], PS, mp, D,
                    *local, CAUSAL, *ws_tail)

    # ---- a, b, d: B = 64 at L = 4096
    if set(a.rows) & set("abdeg"):
        B, L = 64, 4096
        kp, vp, table, mp = pools(B, L)
        lens = i32([L] * B)
    if "a" in a.rows:
        q = torch.randn(B, H, D, device="cuda").half()                     # [T,H,D] with T = B IS [B,H,1,D]
        o = torch.empty_like(q)
        cu = i32(range(B + 1))
        run_row("a decode", {"decode_paged": (rect(lib.lc_attn_decode_paged_f16, q, o, kp, vp, table, lens, B, 1, mp),
                                              capi.attn_decode_paged_kernel_name(B, H, HKV, 1, PS, mp, D, causal=True)),
                             "varlen": (varlen(q, o, kp, vp, cu, table, lens, B, B, 1, mp), vname(B, B, 1, mp))}, "decode_paged", a.rounds, a.secs)
    if set(a.rows) & set("bdeg"):
        nqs = [1] * 63 + [512]
        T = sum(nqs)
        qt = torch.randn(T, H, D, device="cuda").half()
        ot = torch.empty_like(qt)
        qp = torch.randn(B, H, 512, D, device="cuda").half()
        op = torch.empty_like(qp)
        cu = i32(cu_of(nqs))
    if "b" in a.rows:
        variants = {"chunk_paged padded": (rect(lib.lc_attn_chunk_paged_f16, qp, op, kp, vp, table, lens, B, 512, mp),
                                           capi.attn_chunk_paged_kernel_name(B, H, HKV, 512, PS, mp, D, causal=True)),
                    "varlen auto": (varlen(qt, ot, kp, vp, cu, table, lens, B, T, 512, mp), vname(B, T, 512, mp))}
        for s in (1, 2, 4, 8):
            variants[f"varlen S={s}"] = (varlen(qt, ot, kp, vp, cu, table, lens, B, T, 512, mp, split=s), vname(B, T, 512, mp, split=s))
        variants["varlen max_nq=528"] = (varlen(qt, ot, kp, vp, cu, table, lens, B, T, 528, mp), vname(B, T, 528, mp))      # RB = 33: row g
        run_row("b mixed step", variants, "chunk_paged padded", a.rounds, a.secs)
    if "d" in a.rows:
        cu_d = i32(cu_of([1] * 63 + [0]))
        run_row("d empty grid", {"varlen max_nq=1": (varlen(qt, ot, kp, vp, cu_d, table, lens, B, T, 1, mp), vname(B, T, 1, mp)),
                                 "varlen max_nq=512": (varlen(qt, ot, kp, vp, cu_d, table, lens, B, T, 512, mp), vname(B, T, 512, mp))},
                "varlen max_nq=1", a.rounds, a.secs)
    if "g" in a.rows:
        cu_d = i32(cu_of([1] * 63 + [0]))
        run_row("g empty grid RB", {f"varlen max_nq={m}": (varlen(qt, ot, kp, vp, cu_d, table, lens, B, T, m, mp), vname(B, T, m, mp)) for m in (512, 496, 528)},
                "varlen max_nq=512", a.rounds, a.secs)
    # ---- c: eight prompts
    if set(a.rows) & set("ce"):
        Bc, Lc = 8, 2048
        nqc = [100 + (2048 - 100) * i // 7 for i in range(8)]
        Tc = sum(nqc)
        kpc, vpc, tablec, mpc = pools(Bc, Lc)
        lensc = i32(nqc)
        qtc = torch.randn(Tc, H, D, device="cuda").half()
        otc = torch.empty_like(qtc)
        qpc = torch.randn(Bc, H, Lc, D, device="cuda").half()
        opc = torch.empty_like(qpc)
        cuc = i32(cu_of(nqc))
    if "c" in a.rows:
        variants = {"chunk_paged padded": (rect(lib.lc_attn_chunk_paged_f16, qpc, opc, kpc, vpc, tablec, lensc, Bc, Lc, mpc),
                                           capi.attn_chunk_paged_kernel_name(Bc, H, HKV, Lc, PS, mpc, D, causal=True)),
                    "varlen auto": (varlen(qtc, otc, kpc, vpc, cuc, tablec, lensc, Bc, Tc, Lc, mpc), vname(Bc, Tc, Lc, mpc))}
        for s in (1, 2, 4):
            variants[f"varlen S={s}"] = (varlen(qtc, otc, kpc, vpc, cuc, tablec, lensc, Bc, Tc, Lc, mpc, split=s), vname(Bc, Tc, Lc, mpc, split=s))
        run_row("c ragged prefill", variants, "chunk_paged padded", a.rounds, a.secs)
    # ---- e: rope
    if "e" in a.rows:
        cs = capi.rope_table(4096, D).cuda()
        for row, (B_, nq_, T_, mq, kp_, vp_, tab_, lens_, mp_, cu_, qt_, qp_) in (
                ("e rope on b", (B, nqs, T, 512, kp, vp, table, lens, mp, cu, qt, qp)),
                ("e rope on c", (Bc, nqc, Tc, Lc, kpc, vpc, tablec, lensc, mpc, cuc, qtc, qpc))):
            kt, vt = (torch.randn(T_, HKV, D, device="cuda").half() for _ in range(2))
            kr, vr = (torch.randn(B_, HKV, mq, D, device="cuda").half() for _ in range(2))
            qo_t, qo_p = torch.empty_like(qt_), torch.empty_like(qp_)
            run_row(row, {"rope_paged padded": (call(lib.lc_rope_append_paged_f16, qp_.data_ptr(), kr.data_ptr(), vr.data_ptr(), qo_p.data_ptr(), kp_.data_ptr(),
                                                     vp_.data_ptr(), cs.data_ptr(), tab_.data_ptr(), lens_.data_ptr(), B_, H, HKV, mq, kp_.shape[0], PS, mp_, D, D,
                                                     4096, 0, 0, stream),
                                                capi.rope_append_paged_kernel_name(B_, H, HKV, mq, PS, mp_, D, D, 4096)),
                          "rope_varlen": (call(lib.lc_rope_append_varlen_f16, qt_.data_ptr(), kt.data_ptr(), vt.data_ptr(), qo_t.data_ptr(), kp_.data_ptr(),
                                               vp_.data_ptr(), cs.data_ptr(), cu_.data_ptr(), tab_.data_ptr(), lens_.data_ptr(), B_, H, HKV, T_, mq, kp_.shape[0],
                                               PS, mp_, D, D, 4096, H * D, HKV * D, 0, stream),
                                          capi.rope_append_varlen_kernel_name(B_, H, HKV, T_, mq, PS, mp_, D, D, 4096))}, "rope_paged padded", a.rounds, a.secs)
    # ---- h: the bf16 entries against their fp16 twins
    if "h" in a.rows:
        bf16_rows(lib, stream, a.rounds, a.secs)
    # ---- f: the existing calls, this build against the parent's
    if "f" in a.rows:
        if parent is None:
            print("AB f existing calls: not timed (no --parent-lib)", flush=True)
            return
        B, L = 64, 4096
        if not set(a.rows) & set("abdeg"):
            kp, vp, table, mp = pools(B, L)
            lens = i32([L] * B)
        cs = capi.rope_table(4096, D).cuda()
        q1 = torch.randn(B, H, 1, D, device="cuda").half()
        q64 = torch.randn(8, H, 64, D, device="cuda").half()
        o1, o64 = torch.empty_like(q1), torch.empty_like(q64)
        k1, v1 = (torch.randn(B, HKV, 1, D, device="cuda").half() for _ in range(2))
        k64, v64 = (torch.randn(8, HKV, 64, D, device="cuda").half() for _ in range(2))
        lens8 = i32([L] * 8)
        for row, sym, args, name in (
                ("f decode B64 q1", "lc_attn_decode_paged_f16", (q1, o1, kp, vp, table, lens, B, 1, mp), capi.attn_decode_paged_kernel_name(B, H, HKV, 1, PS, mp, D, causal=True)),
                ("f chunk B8 q64", "lc_attn_chunk_paged_f16", (q64, o64, kp, vp, table, lens8, 8, 64, mp), capi.attn_chunk_paged_kernel_name(8, H, HKV, 64, PS, mp, D, causal=True)),
                ("f local W=128", "lc_attn_local_paged_f16", (q1, o1, kp, vp, table, lens, B, 1, mp, 128, None),
                 capi.attn_local_paged_kernel_name(B, H, HKV, 1, PS, mp, D, causal=True, window=128)),
                ("f local q64 W=4k", "lc_attn_local_paged_f16", (q64, o64, kp, vp, table, lens8, 8, 64, mp, 4096, None),
                 capi.attn_local_paged_kernel_name(8, H, HKV, 64, PS, mp, D, causal=True, window=4096))):
            run_row(row, {"parent": (rect(getattr(parent, sym), *args), "(the parent build's choice)"), "this": (rect(getattr(lib, sym), *args), name)},
                    "parent", a.rounds, a.secs)
        for row, (qq, kk, vv, ll_, Bq, Nq) in (("f rope B64 q1", (q1, k1, v1, lens, B, 1)), ("f rope B8 q64", (q64, k64, v64, lens8, 8, 64))):
            qo = torch.empty_like(qq)
            rargs = (qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), qo.data_ptr(), kp.data_ptr(), vp.data_ptr(), cs.data_ptr(), table.data_ptr(), ll_.data_ptr(),
                     Bq, H, HKV, Nq, kp.shape[0], PS, mp, D, D, 4096, 0, 0, stream)
            run_row(row, {"parent": (call(parent.lc_rope_append_paged_f16, *rargs), "(the parent build's choice)"),
                          "this": (call(lib.lc_rope_append_paged_f16, *rargs), capi.rope_append_paged_kernel_name(Bq, H, HKV, Nq, PS, mp, D, D, 4096))},
                    "parent", a.rounds, a.secs)


if __name__ == "__main__":
    main()
