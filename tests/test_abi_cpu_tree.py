"""CPU tests of the boundary of the tree-speculation entries (lc_attn_varlen_paged_tree_f16 / _tree_kv8 / _tree_bf16 / _tree_kv8_bf16,
lc_rope_append_varlen_pos_f16 / _pos_kv8 / _pos_bf16 / _pos_kv8_bf16 and their eight name calls; no call here reaches a
device): header, capi.SYMBOLS and exports agree on the 16 symbols; every bad-argument case gives a tree entry the status of its LSE twin, in
the twin's order, with the NULL and the misaligned mask, the missing causal flag and the NULL pos_ids at their places; the name calls report
the twin's plan with `tree` in the kernel; the workspace is the twin's; the five new audit reports; capi.tree_mask / capi.tree_positions
against the brute force of tests/tree_lib.py; and what the GPU module's reference rests on."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import decode_lib as dl
from tests import lse_lib as sl
from tests import tree_lib as tl
from tests import varlen_lib as vl

P = C.c_void_p(16)
CAUSAL = capi.ATTN_CAUSAL
BF = torch.bfloat16
# (kind, bf16) -> LSE run entry, tree run entry, pointers in front of the twin's shape, LSE name call, tree name call
ENTRIES = {
    ("paged", False): ("lc_attn_varlen_paged_lse_f16", "lc_attn_varlen_paged_tree_f16", 8, "lc_attn_varlen_paged_lse_kernel_name",
                       "lc_attn_varlen_paged_tree_kernel_name"),
    ("kv8", False): ("lc_attn_varlen_paged_lse_kv8", "lc_attn_varlen_paged_tree_kv8", 10, "lc_attn_varlen_paged_lse_kv8_kernel_name",
                     "lc_attn_varlen_paged_tree_kv8_kernel_name"),
    ("paged", True): ("lc_attn_varlen_paged_lse_bf16", "lc_attn_varlen_paged_tree_bf16", 8, "lc_attn_varlen_paged_lse_bf16_kernel_name",
                      "lc_attn_varlen_paged_tree_bf16_kernel_name"),
    ("kv8", True): ("lc_attn_varlen_paged_lse_kv8_bf16", "lc_attn_varlen_paged_tree_kv8_bf16", 10, "lc_attn_varlen_paged_lse_kv8_bf16_kernel_name",
                    "lc_attn_varlen_paged_tree_kv8_bf16_kernel_name"),
}
# twin run entry, _pos_ run entry, pointers in front of the twin's shape, twin name call, _pos_ name call
ROPES = (("lc_rope_append_varlen_f16", "lc_rope_append_varlen_pos_f16", 10, "lc_rope_append_varlen_kernel_name", "lc_rope_append_varlen_pos_kernel_name"),
         ("lc_rope_append_varlen_kv8", "lc_rope_append_varlen_pos_kv8", 12, "lc_rope_append_varlen_kv8_kernel_name",
          "lc_rope_append_varlen_pos_kv8_kernel_name"),
         ("lc_rope_append_varlen_bf16", "lc_rope_append_varlen_pos_bf16", 10, "lc_rope_append_varlen_bf16_kernel_name",
          "lc_rope_append_varlen_pos_bf16_kernel_name"),
         ("lc_rope_append_varlen_kv8_bf16", "lc_rope_append_varlen_pos_kv8_bf16", 12, "lc_rope_append_varlen_kv8_bf16_kernel_name",
          "lc_rope_append_varlen_pos_kv8_bf16_kernel_name"))
BYTES = {"paged": "lc_attn_varlen_paged_workspace_bytes", "kv8": "lc_attn_varlen_paged_kv8_workspace_bytes"}
OK = (2, 8, 2, 40, 20, 70, 16, 64, 128)                        # B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D
BAD = (2, 8, 3, 40, 20, 70, 16, 64, 256)
MASK_AT = 5                                                     # the position of `tree_mask`: right behind lse
POS_AT = 8                                                      # the position of `pos_ids`: right behind cu_q


@pytest.fixture
def knobs(built):
    yield from dl.reset_knobs()


def _with_mask(ptrs, mask=P):
    return list(ptrs[:MASK_AT]) + [mask] + list(ptrs[MASK_AT:])


def _run(sym, ptrs, shape, window, flags, sinks=None, ws=(None, 0)):
    """status of a run call on dummy pointers (only ever used on calls a check refuses: nothing reaches a device)"""
    return getattr(capi.load(), sym)(*ptrs, *shape, window, sinks, flags, *ws, None)


def _name(sym, shape, window, flags):
    B, H, Hkv, T, max_nq, _, ps, mp, D = shape
    return vl._rc_name(sym, B, H, Hkv, T, max_nq, ps, mp, D, window, flags)


def test_header_symbols_and_exports_agree(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()

    def params(sym):
        m = re.search(r"\b" + sym + r"\(([^)]*)\)", header)
        assert m, sym
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]

    new = []
    for twin, sym, nptr, tname, sname in ENTRIES.values():
        for s in (sym, sname):
            assert hasattr(lib, s) and s in capi.SYMBOLS, s
        want = params(twin)
        assert want[MASK_AT - 1] == "float* lse"
        assert params(sym) == want[:MASK_AT] + ["const uint64_t* tree_mask"] + want[MASK_AT:], sym
        res, args = capi.SYMBOLS[twin]
        assert capi.SYMBOLS[sym] == (res, args[:MASK_AT] + [C.c_void_p] + args[MASK_AT:]), sym
        assert params(sname) == params(tname) and capi.SYMBOLS[sname] == capi.SYMBOLS[tname], sname
        new += [sym, sname]
    for twin, sym, nptr, tname, sname in ROPES:
        for s in (sym, sname):
            assert hasattr(lib, s) and s in capi.SYMBOLS, s
        want = params(twin)
        assert want[POS_AT - 1] == "const int* cu_q"
        assert params(sym) == want[:POS_AT] + ["const int* pos_ids"] + want[POS_AT:], sym
        res, args = capi.SYMBOLS[twin]
        assert capi.SYMBOLS[sym] == (res, args[:POS_AT] + [C.c_void_p] + args[POS_AT:]), sym
        assert params(sname) == params(tname) and capi.SYMBOLS[sname] == capi.SYMBOLS[tname], sname
        new += [sym, sname]
    assert len(set(new)) == 16
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays
    for s in ("lc_attn_varlen_paged_tree_workspace_bytes", "lc_attn_varlen_paged_tree_kv8_workspace_bytes",    # the twins' queries serve the tree entries
              "lc_attn_local_paged_tree_f16", "lc_attn_decode_paged_tree_f16", "lc_rope_append_paged_pos_f16"):
        assert not hasattr(lib, s) and s not in capi.SYMBOLS, s


@pytest.mark.parametrize("key", list(ENTRIES), ids=lambda k: f"{k[0]}-{'bf16' if k[1] else 'f16'}")
def test_every_bad_argument_gets_the_status_of_the_twin_in_the_twins_order(built, key):
    twin, sym, nptr, tname, sname = ENTRIES[key]
    seen = []

    def both(want, shape, w, flags, ptrs=None, **kw):
        ptrs = [P] * nptr if ptrs is None else ptrs
        got = [_run(twin, ptrs, shape, w, flags, **kw), _run(sym, _with_mask(ptrs), shape, w, flags, **kw)]
        assert got == [want, want], (shape, w, flags, got)
        seen.append(want)

    def both_names(want, shape, w, flags):
        got = [_name(s, shape, w, flags)[0] for s in (tname, sname)]
        assert got == [want, want], (shape, w, flags, got)

    # the flags and the window, in front of everything
    for w, flags in ((-1, CAUSAL), (5, 0), (0, 4), (0, 4 | CAUSAL), (5, capi.ATTN_V_TRANSPOSED)):
        both(capi.LC_ERR_ARG, OK, w, flags)
        both(capi.LC_ERR_ARG, BAD, w, flags)
        both_names(capi.LC_ERR_ARG, BAD, w, flags)
    # a tree call without LC_ATTN_CAUSAL: the status of a window without it, at that place — in front of the NULL pointers and of the shape
    for shape in (OK, BAD):
        assert _run(sym, _with_mask([P] * nptr), shape, 0, 0) == capi.LC_ERR_ARG
        assert _name(sname, shape, 0, 0)[0] == capi.LC_ERR_ARG
    assert _run(twin, [P] * nptr, BAD, 0, 0) == capi.LC_ERR_SHAPE and _name(tname, BAD, 0, 0)[0] == capi.LC_ERR_SHAPE      # (the twin takes it)
    # a NULL pointer — lse and cu_q among them — in front of the shape
    for i in range(8):
        ptrs = [P] * nptr
        ptrs[i] = None
        both(capi.LC_ERR_ARG, BAD, 7, CAUSAL, ptrs=ptrs)
    assert _run(sym, _with_mask([P] * nptr, None), BAD, 7, CAUSAL) == capi.LC_ERR_ARG       # ... and tree_mask = NULL
    assert _run(sym, _with_mask([P] * nptr, None), OK, 0, CAUSAL) == capi.LC_ERR_ARG
    # the shape, in front of the alignment
    mis = [P] * nptr
    mis[0] = C.c_void_p(8)
    for T, mq in ((0, 1), (-3, 1), (40, 0), (40, -1), (40, 41), (1, 2)):
        bad = (2, 8, 2, T, mq, 70, 16, 64, 96)
        both(capi.LC_ERR_SHAPE, bad, 0, CAUSAL)
        both(capi.LC_ERR_SHAPE, bad, 0, CAUSAL, ptrs=mis)
        both_names(capi.LC_ERR_SHAPE, bad, 0, CAUSAL)
    both(capi.LC_ERR_SHAPE, BAD, 0, CAUSAL)
    both(capi.LC_ERR_SHAPE, (2, 8, 2, 40, 20, 70, 24, 64, 128), 0, CAUSAL)             # a page size that is no power of two
    both(capi.LC_ERR_SHAPE, (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, CAUSAL, ptrs=mis)     # alignment in front of the head dim
    # a tree_mask off 8 bytes joins the alignment check: in front of the head dim, behind the shape; 8 bytes are enough
    for off in (4, 12, 17):
        assert _run(sym, _with_mask([P] * nptr, C.c_void_p(32 + off)), (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, CAUSAL) == capi.LC_ERR_SHAPE, off
        assert _run(sym, _with_mask([P] * nptr, C.c_void_p(32 + off)), OK, 0, CAUSAL) == capi.LC_ERR_SHAPE, off
    assert _run(sym, _with_mask([P] * nptr, C.c_void_p(24)), (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, CAUSAL) == capi.LC_ERR_HEADDIM
    both(capi.LC_ERR_HEADDIM, (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, CAUSAL)
    both_names(capi.LC_ERR_HEADDIM, (2, 8, 2, 40, 40, 70, 16, 64, 96), 7, CAUSAL)
    both_names(capi.LC_OK, (2, 8, 2, 40, 40, 70, 16, 64, 64), 7, CAUSAL)
    for s in (tname, sname):
        fn = getattr(capi.load(), s)
        assert fn(2, 8, 2, 40, 20, 16, 64, 128, 0, CAUSAL, None, 128) == capi.LC_ERR_ARG
        assert fn(2, 8, 2, 40, 20, 16, 64, 128, 0, CAUSAL, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
    assert {capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM} == set(seen)


@pytest.mark.parametrize("key", list(ENTRIES), ids=lambda k: f"{k[0]}-{'bf16' if k[1] else 'f16'}")
def test_the_workspace_is_the_twins(knobs, key):
    twin, sym, nptr, _, _ = ENTRIES[key]
    capi.tune("attn_decode_split", 4)
    for shape in ((2, 8, 2, 90, 40, 70, 16, 64, 128), (2, 8, 2, 9, 4, 70, 16, 64, 64)):      # RB = 3 and RB = 1
        B, H, Hkv, T, mq, _, ps, mp, D = shape
        need = getattr(capi.load(), BYTES[key[0]])(B, H, Hkv, T, mq, ps, mp, D, 33)
        assert need == 4 * (T * H) * (D + 1) * 4
        for s, n in ((twin, nptr), (sym, nptr + 1)):
            for nb in (0, 16, need - 1):
                assert _run(s, [P] * n, shape, 33, CAUSAL, ws=(C.c_void_p(256), nb)) == capi.LC_ERR_ARG, (s, nb)
            assert _run(s, [P] * n, shape, 33, CAUSAL, ws=(C.c_void_p(8), need)) == capi.LC_ERR_ARG, s


def test_the_name_calls_report_the_twins_plan_with_tree_in_the_kernel(knobs):
    """<D,RT> for RT = 1, 2, 4, the chunk kernel past 64 rows and the " xS" suffix are the twin's — forced S and the automatic rule"""
    seen = set()
    for D in vl.DS:
        for H, Hkv, mq in ((8, 2, 1), (8, 2, 4), (8, 2, 5), (8, 2, 9), (8, 2, 16), (8, 2, 17), (8, 2, 64), (2, 2, 64), (2, 2, 65), (64, 1, 2)):
            for s in (1, 3, 64):
                capi.tune("attn_decode_split", s)
                for (kind, bf16), (_, _, _, tname, sname) in ENTRIES.items():
                    for B, T in ((1, 130), (6, 174)):
                        for w in (0, 100):
                            shape = (B, H, Hkv, T, mq, 1, 16, vl.NCAP // 16, D)
                            rc, twin = _name(tname, shape, w, CAUSAL)
                            assert rc == capi.LC_OK
                            got = _name(sname, shape, w, CAUSAL)
                            assert got == (capi.LC_OK, twin.replace("_lse_", "_tree_")), (got, twin)
                            assert got[1] == tl.want_name(kind, bf16, H, Hkv, mq, D, s) and got[1].count("tree") == 1, got
                            assert got[1].endswith(f" x{s}") == (s > 1)
                            seen.add(re.sub(r"<.*", "", got[1]))
    assert seen == {f"attn_varlen_{c}paged_{k}tree_{b}kernel" for c in ("", "chunk_") for k in ("", "kv8_") for b in ("", "bf16_")}
    capi.tune("attn_decode_split", 0)
    for cus in (64, 304):
        capi.tune("rule_cus", cus)
        for B, H, Hkv, T, mq, ncap, D in ((64, 32, 8, 64, 1, 4096, 128), (64, 32, 8, 1024, 16, 4096, 128), (1, 8, 2, 40, 1, 32768, 64)):
            for w in (0, 200):
                s = vl.auto_split(B, H, Hkv, T, mq, ncap, w, cus)
                for (kind, bf16), e in ENTRIES.items():
                    got = _name(e[4], (B, H, Hkv, T, mq, 1, 16, ncap // 16, D), w, CAUSAL)
                    assert got == (capi.LC_OK, tl.want_name(kind, bf16, H, Hkv, mq, D, s)), (cus, B, T, mq, w)
    capi.tune("rule_cus", 0)
    capi.tune("attn_decode_split", 1)
    assert capi.attn_varlen_paged_tree_kernel_name(1, 8, 2, 40, 17, 16, 64, 128) == "attn_varlen_chunk_paged_tree_kernel<128>"
    assert capi.attn_varlen_paged_kv8_tree_bf16_kernel_name(1, 8, 2, 40, 5, 16, 64, 64, window=9) == "attn_varlen_paged_kv8_tree_bf16_kernel<64,2>"
    assert capi.attn_varlen_paged_kv8_tree_kernel_name(1, 8, 2, 40, 5, 16, 64, 64) == "attn_varlen_paged_kv8_tree_kernel<64,2>"
    assert capi.attn_varlen_paged_tree_bf16_kernel_name(1, 8, 2, 40, 1, 16, 64, 128) == "attn_varlen_paged_tree_bf16_kernel<128,1>"
    with pytest.raises(capi.LcError):
        capi.attn_varlen_paged_tree_kernel_name(1, 8, 2, 40, 1, 16, 64, 128, causal=False)


def test_the_rope_entries_refuse_what_their_twins_refuse_and_a_null_pos_ids(built):
    shape = (2, 8, 2, 40, 20, 70, 16, 64, 128, 64, 512)            # B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos
    lib = capi.load()

    def run(sym, ptrs, shape=shape, qs=8 * 128, ks=2 * 128, flags=0):
        return getattr(lib, sym)(*ptrs, *shape, qs, ks, flags, None)

    for twin, sym, nptr, tname, sname in ROPES:
        def with_pos(ptrs, pos=P):
            return list(ptrs[:POS_AT]) + [pos] + list(ptrs[POS_AT:])
        nreq = 10                                                   # (k_scale / v_scale: NULL = 1.0)
        for i in range(nreq):
            ptrs = [P] * nptr
            ptrs[i] = None
            assert run(twin, ptrs) == capi.LC_ERR_ARG and run(sym, with_pos(ptrs)) == capi.LC_ERR_ARG, (sym, i)
        bad = shape[:3] + (0,) + shape[4:]
        assert run(sym, with_pos([P] * nptr, None)) == capi.LC_ERR_ARG                      # pos_ids = NULL ...
        assert run(sym, with_pos([P] * nptr, None), shape=bad) == capi.LC_ERR_ARG           # ... in front of the shape
        for kw in (dict(flags=capi.ROPE_PACKED_SRC), dict(flags=8)):
            assert run(twin, [P] * nptr, **kw) == capi.LC_ERR_ARG and run(sym, with_pos([P] * nptr), **kw) == capi.LC_ERR_ARG, kw
        for kw in (dict(shape=bad), dict(qs=8 * 128 + 4), dict(ks=2 * 128 - 8), dict(shape=shape[:9] + (24, 512)), dict(shape=shape[:10] + (0,))):
            assert run(twin, [P] * nptr, **kw) == capi.LC_ERR_SHAPE and run(sym, with_pos([P] * nptr), **kw) == capi.LC_ERR_SHAPE, kw
        hd = shape[:8] + (96, 64, 512)
        assert run(twin, [P] * nptr, shape=hd, qs=8 * 96, ks=2 * 96) == capi.LC_ERR_HEADDIM
        assert run(sym, with_pos([P] * nptr), shape=hd, qs=8 * 96, ks=2 * 96) == capi.LC_ERR_HEADDIM
        # the names
        for D in (64, 128):
            for il in (False, True):
                args = (2, 8, 2, 40, 20, 16, 64, D, 32, 512, 8 * D, 2 * D, capi.ROPE_INTERLEAVED if il else 0)
                rc, t = vl._rc_name(tname, *args)
                assert (rc, vl._rc_name(sname, *args)) == (capi.LC_OK, (capi.LC_OK, t.replace("rope_append_varlen_", "rope_append_varlen_pos_")))
    assert capi.rope_append_varlen_pos_kernel_name(2, 8, 2, 40, 20, 16, 64, 128, 64, 512) == "rope_append_varlen_pos_kernel<128,false>"
    assert capi.rope_append_varlen_pos_kernel_name(2, 8, 2, 40, 20, 16, 64, 64, 64, 512, interleaved=True, kv8=True, bf16=True) == \
        "rope_append_varlen_pos_kv8_bf16_kernel<64,true>"


def test_audit_knows_the_new_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    units = (("tu_attn_varlen_paged_tree", "_paged", ""), ("tu_attn_varlen_paged_kv8_tree", "_paged_kv8", ""),
             ("tu_attn_varlen_paged_tree_bf16", "_paged", "_bf16"), ("tu_attn_varlen_paged_kv8_tree_bf16", "_paged_kv8", "_bf16"))
    for unit, mid, bf in units:
        rep = json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text())
        names = " ".join(r["kernel"] for r in rep)
        for d in (64, 128):
            assert f"attn_varlen_chunk{mid}_tree{bf}_kernelILi{d}EE" in names, (unit, d)
            for rt in (1, 2, 4):
                assert f"attn_varlen{mid}_tree{bf}_kernelILi{d}ELi{rt}EE" in names, (unit, d, rt)
        assert len(rep) == 8, unit                                      # no twin kernel and no combine kernel is instantiated in a tree unit
        for r in rep:
            assert "_tree" in r["kernel"] and ("bf16" in r["kernel"]) == bool(bf), r["kernel"]
    rep = json.loads((obj / build.AUDIT_OWN_REPORT["tu_rope_append_varlen_pos"]).read_text())
    names = " ".join(r["kernel"] for r in rep)
    for stem in ("rope_append_varlen_pos_kernel", "rope_append_varlen_pos_kv8_kernel", "rope_append_varlen_pos_bf16_kernel",
                 "rope_append_varlen_pos_kv8_bf16_kernel"):
        for d in (64, 128):
            for il in (0, 1):
                assert f"{stem}ILi{d}ELb{il}EE" in names, (stem, d, il)
    assert len(rep) == 16
    for unit in [u[0] for u in units] + ["tu_rope_append_varlen_pos"]:
        for r in json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text()):
            assert r["scratch"] == 0 and not r["violations"], r
            assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]                       # plain HIP: listed for rule R2 only
            assert r["asm_loads"] == 0
            assert r["vgpr"] <= 512, r                                                       # (.vgpr_count: arch + accumulation registers)
    # the twins' units keep their kernels and know nothing of the new ones
    for unit, n in (("tu_attn_varlen_paged_lse", 10), ("tu_attn_varlen_paged_kv8_lse", 8), ("tu_attn_varlen_paged_lse_bf16", 10),
                    ("tu_attn_varlen_paged_kv8_lse_bf16", 8), ("tu_rope_append_varlen", 8), ("tu_rope_append_varlen_bf16", 8)):
        text = (obj / build.AUDIT_OWN_REPORT[unit]).read_text()
        assert "tree" not in text and "_pos_" not in text and len(json.loads(text)) == n, unit


# ------------------------------------------------------------------------------------------------------------------------------------
# the host helpers

def test_tree_mask_and_tree_positions_agree_with_the_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(12):
        sizes = [1, 64, 5, None, 17, 2, None, 33][: 3 + trial % 6]
        rng.shuffle(sizes)
        parents, nqs = [], []
        for s in sizes:
            if s is None:
                parents.append(None)
                nqs.append(int(rng.integers(0, 80)))                 # an ordinary sequence of any Nq_b, 0 and > 64 included
            else:
                parents.append(tl.random_parents(s, rng, chain=(0.0, 0.5, 0.9)[trial % 3]))
                nqs.append(s)
        cu = vl.cu_of(nqs)
        lens = [int(n + rng.integers(0, 500)) for n in nqs]
        got = capi.tree_mask(parents, cu)
        assert got.dtype == torch.int64 and tuple(got.shape) == (cu[-1],) and got.device.type == "cpu"
        assert got.tolist() == [tl.signed(w) for w in tl.brute_mask(parents, cu)], trial
        pos = capi.tree_positions(parents, torch.tensor(cu, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32))
        assert pos.dtype == torch.int32 and pos.tolist() == tl.brute_positions(parents, cu, lens), trial
        for b, par in enumerate(parents):                            # None: all ones, and the slot
            if par is None:
                assert (got[cu[b]:cu[b + 1]] == -1).all()
                assert pos[cu[b]:cu[b + 1]].tolist() == list(range(lens[b] - nqs[b], lens[b]))


def test_a_chain_is_all_ones_and_the_limits_of_a_tree():
    for n in (1, 2, 17, 64):
        chain = list(range(-1, n - 1))
        assert (capi.tree_mask([chain], [0, n]) == -1).all(), n
        assert capi.tree_positions([chain], [0, n], [n + 9]).tolist() == list(range(9, n + 9))
    # a star: every token hangs off the prefix — its own bit and the prefix bits, depth 0 for all
    star = capi.tree_mask([[-1] * 64], [0, 64]).tolist()
    assert star == [tl.signed(1 | ((tl.M64 << (i + 1)) & tl.M64)) for i in range(64)] and star[63] == 1 and star[0] == -1
    assert capi.tree_positions([[-1] * 64], [0, 64], [100]).tolist() == [36] * 64
    # a one-token tree is an ordinary decoding token
    assert capi.tree_mask([[-1]], [0, 1]).tolist() == [-1]
    with pytest.raises(ValueError, match="65 tokens"):
        capi.tree_mask([list(range(-1, 64))], [0, 65])
    with pytest.raises(ValueError, match="65 tokens"):
        capi.tree_positions([list(range(-1, 64))], [0, 65], [70])
    assert (capi.tree_mask([None], [0, 65]) == -1).all()            # (an ordinary sequence has no such limit)
    for bad in ([0], [-1, 1], [-1, 2, 0], [-2]):
        with pytest.raises(ValueError, match="parents"):
            capi.tree_mask([bad], [0, len(bad)])
    with pytest.raises(ValueError, match="parents for"):
        capi.tree_mask([[-1, 0]], [0, 3])
    with pytest.raises(ValueError, match="cu_q"):
        capi.tree_mask([None, None], [0, 3])


def test_capi_wrappers_refuse_wrong_dtypes(built):
    T, H, Hkv, D = 12, 8, 2, 64
    g = torch.Generator().manual_seed(1)
    _, k, v = dl.decode_inputs(3, H, Hkv, 1, 128, D, seed=1)
    lens = torch.tensor([100, 17, 5], dtype=torch.int32)
    cu = torch.tensor([0, 5, 5, 12], dtype=torch.int32)
    mask = capi.tree_mask([[-1, 0, 0, 1, 3], None, None], cu)
    pos = capi.tree_positions([[-1, 0, 0, 1, 3], None, None], cu, lens)
    cs = capi.rope_table(128, 32)
    for el, word in ((torch.half, "float16"), (BF, "bfloat16")):
        bf16 = el == BF
        q = torch.randn(T, H, D, generator=g).to(el)
        o = torch.empty_like(q)
        kp, vp, table = dl.paginate(k.to(el), v.to(el), (100, 17, 5), 16, seed=2)
        kp8, vp8 = (x.view(torch.uint8)[..., :64].contiguous() for x in (kp, vp))
        for kind, pools in (("paged", (kp, vp)), ("kv8", (kp8, vp8))):
            fn = tl.fn_of(kind, bf16)
            with pytest.raises(TypeError, match=word):
                fn(q.float(), *pools, o, cu, table, lens, 7, mask)
            for wrong in (mask.int(), mask.double()):
                with pytest.raises(TypeError, match="tree_mask must be int64"):
                    fn(q, *pools, o, cu, table, lens, 7, wrong)
            for wrong in (mask[:T - 1], mask.view(T, 1), torch.zeros(2 * T, dtype=torch.int64)[::2]):
                with pytest.raises(RuntimeError, match="Tensor size mismatch"):
                    fn(q, *pools, o, cu, table, lens, 7, wrong)
            with pytest.raises(RuntimeError, match="MI355X"):       # everything checked: only the device is missing
                fn(q, *pools, o, cu, table, lens, 7, mask, window=3, sinks=torch.zeros(8))
            rope = tl.rope_fn(kind == "kv8", bf16, True)
            kn, vn = (torch.randn(T, Hkv, D, generator=g).to(el) for _ in range(2))
            with pytest.raises(TypeError, match="pos_ids must be int32"):
                rope(q, kn, vn, *pools, cs, cu, pos.long(), table, lens, 7)
            with pytest.raises(RuntimeError, match="Tensor size mismatch"):
                rope(q, kn, vn, *pools, cs, cu, pos[:T - 1], table, lens, 7)
            with pytest.raises(TypeError, match=word):
                rope(q.float(), kn, vn, *pools, cs, cu, pos, table, lens, 7)
            with pytest.raises(RuntimeError, match="MI355X"):
                rope(q, kn, vn, *pools, cs, cu, pos, table, lens, 7)


# ------------------------------------------------------------------------------------------------------------------------------------
# what the GPU module's reference rests on

def test_the_definition_by_parents_is_the_rule_of_the_mask_words():
    """tree_lib.visible (parents, never the words) against the rule of include/lc_abi.h applied to capi.tree_mask's words, key by key"""
    rng = np.random.default_rng(5)
    for n, L, window in ((1, 40, 0), (5, 5, 0), (16, 300, 0), (17, 90, 10), (64, 64, 0), (64, 700, 40), (64, 1000, 100), (33, 20, 0)):
        par = tl.random_parents(n, rng, chain=0.5)
        ws = tl.brute_mask([par], [0, n])
        for i in range(n):
            p = min(L, tl.NCAP) - n + i
            j = np.arange(tl.NCAP)
            d = p - j
            rule = (j <= p) & ((window == 0) | (j > p - window))
            bit = np.array([(ws[i] >> int(x)) & 1 if 0 <= x < 64 else 1 for x in d], bool)
            assert (tl.visible(par, L, n, i, window) == (rule & bit)).all(), (n, L, window, i)
        assert (tl.visible(None, L, n, n - 1, window).sum()) == (min(window, max(min(L, tl.NCAP), 0)) if window else min(L, tl.NCAP))


def test_tree64_without_a_tree_is_the_ragged_reference():
    D = 64
    q, k, v = sl.inputs(2, 9, D, seed=4, bf16=False, ncap=64)
    cu, lens = [0, 2, 9], (40, 7)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.5, -0.5, 0.25, 3.0])
    for parents in ([None, None], [[-1, 0], list(range(-1, 6))]):   # no tree, and chains: the same visibility
        out, lse, A, nvis = tl.tree64(q, k.double(), v.double(), cu, lens, 7, parents, window=5, sinks=sinks)
        want_o, nv = vl.ragged64(q, k.double(), v.double(), cu, lens, 7, True, window=5, sinks=sinks)
        want_l, want_a, nv2 = sl.lse64(q, k.double(), cu, lens, 7, True, window=5, sinks=sinks)
        assert (nvis == nv).all() and (nvis == nv2).all()
        assert np.allclose(out, want_o, rtol=1e-12, atol=1e-14) and np.allclose(lse, want_l, rtol=1e-13, atol=1e-13) and np.allclose(A, want_a)
    # a fork: token 2 hangs off token 0 and does not see token 1 — one key fewer, by hand
    out, lse, _, nvis = tl.tree64(q, k.double(), v.double(), [0, 3, 9], (40, 7), 7, [[-1, 0, 0], None])
    assert nvis[:3].tolist() == [38, 39, 39]
    keys = [j for j in range(40) if j != 38]
    s = (k[0, 0, keys].double() @ q[2, 1].double()) / 8.0
    assert abs(lse[2, 1] - float(torch.logsumexp(s, 0))) < 1e-12
    assert np.allclose(out[2, 1], (torch.softmax(s, 0) @ v[0, 0, keys].double()).numpy(), rtol=1e-12, atol=1e-14)
