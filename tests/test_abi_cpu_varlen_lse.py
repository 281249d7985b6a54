"""CPU tests of the boundary of the log-sum-exp ragged entries and of the state merge (lc_attn_varlen_paged_lse_f16 / _lse_kv8 / _lse_bf16 /
_lse_kv8_bf16, their four name calls, lc_attn_merge_states_f16 / _bf16; no call here reaches a device): header,
capi.SYMBOLS and exports agree on the ten symbols; every bad-argument case of tests/test_abi_cpu_varlen.py's tables gives an LSE entry the
status of its twin, and lse = NULL is LC_ERR_ARG; the merge entry's argument checks; the name calls report the twin's plan with `_lse` in the
kernel; the Python wrappers refuse wrong dtypes; the five new audit reports; and the references of tests/lse_lib.py that the GPU module's
checks rest on — merge64 against a direct float64 softmax over the concatenated keys, the fp32 emulation under the derived bound."""
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
from tests import varlen_lib as vl

P = C.c_void_p(16)
CAUSAL = capi.ATTN_CAUSAL
BF = torch.bfloat16
# (kind, bf16) -> twin run entry, LSE run entry, pointers in front of the twin's shape, twin name call, LSE name call
ENTRIES = {
    ("paged", False): ("lc_attn_varlen_paged_f16", "lc_attn_varlen_paged_lse_f16", 7, "lc_attn_varlen_paged_kernel_name",
                       "lc_attn_varlen_paged_lse_kernel_name"),
    ("kv8", False): ("lc_attn_varlen_paged_kv8", "lc_attn_varlen_paged_lse_kv8", 9, "lc_attn_varlen_paged_kv8_kernel_name",
                     "lc_attn_varlen_paged_lse_kv8_kernel_name"),
    ("paged", True): ("lc_attn_varlen_paged_bf16", "lc_attn_varlen_paged_lse_bf16", 7, "lc_attn_varlen_paged_bf16_kernel_name",
                      "lc_attn_varlen_paged_lse_bf16_kernel_name"),
    ("kv8", True): ("lc_attn_varlen_paged_kv8_bf16", "lc_attn_varlen_paged_lse_kv8_bf16", 9, "lc_attn_varlen_paged_kv8_bf16_kernel_name",
                    "lc_attn_varlen_paged_lse_kv8_bf16_kernel_name"),
}
MERGE = ("lc_attn_merge_states_f16", "lc_attn_merge_states_bf16")
BYTES = {"paged": "lc_attn_varlen_paged_workspace_bytes", "kv8": "lc_attn_varlen_paged_kv8_workspace_bytes"}
OK = (2, 8, 2, 40, 20, 70, 16, 64, 128)                        # B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D
BAD = (2, 8, 3, 40, 20, 70, 16, 64, 256)
LSE_AT = 4                                                      # the position of `lse`: right behind O


@pytest.fixture
def knobs(built):
    yield from dl.reset_knobs()


def _with_lse(ptrs):
    """the twin's pointers with a valid lse pointer behind O"""
    return list(ptrs[:LSE_AT]) + [P] + list(ptrs[LSE_AT:])


def _run(sym, ptrs, shape, window, flags, sinks=None, ws=(None, 0)):
    """status of a run call on dummy pointers (only ever used on calls a check refuses: nothing reaches a device)"""
    return getattr(capi.load(), sym)(*ptrs, *shape, window, sinks, flags, *ws, None)


def _name(sym, shape, window, flags):
    B, H, Hkv, T, max_nq, _, ps, mp, D = shape
    return vl._rc_name(sym, B, H, Hkv, T, max_nq, ps, mp, D, window, flags)


def _merge(sym, ptrs=None, B=2, T=40, H=8, D=128, cu=P):
    ptrs = [P] * 6 if ptrs is None else ptrs
    return getattr(capi.load(), sym)(*ptrs, cu, B, T, H, D, None)


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
            assert hasattr(lib, s), s
            assert s in capi.SYMBOLS, s
        # the twin's parameter list with `float* lse` right behind O, in the header and in the ctypes signature
        want = params(twin)
        assert want[3] == "void* O"
        assert params(sym) == want[:LSE_AT] + ["float* lse"] + want[LSE_AT:], sym
        res, args = capi.SYMBOLS[twin]
        assert capi.SYMBOLS[sym] == (res, args[:LSE_AT] + [C.c_void_p] + args[LSE_AT:]), sym
        assert params(sname) == params(tname) and capi.SYMBOLS[sname] == capi.SYMBOLS[tname], sname
        new += [sym, sname]
    for s in MERGE:
        assert hasattr(lib, s) and s in capi.SYMBOLS, s
        assert params(s) == ["const void* Oa", "const float* lse_a", "const void* Ob", "const float* lse_b", "void* Oout", "float* lse_out",
                             "const int* cu_q", "int B", "int T", "int H", "int D", "void* stream"]
        assert capi.SYMBOLS[s] == (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p])
        new.append(s)
    assert len(set(new)) == 10
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays
    for s in ("lc_attn_varlen_paged_lse_workspace_bytes", "lc_attn_varlen_paged_lse_kv8_workspace_bytes",      # the twins' queries serve the LSE entries
              "lc_attn_decode_paged_lse_f16", "lc_attn_local_paged_lse_f16", "lc_attn_fwd_lse_f16"):
        assert not hasattr(lib, s), s
        assert s not in capi.SYMBOLS


@pytest.mark.parametrize("key", list(ENTRIES), ids=lambda k: f"{k[0]}-{'bf16' if k[1] else 'f16'}")
def test_every_bad_argument_gets_the_status_of_the_twin(built, key):
    """tests/test_abi_cpu_varlen.py::test_statuses_and_their_order, case for case, on the twin and on the LSE entry"""
    twin, sym, nptr, tname, sname = ENTRIES[key]
    seen = []

    def both(want, shape, w, flags, ptrs=None, **kw):
        ptrs = [P] * nptr if ptrs is None else ptrs
        got = [_run(twin, ptrs, shape, w, flags, **kw), _run(sym, _with_lse(ptrs), shape, w, flags, **kw)]
        assert got == [want, want], (shape, w, flags, got)
        seen.append(want)

    def both_names(want, shape, w, flags):
        got = [_name(s, shape, w, flags)[0] for s in (tname, sname)]
        assert got == [want, want], (shape, w, flags, got)

    for w, flags in ((-1, CAUSAL), (5, 0), (0, 4), (5, capi.ATTN_V_TRANSPOSED)):
        both(capi.LC_ERR_ARG, OK, w, flags)
        both(capi.LC_ERR_ARG, BAD, w, flags)
        both_names(capi.LC_ERR_ARG, BAD, w, flags)
    for i in range(7):                                              # a NULL pointer — cu_q among them — in front of the shape
        ptrs = [P] * nptr
        ptrs[i] = None
        both(capi.LC_ERR_ARG, BAD, 7, CAUSAL, ptrs=ptrs)
    null_lse = [P] * (nptr + 1)
    null_lse[LSE_AT] = None                                         # ... and lse = NULL, in front of the shape checks too
    assert _run(sym, null_lse, BAD, 7, CAUSAL) == capi.LC_ERR_ARG
    assert _run(sym, null_lse, OK, 0, 0) == capi.LC_ERR_ARG
    mis = [P] * nptr
    mis[0] = C.c_void_p(8)
    for T, mq in ((0, 1), (-3, 1), (40, 0), (40, -1), (40, 41), (1, 2)):
        bad = (2, 8, 2, T, mq, 70, 16, 64, 96)
        both(capi.LC_ERR_SHAPE, bad, 0, 0)
        both(capi.LC_ERR_SHAPE, bad, 0, 0, ptrs=mis)
        both_names(capi.LC_ERR_SHAPE, bad, 0, 0)
    both(capi.LC_ERR_SHAPE, BAD, 0, 0)
    both(capi.LC_ERR_SHAPE, (2, 8, 2, 40, 20, 70, 24, 64, 128), 0, 0)             # a page size that is no power of two
    both(capi.LC_ERR_SHAPE, (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, 0, ptrs=mis)     # alignment in front of the head dim
    both(capi.LC_ERR_HEADDIM, (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, 0)
    both_names(capi.LC_ERR_HEADDIM, (2, 8, 2, 40, 40, 70, 16, 64, 96), 7, CAUSAL)
    both_names(capi.LC_OK, (2, 8, 2, 40, 40, 70, 16, 64, 64), 7, CAUSAL)
    for s in (tname, sname):
        fn = getattr(capi.load(), s)
        assert fn(2, 8, 2, 40, 20, 16, 64, 128, 0, 0, None, 128) == capi.LC_ERR_ARG
        assert fn(2, 8, 2, 40, 20, 16, 64, 128, 0, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG
    assert {capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM} == set(seen)


@pytest.mark.parametrize("key", list(ENTRIES), ids=lambda k: f"{k[0]}-{'bf16' if k[1] else 'f16'}")
def test_a_small_or_misaligned_workspace_is_refused_as_the_twin_refuses_it(knobs, key):
    """the existing workspace queries serve the LSE entries: an LSE call needs the twin's bytes"""
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


@pytest.mark.parametrize("sym", MERGE)
def test_merge_argument_checks_and_their_order(built, sym):
    for i in range(6):                                              # every pointer but cu_q
        ptrs = [P] * 6
        ptrs[i] = None
        assert _merge(sym, ptrs) == capi.LC_ERR_ARG, i
        assert _merge(sym, ptrs, T=0, D=96) == capi.LC_ERR_ARG, i   # in front of the shape and the head dim
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-5), dict(H=0), dict(D=0), dict(D=-64), dict(T=1 << 20, H=1 << 12)):
        assert _merge(sym, **kw) == capi.LC_ERR_SHAPE, kw
        assert _merge(sym, cu=None, **kw) == capi.LC_ERR_SHAPE, kw
    assert _merge(sym, T=0, D=96) == capi.LC_ERR_SHAPE              # the shape in front of the head dim
    for i in (0, 2, 4):                                             # an O pointer off 16 bytes, in front of the head dim
        ptrs = [P] * 6
        ptrs[i] = C.c_void_p(8)
        assert _merge(sym, ptrs) == capi.LC_ERR_SHAPE, i
        assert _merge(sym, ptrs, D=96) == capi.LC_ERR_SHAPE, i
    for D in (32, 96, 256, 512):
        assert _merge(sym, D=D) == capi.LC_ERR_HEADDIM, D
        assert _merge(sym, D=D, cu=None) == capi.LC_ERR_HEADDIM, D


def test_the_name_calls_report_the_twins_plan_with_lse_in_the_kernel(knobs):
    """<D,RT>, the chunk kernel past 64 rows and the " xS" suffix are the twin's — forced S and the automatic rule at two CU counts"""
    seen = set()
    for D in vl.DS:
        for H, Hkv, mq in ((8, 2, 1), (8, 2, 4), (8, 2, 5), (8, 2, 9), (8, 2, 16), (8, 2, 17), (8, 2, 130), (2, 2, 64), (2, 2, 65), (64, 1, 2)):
            for s in (1, 3, 64):
                capi.tune("attn_decode_split", s)
                for (kind, bf16), (_, _, _, tname, sname) in ENTRIES.items():
                    for B, T in ((1, 130), (6, 174)):
                        for w, flags in ((0, 0), (0, CAUSAL), (100, CAUSAL)):
                            shape = (B, H, Hkv, T, mq, 1, 16, vl.NCAP // 16, D)
                            rc, twin = _name(tname, shape, w, flags)
                            assert rc == capi.LC_OK
                            got = _name(sname, shape, w, flags)
                            assert got == (capi.LC_OK, sl.lse_name(twin)) and got[1] == sl.want_name(kind, bf16, H, Hkv, mq, D, s), (got, twin)
                            assert got[1].count("_lse") == 1 and got[1].replace("_lse", "") == twin
                            seen.add(re.sub(r"<.*", "", got[1]))
    assert seen == {f"attn_varlen_{c}paged_{k}lse_{b}kernel" for c in ("", "chunk_") for k in ("", "kv8_") for b in ("", "bf16_")}
    capi.tune("attn_decode_split", 0)
    for cus in (64, 304):
        capi.tune("rule_cus", cus)
        for B, H, Hkv, T, mq, ncap, D in ((64, 32, 8, 64, 1, 4096, 128), (64, 32, 8, 575, 512, 4096, 128), (1, 8, 2, 40, 1, 32768, 64)):
            for w in (0, 200):
                s = vl.auto_split(B, H, Hkv, T, mq, ncap, w, cus)
                for (kind, bf16), e in ENTRIES.items():
                    got = _name(e[4], (B, H, Hkv, T, mq, 1, 16, ncap // 16, D), w, CAUSAL)
                    assert got == (capi.LC_OK, sl.want_name(kind, bf16, H, Hkv, mq, D, s)), (cus, B, T, mq, w)
    capi.tune("rule_cus", 0)
    capi.tune("attn_decode_split", 1)
    assert capi.attn_varlen_paged_lse_kernel_name(1, 8, 2, 40, 17, 16, 64, 128) == "attn_varlen_chunk_paged_lse_kernel<128>"
    assert capi.attn_varlen_paged_lse_kernel_name(1, 8, 2, 40, 5, 16, 64, 64, causal=True, window=9, kv8=True, bf16=True) == \
        "attn_varlen_paged_kv8_lse_bf16_kernel<64,2>"
    assert capi.attn_varlen_paged_lse_kernel_name(1, 8, 2, 40, 5, 16, 64, 64, kv8=True) == "attn_varlen_paged_kv8_lse_kernel<64,2>"
    assert capi.attn_varlen_paged_lse_kernel_name(1, 8, 2, 40, 1, 16, 64, 128, bf16=True) == "attn_varlen_paged_lse_bf16_kernel<128,1>"


def test_audit_knows_the_new_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    units = (("tu_attn_varlen_paged_lse", "_paged", "", 2), ("tu_attn_varlen_paged_kv8_lse", "_paged_kv8", "", 0),
             ("tu_attn_varlen_paged_lse_bf16", "_paged", "_bf16", 2), ("tu_attn_varlen_paged_kv8_lse_bf16", "_paged_kv8", "_bf16", 0))
    for unit, mid, bf, extra in units:
        rep = json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text())
        names = " ".join(r["kernel"] for r in rep)
        for d in (64, 128):
            assert f"attn_varlen_chunk{mid}_lse{bf}_kernelILi{d}EE" in names, (unit, d)
            for rt in (1, 2, 4):
                assert f"attn_varlen{mid}_lse{bf}_kernelILi{d}ELi{rt}EE" in names, (unit, d, rt)
            assert (f"attn_varlen_combine_lse{bf}_kernelILi{d}EE" in names) == (extra == 2)
        assert len(rep) == 8 + extra, unit                              # no twin kernel is instantiated a second time in an LSE unit
        for r in rep:
            assert "_lse" in r["kernel"] and ("bf16" in r["kernel"]) == bool(bf), r["kernel"]
    rep = json.loads((obj / build.AUDIT_OWN_REPORT["tu_attn_merge"]).read_text())
    names = " ".join(r["kernel"] for r in rep)
    for d in (64, 128):
        assert f"attn_merge_states_kernelILi{d}EE" in names and f"attn_merge_states_bf16_kernelILi{d}EE" in names
    assert len(rep) == 4
    for unit in [u[0] for u in units] + ["tu_attn_merge"]:
        for r in json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text()):
            assert r["scratch"] == 0 and not r["violations"], r
            assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]                       # plain HIP: listed for rule R2 only
            assert r["asm_loads"] == 0
    # the twins' units keep their kernels and know nothing of the new ones
    for unit, n in (("tu_attn_varlen_paged", 10), ("tu_attn_varlen_paged_kv8", 8), ("tu_attn_varlen_paged_bf16", 10),
                    ("tu_attn_varlen_paged_kv8_bf16", 8)):
        text = (obj / build.AUDIT_OWN_REPORT[unit]).read_text()
        assert "lse" not in text and "merge" not in text and len(json.loads(text)) == n, unit


def test_capi_wrappers_refuse_wrong_dtypes(built):
    T, H, Hkv, D = 12, 8, 2, 64
    g = torch.Generator().manual_seed(1)
    _, k, v = dl.decode_inputs(3, H, Hkv, 1, 128, D, seed=1)
    lens = torch.tensor([100, 17, 5], dtype=torch.int32)
    cu = torch.tensor([0, 5, 5, 12], dtype=torch.int32)
    for el, other, word in ((torch.half, BF, "float16"), (BF, torch.half, "bfloat16")):
        q = torch.randn(T, H, D, generator=g).to(el)
        o = torch.empty_like(q)
        kp, vp, table = dl.paginate(k.to(el), v.to(el), (100, 17, 5), 16, seed=2)
        kp8, vp8 = (x.view(torch.uint8)[..., :64].contiguous() for x in (kp, vp))
        f16, f8 = ((capi.attn_varlen_paged_lse, capi.attn_varlen_paged_kv8_lse) if el == torch.half
                   else (capi.attn_varlen_paged_lse_bf16, capi.attn_varlen_paged_kv8_lse_bf16))
        calls = (lambda **kw: f16(kw.pop("q", q), kw.pop("kp", kp), kw.pop("vp", vp), kw.pop("o", o), cu, table, lens, kw.pop("max_nq", 7),
                                  causal=True, **kw),
                 lambda **kw: f8(kw.pop("q", q), kp8, vp8, kw.pop("o", o), cu, table, lens, kw.pop("max_nq", 7), causal=True, **kw))
        for call in calls:
            for wrong in (other, torch.float32):
                with pytest.raises(TypeError, match=word):
                    call(q=q.to(wrong))
                with pytest.raises(TypeError, match=word):
                    call(o=o.to(wrong))
            with pytest.raises(TypeError, match="lse must be float32"):
                call(lse=torch.zeros(T, H, dtype=torch.float64))
            with pytest.raises(TypeError, match="lse must be float32"):
                call(lse=torch.zeros(T, H, dtype=el))
            for bad in (torch.zeros(T, H + 1), torch.zeros(T * H), torch.zeros(H, T).t()):
                with pytest.raises(RuntimeError, match="Tensor size mismatch"):
                    call(lse=bad)
            with pytest.raises(ValueError, match="max_nq"):
                call(max_nq=T + 1)
            with pytest.raises(RuntimeError, match="MI355X"):           # everything checked: only the device is missing
                call(window=3, sinks=torch.zeros(8), lse=torch.zeros(T, H))
            with pytest.raises(RuntimeError, match="MI355X"):
                call()                                                  # lse = None: allocated
        with pytest.raises(TypeError, match=word):
            calls[0](kp=kp.to(other), vp=vp.to(other))
        with pytest.raises(TypeError, match=word):
            f16(q, kp8, vp8, o, cu, table, lens, 7)
        with pytest.raises(TypeError, match="float8_e4m3fn or uint8"):
            f8(q, kp, vp, o, cu, table, lens, 7)
        # the merge: one 16-bit dtype for the three O tensors, float32 lse, float32 O refused
        la = torch.zeros(T, H)
        with pytest.raises(TypeError, match="float16 or bfloat16"):
            capi.attn_merge_states(q.float(), la, o.float(), la)
        with pytest.raises(TypeError, match="share one 16-bit dtype"):
            capi.attn_merge_states(q, la, o.to(other), la)
        with pytest.raises(TypeError, match="share one 16-bit dtype"):
            capi.attn_merge_states(q, la, o, la, out=torch.empty_like(q, dtype=torch.float32))
        with pytest.raises(TypeError, match="lse must be float32"):
            capi.attn_merge_states(q, la.double(), o, la)
        with pytest.raises(TypeError, match="cu_q must be int32"):
            capi.attn_merge_states(q, la, o, la, cu_q=cu.long())
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi.attn_merge_states(q, la, o[:T - 1], la)
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi.attn_merge_states(q, la[:, :4], o, la)
        with pytest.raises(RuntimeError, match="MI355X"):
            capi.attn_merge_states(q, la, o, la, out=q, lse_out=la, cu_q=cu)
        # the cascade wrapper: the caller's scratch, the element type of q
        scratch = (torch.empty_like(q), torch.empty(T, H), torch.empty(T, H))
        cg, pt, pl = torch.tensor([0, 12], dtype=torch.int32), table[:1], lens[:1]
        with pytest.raises(TypeError, match="scratch"):
            capi.attn_cascade_paged(q, kp, vp, o, cg, pt, pl, cu, table, lens, 12, 7, scratch=(scratch[0],))
        with pytest.raises(TypeError, match="float16 or bfloat16"):
            capi.attn_cascade_paged(q.float(), kp, vp, o, cg, pt, pl, cu, table, lens, 12, 7, scratch=scratch)
        with pytest.raises(TypeError, match=word):
            capi.attn_cascade_paged(q, kp.to(other), vp.to(other), o, cg, pt, pl, cu, table, lens, 12, 7, scratch=scratch)
        for pools in ((kp, vp), (kp8, vp8)):
            with pytest.raises(RuntimeError, match="MI355X"):
                capi.attn_cascade_paged(q, *pools, o, cg, pt, pl, cu, table, lens, 12, 7, scratch=scratch, sinks=torch.zeros(8))


# ------------------------------------------------------------------------------------------------------------------------------------
# what the GPU module's checks rest on

def test_merge64_is_the_softmax_over_the_concatenated_keys():
    rng = np.random.default_rng(3)
    D = 64
    for na, nb in ((5, 9), (1, 1), (40, 3), (0, 7), (6, 0), (0, 0)):
        q = rng.standard_normal(D) * 2
        k, v = rng.standard_normal((na + nb, D)), rng.standard_normal((na + nb, D))
        oa, la = sl.attend64(q, k[:na], v[:na])
        ob, lb = sl.attend64(q, k[na:], v[na:])
        o, l = sl.merge64(oa, la, ob, lb)
        want_o, want_l = sl.attend64(q, k, v)
        assert np.allclose(o, want_o, rtol=1e-13, atol=1e-15), (na, nb)
        assert l == want_l or abs(l - want_l) <= 1e-13 * max(1.0, abs(want_l)), (na, nb, l, want_l)
    # vectorised over rows, pass-through and the empty state
    oa, ob = rng.standard_normal((4, D)), rng.standard_normal((4, D))
    la, lb = np.array([1.0, -np.inf, -np.inf, 3.0]), np.array([-np.inf, 2.0, -np.inf, 3.0])
    o, l = sl.merge64(oa, la, ob, lb)
    assert (o[0] == oa[0]).all() and l[0] == 1.0 and (o[1] == ob[1]).all() and l[1] == 2.0
    assert (o[2] == 0).all() and l[2] == -np.inf
    assert np.allclose(o[3], (oa[3] + ob[3]) / 2, rtol=1e-15) and abs(l[3] - (3.0 + np.log(2.0))) < 1e-15


def test_lse64_is_the_log_of_ragged64s_denominator_and_the_names_follow_the_twins():
    D = 64
    q, k, v = sl.inputs(2, 9, D, seed=4, bf16=False, ncap=64)
    cu, lens = [0, 2, 9], (40, 7)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.5, -0.5, 0.25, 3.0])
    lse, A, nvis = sl.lse64(q, k.double(), cu, lens, 7, True, window=5, sinks=sinks)
    assert nvis.tolist() == [5, 5, 1, 2, 3, 4, 5, 5, 5]
    # one row by hand: token 2 = query 0 of sequence 1, which sees key 0 only
    s = float((q[2, 3].double() * k[1, 0, 0].double()).sum()) / 8.0
    assert abs(lse[2, 3] - np.log(np.exp(s) + np.exp(0.0))) < 1e-12
    assert abs(A[2, 3] - float((q[2, 3].double() * k[1, 0, 0].double()).abs().sum()) / 8.0) < 1e-12
    lse0, _, nv0 = sl.lse64(q, k.double(), [0, 2, 9], (0, 3), 7, True)
    assert (lse0[:2] == -np.inf).all() and nv0[:2].tolist() == [0, 0]           # no key, no sink
    assert np.isinf(lse0[2:6]).all() and np.isfinite(lse0[6:]).all()             # sequence 1: queries 0 .. 3 sit in front of key 0
    assert sl.lse_name("attn_varlen_paged_kernel<128,1> x3") == "attn_varlen_paged_lse_kernel<128,1> x3"
    assert sl.lse_name("attn_varlen_chunk_paged_kv8_bf16_kernel<64>") == "attn_varlen_chunk_paged_kv8_lse_bf16_kernel<64>"


@pytest.mark.parametrize("D", vl.DS)
def test_the_fp32_emulation_of_the_kernel_stays_under_the_derived_bound(D):
    """the bound of the GPU module's random-input test is derived from the arithmetic (lse_lib.lse_bound), not tuned: on THAT test's inputs — the
    same caches, tokens, window and sinks; here the first, a middle and the last token of every sequence — an fp32 restatement of the kernel's
    arithmetic with the worst summation order, sequential, must stay under it, with room"""
    cu = vl.cu_of(sl.NQS)
    only = sorted({t for b in range(len(sl.NQS)) for t in (cu[b], (cu[b] + cu[b + 1]) // 2, cu[b + 1] - 1)})
    worst = 0.0
    for bf16 in (False, True):
        c, q = sl.cache(D, bf16, sl.LENS), sl.tokens(D, bf16, sl.T_RAGGED)
        for kind in sl.KINDS:
            klog, _ = c.logical(kind)
            kmul, ksc = (dl.OCP[c.k8.long()], c.ks.numpy()) if kind == "kv8" else (c.k, None)      # what the MFMA multiplies
            for window, sk in ((0, None), (45, sl.SINKS)):
                want, A, nvis = sl.lse64(q, klog, cu, sl.LENS, sl.MAX_NQ, True, window=window, sinks=sk)
                got = sl.emulate_lse32(q, kmul, cu, sl.LENS, sl.MAX_NQ, True, window=window, sinks=sk, k_scale=ksc, only=only)
                bound = sl.lse_bound(A, want, nvis[:, None], D, float(sl.SINKS.abs().max()) if sk is not None else 0.0)
                ratio = (np.abs(got - want) / bound)[only]
                assert np.isfinite(ratio).all() and (ratio < 0.5).all(), (D, bf16, kind, window, float(ratio.max()))
                worst = max(worst, float(ratio.max()))
    print(f"fp32 emulation, D = {D}: worst |err| / bound {worst:.3f}")


def test_the_merge_bound_holds_for_an_fp32_restatement_of_the_merge():
    rng = np.random.default_rng(9)
    la = (rng.standard_normal(20000) * 6).astype(np.float32)
    lb = (la + rng.standard_normal(20000).astype(np.float32) * np.float32(8)).astype(np.float32)
    m = np.maximum(la, lb)
    wa = np.exp2(((la - m).astype(np.float32) * sl.LOG2E_32).astype(np.float32)).astype(np.float32)
    wb = np.exp2(((lb - m).astype(np.float32) * sl.LOG2E_32).astype(np.float32)).astype(np.float32)
    got = (m + (np.log2((wa + wb).astype(np.float32)).astype(np.float32) * sl.LN2_32).astype(np.float32)).astype(np.float32)
    _, want = sl.merge64(np.zeros((20000, 1)), la, np.zeros((20000, 1)), lb)
    ratio = np.abs(got.astype(np.float64) - want) / sl.merge_lse_bound(want)
    assert (ratio <= 1.0).all(), float(ratio.max())
    assert sl.ulp32(1.0) == 2.0 ** -23 and sl.ulp32(-3.0) == 2.0 ** -22 and sl.ulp32(0.0) == 2.0 ** -149
