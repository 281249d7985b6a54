"""CPU tests of the boundary of the three lc_attn_mla_sparse_kv8* entries; no call here reaches a device."""
import ctypes as C
import re
from pathlib import Path

import pytest

from leetcuda_amd import capi
from tests.test_abi_cpu_mla_sparse import ARG, BAD, NEED3, OK, P, knobs  # noqa: F401  (knobs: the fixture)

RUN = ("lc_attn_mla_sparse_kv8", "lc_attn_mla_sparse_kv8_bf16")
TWIN = ("lc_attn_mla_sparse_f16", "lc_attn_mla_sparse_bf16")
NAME = "lc_attn_mla_sparse_kv8_kernel_name"


def params(header, sym):
    return [re.sub(r"\s+", " ", p.strip()) for p in re.search(r"\b" + sym + r"\(([^)]*)\)", header).group(1).split(",")]


def name(bf16=0, **kw):
    b = C.create_string_buffer(128)
    rc = getattr(capi.load(), NAME)(*(dict(OK, **kw)[k] for k in ("T", "H", "topk", "Dc", "Dr", "flags")), bf16, b, 128)
    return rc, b.value.decode()


def test_header_symbols_and_exports_agree(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()
    ctype = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "char*": C.c_char_p}
    for sym in RUN + (NAME,):
        assert hasattr(lib, sym) and sym in capi.SYMBOLS, sym
        assert capi.SYMBOLS[sym][1] == [ctype.get(p.rsplit(" ", 1)[0], C.c_void_p) for p in params(header, sym)], sym
    for sym, twin in zip(RUN, TWIN):                                # the twin's list with the scale right behind slots
        want = params(header, twin)
        want.insert(want.index("const int* slots") + 1, "const float* ckv_scale")
        assert [p.replace("CKVpool8", "CKVpool") for p in params(header, sym)] == want, sym
    assert params(header, NAME) == params(header, "lc_attn_mla_sparse_kernel_name")
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays


@pytest.mark.parametrize("want,bad", BAD, ids=lambda x: str(x) if isinstance(x, int) else ",".join(f"{k}={v}" for k, v in x.items()))
def test_every_bad_call_of_the_16_bit_table_gets_the_twins_status(knobs, want, bad):
    bad = dict(bad)
    ptrs = [P] * 5 + [None] + [P]                                   # lse may be NULL
    seen_by_name = not {"null", "mis", "ws", "sm_scale", "num_slots"} & set(bad)
    if "null" in bad:
        ptrs[bad.pop("null")] = None
    if "mis" in bad:
        i, addr = bad.pop("mis")
        ptrs[i] = C.c_void_p(addr)
    ws = bad.pop("ws", None)
    capi.tune("attn_decode_split", 3 if ws else 0)
    a = dict(OK, **bad)
    tail = (*(a[k] for k in OK), *((C.c_void_p(ws[0]), ws[1]) if ws else (None, 0)), None)
    for sym, twin in zip(RUN, TWIN):
        assert getattr(capi.load(), twin)(*ptrs, *tail) == want
        for scale in (None, C.c_void_p(4)):                         # no scale; a scale on 4 bytes
            assert getattr(capi.load(), sym)(*ptrs, scale, *tail) == want
    if seen_by_name:
        assert name(**bad)[0] == want and name(1, **bad)[0] == want


def test_a_scale_off_4_bytes_is_refused_with_the_pointers(built):
    for sym in RUN:
        for off in (2, 17):
            assert getattr(capi.load(), sym)(*([P] * 7), C.c_void_p(off), *(dict(OK, T=0, Dc=128)[k] for k in OK), None, 0, None) == ARG


def test_the_name_query_names_the_kernels(knobs):
    assert getattr(capi.load(), NAME)(40, 16, 130, 512, 64, 0, 0, None, 128) == ARG
    for s in (1, 2):
        capi.tune("attn_decode_split", s)
        assert capi.attn_mla_sparse_workspace_bytes(OK["T"], OK["H"], OK["topk"]) == (NEED3 // 3 * 2 if s == 2 else 0)   # one query serves both widths
        for bf16, bf in ((0, ""), (1, "bf16_")):
            tail = f" + attn_mla_sparse_combine_{bf}kernel x{s}" if s > 1 else ""
            assert name(bf16) == (capi.LC_OK, f"attn_mla_sparse_kv8_{bf}kernel{tail}")
            assert capi.attn_mla_sparse_kv8_kernel_name(OK["T"], OK["H"], OK["topk"], bf16=bool(bf16)) == f"attn_mla_sparse_kv8_{bf}kernel{tail}"
