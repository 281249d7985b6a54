"""CPU tests of the boundary of the three lc_attn_mla_paged_kv8* entries; no call here reaches a device."""
import ctypes as C
import re
from pathlib import Path

import pytest

from leetcuda_amd import capi
from tests.test_abi_cpu_mla import knobs  # noqa: F401  (the fixture: the library loaded, the knobs back at their defaults afterwards)

P = C.c_void_p(16)
RUN = ("lc_attn_mla_paged_kv8", "lc_attn_mla_paged_kv8_bf16")
OK = dict(B=2, H=16, T=40, max_nq=20, num_pages=70, page_size=16, max_pages=64, Dc=512, Dr=64, sm_scale=0.1, flags=0)
ARG, SHAPE, HEADDIM = capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM
SCALE = 9                                  # the position of ckv_scale; 5 is lse


def run(sym, ptrs=None, ws=(None, 0), **kw):
    a = dict(OK, **kw)
    return getattr(capi.load(), sym)(*([P] * 10 if ptrs is None else ptrs), *(a[k] for k in OK), *ws, None)


def name(bf16=0, buf=True, **kw):
    b = C.create_string_buffer(128) if buf else None
    rc = capi.load().lc_attn_mla_paged_kv8_kernel_name(*(dict(OK, **kw)[k] for k in ("B", "H", "T", "max_nq", "page_size", "max_pages", "Dc", "Dr", "flags")),
                                                       bf16, b, 128)
    return rc, (b.value.decode() if buf else "")


def test_header_symbols_and_exports_agree(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()
    ctype = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "char*": C.c_char_p}
    for sym in RUN + ("lc_attn_mla_paged_kv8_kernel_name",):
        assert hasattr(lib, sym) and sym in capi.SYMBOLS, sym
        m = re.search(r"\b" + sym + r"\(([^)]*)\)", header)     # (None: the header lacks the symbol)
        types = [re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0] for p in m.group(1).split(",")]
        assert capi.SYMBOLS[sym][1] == [ctype.get(t, C.c_void_p) for t in types], sym
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays


BAD = [
    (ARG, dict(flags=2)), (ARG, dict(flags=2, T=0, Dc=128)),
    *((ARG, dict(null=i, T=0)) for i in (0, 1, 2, 3, 4, 6, 7, 8)),             # every pointer but lse and ckv_scale, in front of the shape
    (ARG, dict(mis=SCALE, off=2, T=0)), (ARG, dict(mis=SCALE, off=17, T=0, Dc=128)),   # ckv_scale off 4 bytes: with the pointers
    *((ARG, dict(sm_scale=s, T=0)) for s in (0.0, float("nan"))),
    *((SHAPE, {k: 0, "Dc": 128}) for k in ("B", "H", "T", "max_nq", "num_pages", "max_pages")),
    (SHAPE, dict(max_nq=41)), (SHAPE, dict(page_size=8, Dc=128)), (SHAPE, dict(page_size=24, Dc=128)),
    (SHAPE, dict(page_size=1 << 10, max_pages=1 << 11, Dc=128)),                # the plan and its bounds are the 16-bit call's
    *((SHAPE, dict(mis=i, Dc=128)) for i in (0, 1, 2, 3, 4)),                   # a pointer off 16 bytes (the code pool too), in front of the head dims
    (HEADDIM, dict(Dc=128)), (HEADDIM, dict(Dr=128)), (HEADDIM, dict(Dc=64, Dr=512)),
]


@pytest.mark.parametrize("want,bad", BAD, ids=lambda x: str(x) if isinstance(x, int) else ",".join(f"{k}={v}" for k, v in x.items()))
def test_statuses_and_their_order(built, want, bad):
    bad = dict(bad)
    ptrs = [P] * 10
    if "null" in bad:
        ptrs[bad.pop("null")] = None
    if "mis" in bad:
        ptrs[bad.pop("mis")] = C.c_void_p(bad.pop("off", 8))
    for sym in RUN:
        assert run(sym, ptrs, **bad) == want
    if all(p is not None and p.value == 16 for p in ptrs) and not {"sm_scale", "num_pages"} & set(bad):     # what a name call can see
        assert name(**bad)[0] == want and name(1, **bad)[0] == want


def test_scale_and_lse_may_be_null_and_a_bad_workspace_is_refused_last(knobs):
    capi.tune("attn_decode_split", 3)
    need = capi.attn_mla_paged_workspace_bytes(*(OK[k] for k in ("B", "H", "T", "max_nq", "page_size", "max_pages")))
    assert need == 3 * OK["T"] * OK["H"] * 513 * 4                              # one query serves both element widths
    for ptrs in ([P] * 5 + [None] + [P] * 3 + [None], [P] * 9 + [C.c_void_p(4)]):     # no lse and no scale; a scale on 4 bytes
        for sym in RUN:
            for ws in ((C.c_void_p(256), 0), (C.c_void_p(256), need - 1), (C.c_void_p(8), need)):
                assert run(sym, ptrs, ws=ws) == ARG
            assert run(sym, ptrs, ws=(C.c_void_p(8), 0), Dc=128) == HEADDIM    # ... behind the head dims


def test_the_name_query_names_the_kernels(knobs):
    assert name(buf=False)[0] == ARG
    for s in (1, 2, 64):
        capi.tune("attn_decode_split", s)
        for bf16, bf in ((0, ""), (1, "bf16_")):
            tail = f" + attn_mla_combine_{bf}kernel x{s}" if s > 1 else ""
            assert name(bf16, flags=capi.ATTN_CAUSAL) == (capi.LC_OK, f"attn_mla_paged_kv8_{bf}kernel{tail}")
    assert capi.attn_mla_paged_kv8_kernel_name(2, 128, 40, 2, 64, 64, bf16=True, causal=True) == "attn_mla_paged_kv8_bf16_kernel + attn_mla_combine_bf16_kernel x64"
