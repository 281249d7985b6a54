"""CPU tests of the boundary of the three lc_attn_mla_prefill_* entries; no call here reaches a device."""
import ctypes as C
from pathlib import Path

import pytest

from leetcuda_amd import capi
from tests.test_abi_cpu_mla_sparse_kv8 import params

P = C.c_void_p(16)
RUN = ("lc_attn_mla_prefill_f16", "lc_attn_mla_prefill_bf16")
NAME = "lc_attn_mla_prefill_kernel_name"
STRIDES = ("qr", "qh", "knr", "knh", "kper", "vr", "vh")
OK = dict(B=2, H=4, Tq=300, Tk=400, max_nq=130, Dn=128, Dr=64, Dv=128, sm_scale=0.07, flags=1,
          qr=4 * 192, qh=192, knr=4 * 256, knh=256, kper=64, vr=4 * 256, vh=256)
ARG, SHAPE, HEADDIM = capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM


def name(bf16=0, **kw):
    b = C.create_string_buffer(128)
    rc = getattr(capi.load(), NAME)(*(dict(OK, **kw)[k] for k in ("B", "H", "Tq", "max_nq", "Dn", "Dr", "Dv", "flags")), bf16, b, 128)
    return rc, b.value.decode()


BAD = [
    (ARG, dict(flags=2)), (ARG, dict(flags=3)), (ARG, dict(flags=4, Tq=0, Dr=32)),      # only LC_ATTN_CAUSAL; the triply-bad call: flags first
    *((ARG, dict(null=i, Tq=0)) for i in (0, 1, 2, 3, 4, 6, 7)),                        # every pointer but lse, in front of the shape
    *((ARG, dict(sm_scale=s, Tq=0)) for s in (0.0, -0.5, float("inf"), float("nan"))),
    *((SHAPE, {"Dr": 32, k: v}) for k in ("B", "H", "Tq", "Tk", "max_nq", "Dn", "Dr", "Dv") for v in (0, -3)),
    (SHAPE, dict(max_nq=301, Dr=32)),                                                   # max_nq > Tq
    (SHAPE, dict(Tq=1 << 20, H=1 << 12, Dr=32)),                                        # Tq H past 2^31 - 1
    (SHAPE, dict(B=1 << 21, H=1 << 10, Tq=1 << 20, Dr=32)),                             # the grid: 2 row blocks x B x H
    *((SHAPE, dict(mis=(i, 8), Dr=32)) for i in range(5)), *((SHAPE, dict(mis=(i, 18), Dr=32)) for i in (5, 6, 7)),   # 16-bit pointers off 16, lse / cu_* off 4
    *((SHAPE, {k: v}) for k, v in (("qh", 184), ("qh", 196), ("qr", 4 * 192 - 8), ("qr", 4 * 192 + 4), ("knh", 120), ("knr", 3 * 256 + 120),
                                   ("kper", 56), ("kper", 68), ("vh", 124), ("vr", 3 * 256 + 120), ("vr", -1024))),
    (SHAPE, dict(kper=56, Dv=64)),                                                      # a stride in front of the head dims
    (HEADDIM, dict(Dn=64)), (HEADDIM, dict(Dr=32)), (HEADDIM, dict(Dv=64)), (HEADDIM, dict(Dv=120)), (HEADDIM, dict(Dn=96, Dr=32)),
]


@pytest.mark.parametrize("want,bad", BAD, ids=lambda x: str(x) if isinstance(x, int) else ",".join(f"{k}={v}" for k, v in x.items()))
def test_statuses_and_their_order(built, want, bad):
    bad = dict(bad)
    ptrs = [P] * 5 + [None] + [P] * 2                                                   # lse may be NULL
    seen_by_name = not ({"null", "mis", "sm_scale", "Tk"} | set(STRIDES)) & set(bad)
    if "null" in bad:
        ptrs[bad.pop("null")] = None
    if "mis" in bad:
        i, addr = bad.pop("mis")
        ptrs[i] = C.c_void_p(addr)
    a = dict(OK, **bad)
    for sym in RUN:
        assert getattr(capi.load(), sym)(*ptrs, *(a[k] for k in OK), None) == want
    if seen_by_name:
        assert name(**bad)[0] == want and name(1, **bad)[0] == want


@pytest.mark.parametrize("max_nq,rs", ((64, 1), (65, 2)))
def test_the_name_call_names_the_row_sets(built, max_nq, rs):
    assert getattr(capi.load(), NAME)(2, 4, 300, max_nq, 128, 64, 128, 1, 0, None, 128) == ARG
    for bf16, bf in ((0, ""), (1, "bf16_")):
        assert name(bf16, max_nq=max_nq) == (capi.LC_OK, f"attn_mla_prefill_{bf}kernel<{rs}>")
        assert capi.attn_mla_prefill_kernel_name(2, 4, 300, max_nq, causal=False, bf16=bool(bf16)) == f"attn_mla_prefill_{bf}kernel<{rs}>"


def test_header_symbols_and_exports_agree(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()
    ctype = {"int": C.c_int, "float": C.c_float, "long long": C.c_longlong, "char*": C.c_char_p}
    for sym in RUN + (NAME,):
        assert hasattr(lib, sym) and sym in capi.SYMBOLS, sym
        assert capi.SYMBOLS[sym][1] == [ctype.get(p.rsplit(" ", 1)[0], C.c_void_p) for p in params(header, sym)], sym
    assert params(header, RUN[0]) == params(header, RUN[1])
    assert lib.lc_abi_version() == 2                                                    # additive: the ABI version stays
