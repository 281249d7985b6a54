"""CPU tests of the boundary of the five lc_mla_append_paged_* entries; no call here reaches a device."""
import ctypes as C
import re
from pathlib import Path

import pytest

from leetcuda_amd import capi

P, NAME = C.c_void_p(16), "lc_mla_append_paged_kernel_name"
RUN = {"lc_mla_append_paged_f16": 11, "lc_mla_append_paged_bf16": 11, "lc_mla_append_paged_kv8": 12, "lc_mla_append_paged_kv8_bf16": 12}   # pointers
OK = dict(B=2, H=16, T=40, max_nq=20, num_pages=70, page_size=16, max_pages=64, Dc=512, Dr=64, max_pos=1024, eps=1e-6, cs=584, ks=584,
          qs=16 * 192, qh=192, flags=0)
ARG, SHAPE, HEADDIM, QOUT, GAMMA, COS, SCALE = capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM, 3, 6, 7, 11      # statuses; pointer positions


def run(sym, ptrs, **kw):
    return getattr(capi.load(), sym)(*ptrs, *(dict(OK, **kw)[k] for k in OK), None)


def name(kv8=0, bf16=0, buf=True, **kw):
    a = dict(OK, **kw)
    b = C.create_string_buffer(128) if buf else None
    rc = getattr(capi.load(), NAME)(*(a[k] for k in ("B", "H", "T", "max_nq", "page_size", "max_pages", "Dc", "Dr", "max_pos", "flags")), kv8, bf16, b, 128)
    return rc, (b.value.decode() if buf else "")


def test_header_symbols_and_exports_agree(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()
    ctype = {"int": C.c_int, "float": C.c_float, "long long": C.c_longlong, "char*": C.c_char_p}
    for sym in (*RUN, NAME):
        assert hasattr(lib, sym) and sym in capi.SYMBOLS, sym
        m = re.search(r"\b" + sym + r"\(([^)]*)\)", header)         # (None: the header lacks the symbol)
        types = [re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0] for p in m.group(1).split(",")]
        assert capi.SYMBOLS[sym][1] == [ctype.get(t, C.c_void_p) for t in types], sym
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays
    assert "Not here: writing the latent cache" not in header


# in the order of the checks: every case is bad in one check and, where it can be, in a LATER one too, whose status must not show
BAD = [
    *((ARG, dict(null=i, mis=0, T=0, flags=2)) for i in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10)),      # every pointer but gamma and ckv_scale
    *((SHAPE, dict(mis=i, flags=2, Dc=128)) for i in (0, 1, 2, 3, 4, 5)),                      # off 16 bytes
    *((SHAPE, dict(mis=i, off=18, eps=-1.0)) for i in (GAMMA, COS)),                           # a float pointer off 4 bytes
    *((SHAPE, {k: 0, "flags": 2, "Dc": 128}) for k in ("B", "H", "T", "max_nq", "num_pages", "max_pages", "max_pos")),
    (SHAPE, dict(max_nq=41, flags=2)), (SHAPE, dict(page_size=8, eps=-1.0)), (SHAPE, dict(page_size=24, Dr=128)),
    (SHAPE, dict(page_size=1 << 10, max_pages=1 << 11, flags=2)),                             # one sequence's latent rows reach 2 GiB
    (SHAPE, dict(T=1 << 20, H=1 << 11, flags=2)),                                             # T H rows in 32 bits
    *((SHAPE, dict(flags=2, **{k: v})) for k, v in (("cs", 504), ("cs", 516), ("ks", 56), ("ks", 68), ("qh", 56), ("qh", 196), ("qs", 15 * 192 + 56), ("qs", 16 * 192 + 4))),
    (SHAPE, dict(same=True, flags=2)), (SHAPE, dict(same=True, Dc=128, qs=16 * 64 + 8, qh=64)),   # in place needs the dense layout
    (ARG, dict(flags=2, Dc=128)), (ARG, dict(flags=capi.ROPE_PACKED_SRC | capi.ROPE_INTERLEAVED)),
    *((ARG, dict(eps=e, Dc=128)) for e in (-1e-6, -1e-45, float("inf"), float("nan"))),
    (HEADDIM, dict(Dc=128, cs=128)), (HEADDIM, dict(Dr=128, ks=128, qh=128)), (HEADDIM, dict(Dc=64, Dr=512, cs=64, ks=512, qs=16 * 512, qh=512)),
    (HEADDIM, dict(same=True, Dc=256, flags=capi.ROPE_INTERLEAVED, eps=0.0, qs=16 * 64, qh=64)),           # in place on dense rows, eps = 0: accepted so far
]


@pytest.mark.parametrize("want,bad", BAD, ids=lambda x: str(x) if isinstance(x, int) else ",".join(f"{k}={v}" for k, v in x.items()))
def test_statuses_and_their_order(built, want, bad):
    bad = dict(bad)
    null, mis, off, same = bad.pop("null", None), bad.pop("mis", None), bad.pop("off", 8), bad.pop("same", False)
    for sym, nptr in RUN.items():
        ptrs = [P] * nptr
        ptrs[QOUT] = P if same else C.c_void_p(1 << 20)             # Qpe_out is Qpe only where the case says so
        if mis is not None:
            ptrs[mis] = C.c_void_p(off)
        if null is not None:
            ptrs[null] = None
        assert run(sym, ptrs, **bad) == want, sym
        if nptr == 12 and mis == COS:                               # ... and the scale of an fp8 pool, off 4 bytes
            ptrs[COS], ptrs[SCALE] = P, C.c_void_p(off)
            assert run(sym, ptrs, **bad) == want
    if null is None and mis is None and not same and not {"num_pages", "eps", "cs", "ks", "qs", "qh"} & set(bad):   # what the name call can see
        assert name(**bad)[0] == want and name(1, 1, **bad)[0] == want


def test_the_name_query_names_the_eight_kernels(built):
    assert name(buf=False)[0] == ARG and name(Dc=128)[0] == HEADDIM and name(1, 1, Dr=32)[0] == HEADDIM      # dense strides of the stated widths
    seen = set()
    for kv8, k8 in ((0, ""), (1, "kv8_")):
        for bf16, bf in ((0, ""), (1, "bf16_")):
            for flags, il in ((0, "false"), (capi.ROPE_INTERLEAVED, "true")):
                for T in (1, 40, 8192):                             # one token a wave and four: the same kernel
                    assert name(kv8, bf16, flags=flags, T=T, max_nq=1) == (capi.LC_OK, f"mla_append_paged_{k8}{bf}kernel<{il}>")
                seen.add(capi.mla_append_paged_kernel_name(64, 128, 64, 1, 64, 128, 4096, interleaved=bool(flags), kv8=bool(kv8), bf16=bool(bf16)))
    assert len(seen) == 8
