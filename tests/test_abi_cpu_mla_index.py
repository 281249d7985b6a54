"""CPU tests of the boundary of the lightning-indexer entries; no call here reaches a device."""
import ctypes as C

import pytest

from leetcuda_amd import capi

P = C.c_void_p(16)
ARG, SHAPE, HEADDIM = capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM
OK = dict(B=3, Hi=64, T=40, max_nq=9, num_pages=50, page_size=16, max_pages=10, Di=128, ld=160, topk=33, flags=1)
LOGITS = ("B", "Hi", "T", "max_nq", "num_pages", "page_size", "max_pages", "Di", "ld", "flags")
TOPK = ("B", "T", "max_nq", "num_pages", "page_size", "max_pages", "ld", "topk", "flags")


def run_logits(a, ptrs):
    return [getattr(capi.load(), s)(*ptrs, *(a[k] for k in LOGITS), None) for s in ("lc_mla_index_logits_f16", "lc_mla_index_logits_bf16")]


def name_logits(a, bf16):
    b = C.create_string_buffer(64)
    return capi.load().lc_mla_index_logits_kernel_name(*(a[k] for k in LOGITS), bf16, b, 64), b.value.decode()


def name_topk(a):
    b = C.create_string_buffer(64)
    return capi.load().lc_mla_index_topk_kernel_name(*(a[k] for k in TOPK), b, 64), b.value.decode()


# what both entries refuse, in the documented order: every case is made worse by a later-ranked fault (Di = 64: the head dims come last)
BOTH = [
    (ARG, dict(flags=2)), (ARG, dict(flags=3, T=0)), (ARG, dict(null=0, T=0)), (ARG, dict(null=-1, T=0)), (ARG, dict(null=-3, page_size=24)),
    *((SHAPE, {k: v, "Di": 64}) for k in ("B", "T", "max_nq", "num_pages", "max_pages") for v in (0, -2)),
    (SHAPE, dict(max_nq=41, Di=64)),
    *((SHAPE, dict(page_size=v, Di=64)) for v in (0, 8, 24)),
    (SHAPE, dict(max_pages=1 << 27, ld=1 << 40, Di=64)),          # positions past 2^31 - 1
    (SHAPE, dict(ld=159, Di=64)), (SHAPE, dict(ld=156, Di=64)), (SHAPE, dict(ld=162, Di=64)),
    (SHAPE, dict(mis=(-1, 18), Di=64)), (SHAPE, dict(mis=(-4, 17), Di=64)),   # kv_len, logits off 4 bytes
]
ONLY_LOGITS = [
    (ARG, dict(null=1, T=0)), (ARG, dict(null=2, T=0)),
    (SHAPE, dict(Hi=0, Di=64)), (SHAPE, dict(Di=0, Hi=128)), (SHAPE, dict(Di=-128, Hi=128)),
    (SHAPE, dict(B=1 << 22, max_nq=1 << 12, T=1 << 12, Di=64)),   # the grid: B x ceil(max_nq / 8) x 64
    (SHAPE, dict(mis=(0, 8), Di=64)), (SHAPE, dict(mis=(2, 24), Di=64)), (SHAPE, dict(mis=(1, 18), Di=64)),
    (HEADDIM, dict(Di=64)), (HEADDIM, dict(Hi=128)), (HEADDIM, dict(Hi=128, Di=64)),
]
ONLY_TOPK = [
    (ARG, dict(null=1, T=0)), (SHAPE, dict(topk=0)), (SHAPE, dict(topk=-1)),
    (SHAPE, dict(T=1 << 20, topk=1 << 11)),                        # T topk past 2^31 - 1
    (SHAPE, dict(mis=(1, 18))),
]
IDS = lambda x: str(x) if not isinstance(x, dict) else ",".join(f"{k}={v}" for k, v in x.items())


def pointers(n, bad):
    """n pointers; null / mis name one by index: negative indices count from the end (cu_q, block_table, kv_len are the last three of both)"""
    ptrs = [P] * n
    if "null" in bad:
        ptrs[bad.pop("null")] = None
    if "mis" in bad:
        i, addr = bad.pop("mis")
        ptrs[i] = C.c_void_p(addr)
    return ptrs


CASES = [("logits", *c) for c in BOTH + ONLY_LOGITS] + [("topk", *c) for c in BOTH + ONLY_TOPK]


@pytest.mark.parametrize("entry,want,bad", CASES, ids=IDS)
def test_statuses_and_their_order(built, entry, want, bad):
    logits = entry == "logits"
    bad = {k: v for k, v in bad.items() if logits or k != "Di"}
    if bad.get("mis", (0, 0))[0] == -4:
        bad["mis"] = (3 if logits else 0, bad["mis"][1])           # where the entry takes logits
    by_name = not {"null", "mis"} & set(bad)
    a = dict(OK, **{k: v for k, v in bad.items() if k not in ("null", "mis")})
    if logits:
        assert run_logits(a, pointers(7, bad)) == [want, want]
    else:
        assert capi.load().lc_mla_index_topk(*pointers(5, bad), *(a[k] for k in TOPK), None) == want
    if by_name:
        assert (name_logits(a, 0)[0], name_logits(a, 1)[0]) == (want, want) if logits else name_topk(a)[0] == want


def test_the_kernel_names(built):
    assert name_logits(OK, 0) == (capi.LC_OK, "mla_index_logits_kernel") and name_logits(OK, 1) == (capi.LC_OK, "mla_index_logits_bf16_kernel")
    assert name_logits(dict(OK, flags=0), 0)[0] == capi.LC_OK and name_topk(OK) == (capi.LC_OK, "mla_index_topk_kernel")
    assert capi.mla_index_logits_kernel_name(64, 64, 1, 1024, 64, 512, bf16=True) == "mla_index_logits_bf16_kernel"
    assert capi.mla_index_topk_kernel_name(64, 64, 1, 1024, 64, 512, 2048) == "mla_index_topk_kernel"
    assert capi.load().lc_mla_index_logits_kernel_name(*(OK[k] for k in LOGITS), 0, None, 64) == ARG
    assert capi.load().lc_mla_index_topk_kernel_name(*(OK[k] for k in TOPK), None, 64) == ARG
