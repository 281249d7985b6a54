"""CPU tests of the boundary of the fp8 lightning-indexer entries; no call here reaches a device."""
import ctypes as C

import pytest

from leetcuda_amd import capi
from tests.test_abi_cpu_mla_index import ARG, HEADDIM, IDS, LOGITS, OK, SHAPE, pointers

APPEND = ("B", "T", "max_nq", "num_pages", "page_size", "max_pages", "Di", "row_stride", "pow2")
OKA = dict(OK, row_stride=136, pow2=1)


def name_logits(a):
    b = C.create_string_buffer(64)
    return capi.load().lc_mla_index_logits_fp8_kernel_name(*(a[k] for k in LOGITS), b, 64), b.value.decode()


def name_append(a, bf16):
    b = C.create_string_buffer(64)
    return capi.load().lc_mla_index_append_fp8_kernel_name(*(a[k] for k in APPEND), bf16, b, 64), b.value.decode()


# what all three refuse, in the documented order: every case is made worse by a later-ranked fault (Di = 64: the head dim comes last)
ALL = [
    *((ARG, dict(null=i, T=0)) for i in (0, 1, 2, -1, -3)), (ARG, dict(null=-2, page_size=24)),
    *((SHAPE, {k: v, "Di": 64}) for k in ("B", "T", "max_nq", "num_pages", "max_pages") for v in (0, -2)),
    (SHAPE, dict(max_nq=41, Di=64)),
    *((SHAPE, dict(page_size=v, Di=64)) for v in (0, 8, 24)),
    (SHAPE, dict(max_pages=1 << 27, ld=1 << 40, Di=64)),          # positions past 2^31 - 1
    (SHAPE, dict(mis=(-1, 18), Di=64)), (SHAPE, dict(mis=(-3, 17), Di=64)),   # kv_len, cu_q off 4 bytes
    (HEADDIM, dict(Di=64)),
]
ONLY_LOGITS = [
    (ARG, dict(flags=2)), (ARG, dict(flags=3, T=0)), (ARG, dict(null=3, T=0)), (ARG, dict(null=4, T=0)),
    (SHAPE, dict(Hi=0, Di=64)), (SHAPE, dict(Di=0, Hi=128)),
    (SHAPE, dict(ld=159, Di=64)), (SHAPE, dict(ld=162, Di=64)),
    (SHAPE, dict(B=1 << 17, max_nq=1 << 12, T=1 << 12, Di=64)),   # the grid at the 16-token block: B x ceil(max_nq / 16) x 64 = 2^31
    (SHAPE, dict(B=1 << 25, max_nq=8, Di=64)),                     # ... and at the 8-token block: B x 1 x 64 = 2^31
    (SHAPE, dict(mis=(0, 8), Di=64)), (SHAPE, dict(mis=(2, 24), Di=64)),      # q8, the pool off 16 bytes
    (SHAPE, dict(mis=(1, 18), Di=64)), (SHAPE, dict(mis=(3, 18), Di=64)), (SHAPE, dict(mis=(4, 17), Di=64)),   # w, ks, logits off 4 bytes
    (HEADDIM, dict(Hi=128)), (HEADDIM, dict(Hi=128, Di=64)),
]
ONLY_APPEND = [
    (SHAPE, dict(row_stride=62, Di=64)), (SHAPE, dict(row_stride=126)), (SHAPE, dict(row_stride=129, Di=64)), (SHAPE, dict(row_stride=0, Di=64)),
    (SHAPE, dict(mis=(1, 24), Di=64)), (SHAPE, dict(mis=(0, 18), Di=64)), (SHAPE, dict(mis=(2, 18), Di=64)),   # the pool off 16, Kinew / ks off 4
]
CASES = [("logits", *c) for c in ALL + ONLY_LOGITS] + [("append", *c) for c in ALL + ONLY_APPEND]


@pytest.mark.parametrize("entry,want,bad", CASES, ids=IDS)
def test_statuses_and_their_order(built, entry, want, bad):
    bad = dict(bad)
    by_name = not {"null", "mis"} & set(bad)
    a = dict(OKA, **{k: v for k, v in bad.items() if k not in ("null", "mis")})
    if entry == "logits":
        assert capi.load().lc_mla_index_logits_fp8(*pointers(8, bad), *(a[k] for k in LOGITS), None) == want
        assert not by_name or name_logits(a)[0] == want
    else:
        ptrs = pointers(6, bad)
        assert [getattr(capi.load(), "lc_mla_index_append_fp8_" + el)(*ptrs, *(a[k] for k in APPEND), None) for el in ("f16", "bf16")] == [want, want]
        assert not by_name or (name_append(a, 0)[0], name_append(a, 1)[0]) == (want, want)


def test_the_edges_that_are_accepted_and_the_kernel_names(built):
    assert name_logits(OKA) == (capi.LC_OK, "mla_index_logits_fp8_kernel") and name_logits(dict(OKA, flags=0))[0] == capi.LC_OK
    assert name_logits(dict(OKA, B=(1 << 25) - 1, max_nq=8))[0] == capi.LC_OK        # one workgroup below the grid bound of the 8-token block
    assert name_logits(dict(OKA, B=(1 << 24), max_nq=9))[0] == capi.LC_OK            # nine tokens: ONE 16-token block, where the 16-bit entry has two
    assert name_logits(dict(OKA, B=(1 << 17) - 1, max_nq=1 << 12, T=1 << 12))[0] == capi.LC_OK
    assert name_append(OKA, 0) == (capi.LC_OK, "mla_index_append_fp8_kernel") and name_append(OKA, 1) == (capi.LC_OK, "mla_index_append_fp8_bf16_kernel")
    assert name_append(dict(OKA, row_stride=128, pow2=0), 0)[0] == capi.LC_OK
    assert capi.mla_index_logits_fp8_kernel_name(64, 64, 1, 1024, 64, 512) == "mla_index_logits_fp8_kernel"
    assert capi.mla_index_append_fp8_kernel_name(64, 64, 1, 1024, 64, 512, bf16=True) == "mla_index_append_fp8_bf16_kernel"
    assert capi.load().lc_mla_index_logits_fp8_kernel_name(*(OKA[k] for k in LOGITS), None, 64) == ARG
    assert capi.load().lc_mla_index_append_fp8_kernel_name(*(OKA[k] for k in APPEND), 0, None, 64) == ARG
