"""CPU tests of the boundary of the four lc_attn_mla_sparse_* entries; no call here reaches a device."""
import ctypes as C

import pytest

from leetcuda_amd import capi
from tests import decode_lib as dl

P = C.c_void_p(16)
RUN = ("lc_attn_mla_sparse_f16", "lc_attn_mla_sparse_bf16")
OK = dict(T=40, H=16, topk=130, num_slots=1000, Dc=512, Dr=64, sm_scale=0.1, flags=0)
ARG, SHAPE, HEADDIM = capi.LC_ERR_ARG, capi.LC_ERR_SHAPE, capi.LC_ERR_HEADDIM
NEED3 = 3 * OK["T"] * OK["H"] * 513 * 4      # the partials of three ranges


@pytest.fixture
def knobs(built):
    yield from dl.reset_knobs()


def name(bf16=0, **kw):
    b = C.create_string_buffer(128)
    rc = capi.load().lc_attn_mla_sparse_kernel_name(*(dict(OK, **kw)[k] for k in ("T", "H", "topk", "Dc", "Dr", "flags")), bf16, b, 128)
    return rc, b.value.decode()


BAD = [
    (ARG, dict(flags=1)), (ARG, dict(flags=2)), (ARG, dict(flags=1, T=0, Dc=128)),      # no flag is defined; the doubly-bad call: flags first
    *((ARG, dict(null=i, T=0)) for i in (0, 1, 2, 3, 4, 6)),                            # every pointer but lse, in front of the shape
    *((ARG, dict(sm_scale=s, T=0)) for s in (0.0, -0.5, float("inf"), float("nan"))),
    *((SHAPE, {k: v, "Dc": 128}) for k in ("T", "H", "topk", "num_slots") for v in (0, -3)),
    (SHAPE, dict(T=1 << 20, H=1 << 12, Dc=128)),                                        # T H past 2^31 - 1
    (SHAPE, dict(T=1 << 25, H=1, Dc=128)),                                              # the grid: T x RB x 64
    *((SHAPE, dict(mis=(i, 8), Dc=128)) for i in (0, 1, 2, 3, 4)), (SHAPE, dict(mis=(6, 18), Dc=128)),   # 16-bit pointers off 16 bytes, slots off 4
    (HEADDIM, dict(Dc=128)), (HEADDIM, dict(Dr=128)), (HEADDIM, dict(Dc=576)), (HEADDIM, dict(Dc=64, Dr=512)),
    *((ARG, dict(ws=ws)) for ws in ((256, 0), (256, NEED3 - 1), (8, NEED3))), (HEADDIM, dict(ws=(8, 0), Dc=128)),   # the workspace, last
]


@pytest.mark.parametrize("want,bad", BAD, ids=lambda x: str(x) if isinstance(x, int) else ",".join(f"{k}={v}" for k, v in x.items()))
def test_statuses_and_their_order(knobs, want, bad):
    bad = dict(bad)
    ptrs = [P] * 5 + [None] + [P]                                                       # lse may be NULL
    seen_by_name = not {"null", "mis", "ws", "sm_scale", "num_slots"} & set(bad)
    if "null" in bad:
        ptrs[bad.pop("null")] = None
    if "mis" in bad:
        i, addr = bad.pop("mis")
        ptrs[i] = C.c_void_p(addr)
    ws = bad.pop("ws", None)
    capi.tune("attn_decode_split", 3 if ws else 0)
    a = dict(OK, **bad)
    for sym in RUN:
        assert getattr(capi.load(), sym)(*ptrs, *(a[k] for k in OK), *((C.c_void_p(ws[0]), ws[1]) if ws else (None, 0)), None) == want
    if seen_by_name:
        assert name(**bad)[0] == want and name(1, **bad)[0] == want
        assert "flags" in bad or capi.load().lc_attn_mla_sparse_workspace_bytes(*(a[k] for k in ("T", "H", "topk", "Dc", "Dr"))) == 0


def test_the_name_and_workspace_queries(knobs):
    assert capi.load().lc_attn_mla_sparse_kernel_name(40, 16, 130, 512, 64, 0, 0, None, 128) == ARG
    for s in (1, 3):
        capi.tune("attn_decode_split", s)
        assert capi.attn_mla_sparse_workspace_bytes(OK["T"], OK["H"], OK["topk"]) == (NEED3 if s == 3 else 0)
        for bf16, bf in ((0, ""), (1, "bf16_")):
            tail = f" + attn_mla_sparse_combine_{bf}kernel x{s}" if s > 1 else ""
            assert name(bf16) == (capi.LC_OK, f"attn_mla_sparse_{bf}kernel{tail}")
    capi.tune("attn_decode_split", 0)
    capi.tune("rule_cus", 256)                       # S from T, H, topk and the CU count: 64 tokens x 2 row blocks, 32 tiles
    assert capi.attn_mla_sparse_kernel_name(64, 128, 2048, bf16=True) == "attn_mla_sparse_bf16_kernel + attn_mla_sparse_combine_bf16_kernel x2"
    assert capi.attn_mla_sparse_kernel_name(1024, 128, 2048) == "attn_mla_sparse_kernel"
