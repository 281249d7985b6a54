"""CPU tests of the boundary of ragged-batch attention and rotary embedding + append (lc_attn_varlen_paged_f16 / _kv8, lc_rope_append_varlen_f16 /
_kv8 and their name and workspace calls; no call here reaches a device): the ten exports and their argument counts, the statuses and their
order on doubly-bad calls, the name grid, the split rule's dependence on (B, T, max_nq, window) and on nothing else, the workspace formula, the
audit reports of the three new units, the Python wrappers' refusals — and the float64 reference of the GPU tests, local_lib.local64 per
sequence, against a by-hand case.

Inputs, truth and plan restatement are shared with tests/test_gpu_varlen.py: tests/varlen_lib.py."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import decode_lib as dl
from tests import local_lib as ll
from tests import varlen_lib as vl

P = C.c_void_p(16)
CAUSAL = capi.ATTN_CAUSAL
# per kind: (run symbol, pointers in front of the shape); ten ints B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window follow
RUN = {"paged": ("lc_attn_varlen_paged_f16", 7), "kv8": ("lc_attn_varlen_paged_kv8", 9)}
QUERY = {"paged": "lc_attn_varlen_paged", "kv8": "lc_attn_varlen_paged_kv8"}
ROPE = {"paged": ("lc_rope_append_varlen_f16", 10), "kv8": ("lc_rope_append_varlen_kv8", 12)}
ROPE_NAME = {"paged": "lc_rope_append_varlen_kernel_name", "kv8": "lc_rope_append_varlen_kv8_kernel_name"}
OK = (2, 8, 2, 40, 20, 70, 16, 64, 128)                        # B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D


@pytest.fixture
def knobs(built):
    yield from dl.reset_knobs()


def _run(kind, shape, window, flags, sinks=None, ptrs=None, ws=(None, 0)):
    """status of the run call on dummy pointers (only ever used on calls a check refuses: nothing reaches a device)"""
    sym, nptr = RUN[kind]
    return getattr(capi.load(), sym)(*([P] * nptr if ptrs is None else ptrs), *shape, window, sinks, flags, *ws, None)


def _name(kind, shape, window, flags):
    B, H, Hkv, T, max_nq, _, ps, mp, D = shape
    return vl._rc_name(QUERY[kind] + "_kernel_name", B, H, Hkv, T, max_nq, ps, mp, D, window, flags)


def _rope(kind, shape, rot=64, max_pos=1024, qs=None, ks=None, flags=0, ptrs=None):
    B, H, Hkv, T, max_nq, npg, ps, mp, D = shape
    sym, nptr = ROPE[kind]
    return getattr(capi.load(), sym)(*([P] * nptr if ptrs is None else ptrs), B, H, Hkv, T, max_nq, npg, ps, mp, D, rot, max_pos,
                                     H * D if qs is None else qs, Hkv * D if ks is None else ks, flags, None)


def _rope_name(kind, shape, rot=64, max_pos=1024, qs=None, ks=None, flags=0):
    B, H, Hkv, T, max_nq, _, ps, mp, D = shape
    return vl._rc_name(ROPE_NAME[kind], B, H, Hkv, T, max_nq, ps, mp, D, rot, max_pos, H * D if qs is None else qs, Hkv * D if ks is None else ks, flags)


def test_the_ten_symbols_are_exported_with_their_argument_counts(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()
    want = {}
    for kind in RUN:
        want[RUN[kind][0]] = RUN[kind][1] + 10 + 1 + 1 + 3          # pointers, ints with window, sinks, flags, workspace + bytes + stream
        want[QUERY[kind] + "_workspace_bytes"] = 9
        want[QUERY[kind] + "_kernel_name"] = 9 + 1 + 2
        want[ROPE[kind][0]] = ROPE[kind][1] + 11 + 2 + 1 + 1        # pointers, ints, two strides, flags, stream
        want[ROPE_NAME[kind]] = 10 + 2 + 1 + 2
    assert len(want) == 10
    for sym, n in want.items():
        assert hasattr(lib, sym), sym
        m = re.search(r"\b" + sym + r"\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == n == len(capi.SYMBOLS[sym][1]), (sym, n)
        params = [p.strip() for p in m.group(1).split(",")]
        if sym in (r[0] for r in RUN.values()):
            i = params.index("int flags")
            assert params[i - 2:i] == ["int window", "const float* sinks"], sym
            assert params[4] == "const int* cu_q" and params[params.index("int Hkv") + 1:][:2] == ["int T", "int max_nq"], sym
        if sym in (r[0] for r in ROPE.values()):
            assert params[7] == "const int* cu_q" and params[-4:-2] == ["long long q_row_stride", "long long kv_row_stride"], sym
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays
    for sym in ("lc_attn_varlen_f16", "lc_attn_varlen_kernel_name"):    # no contiguous-cache form
        assert not hasattr(lib, sym)


@pytest.mark.parametrize("kind", list(RUN))
def test_statuses_and_their_order(built, kind):
    nptr = RUN[kind][1]
    bad_shape = (2, 8, 3, 40, 20, 70, 16, 64, 256)
    # the local entry's two ARG cases in front of everything
    for w, flags in ((-1, CAUSAL), (5, 0), (0, 4), (5, capi.ATTN_V_TRANSPOSED)):
        assert _run(kind, OK, w, flags) == capi.LC_ERR_ARG
        assert _run(kind, bad_shape, w, flags) == capi.LC_ERR_ARG
        assert _name(kind, bad_shape, w, flags)[0] == capi.LC_ERR_ARG
    # a NULL pointer — cu_q among them — in front of the shape; the scales and the sinks may be NULL
    required = [0, 1, 2, 3, 4, 5, 6]
    for i in required:
        ptrs = [P] * nptr
        ptrs[i] = None
        assert _run(kind, bad_shape, 7, CAUSAL, ptrs=ptrs) == capi.LC_ERR_ARG, i
    # T < 1, max_nq < 1, max_nq > T: shape errors, in front of alignment and head dim
    mis = [P] * nptr
    mis[0] = C.c_void_p(8)
    for T, mq in ((0, 1), (-3, 1), (40, 0), (40, -1), (40, 41), (1, 2)):
        bad = (2, 8, 2, T, mq, 70, 16, 64, 96)
        assert _run(kind, bad, 0, 0) == capi.LC_ERR_SHAPE, (T, mq)
        assert _run(kind, bad, 0, 0, ptrs=mis) == capi.LC_ERR_SHAPE
        assert _name(kind, bad, 0, 0)[0] == capi.LC_ERR_SHAPE
        assert getattr(capi.load(), QUERY[kind] + "_workspace_bytes")(2, 8, 2, T, mq, 16, 64, 128, 0) == 0
    assert _run(kind, bad_shape, 0, 0) == capi.LC_ERR_SHAPE
    assert _run(kind, (2, 8, 2, 40, 20, 70, 24, 64, 128), 0, 0) == capi.LC_ERR_SHAPE           # a page size that is no power of two
    assert _run(kind, (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, 0, ptrs=mis) == capi.LC_ERR_SHAPE   # alignment in front of the head dim
    assert _run(kind, (2, 8, 2, 40, 40, 70, 16, 64, 96), 0, 0) == capi.LC_ERR_HEADDIM           # G max_nq > 64 is no error: the head dim is
    assert _name(kind, (2, 8, 2, 40, 40, 70, 16, 64, 96), 7, CAUSAL)[0] == capi.LC_ERR_HEADDIM
    assert _name(kind, (2, 8, 2, 40, 40, 70, 16, 64, 64), 7, CAUSAL)[0] == capi.LC_OK
    name_sym = getattr(capi.load(), QUERY[kind] + "_kernel_name")
    assert name_sym(2, 8, 2, 40, 20, 16, 64, 128, 0, 0, None, 128) == capi.LC_ERR_ARG
    assert name_sym(2, 8, 2, 40, 20, 16, 64, 128, 0, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG


@pytest.mark.parametrize("kind", list(RUN))
def test_a_small_or_misaligned_workspace_is_refused_before_any_device_work(knobs, kind):
    capi.tune("attn_decode_split", 4)
    for shape in ((2, 8, 2, 90, 40, 70, 16, 64, 128), (2, 8, 2, 9, 4, 70, 16, 64, 64)):      # RB = 3 and RB = 1
        B, H, Hkv, T, mq, _, ps, mp, D = shape
        need = vl.nbytes(kind, B, H, Hkv, T, mq, D, 33)
        assert need == 4 * (T * H) * (D + 1) * 4
        for nb in (0, 16, need - 1):
            assert _run(kind, shape, 33, CAUSAL, ws=(C.c_void_p(256), nb)) == capi.LC_ERR_ARG, nb
        assert _run(kind, shape, 33, CAUSAL, ws=(C.c_void_p(8), need)) == capi.LC_ERR_ARG


@pytest.mark.parametrize("kind", list(ROPE))
def test_rope_statuses_and_their_order(built, kind):
    nptr = ROPE[kind][1]
    bad_shape = (2, 8, 3, 40, 20, 70, 16, 64, 256)
    assert _rope_name(kind, OK) == (capi.LC_OK, f"rope_append_varlen{'_kv8' if kind == 'kv8' else ''}_kernel<128,false>")
    assert _rope_name(kind, OK, flags=capi.ROPE_INTERLEAVED)[1].endswith("<128,true>")
    assert _rope_name(kind, OK, qs=(8 + 4) * 128, ks=(8 + 4) * 128)[0] == capi.LC_OK      # three pointers into one projection output
    # LC_ROPE_PACKED_SRC is not accepted: the strides say it all
    for flags in (capi.ROPE_PACKED_SRC, capi.ROPE_PACKED_SRC | capi.ROPE_INTERLEAVED, 4):
        assert _rope(kind, bad_shape, flags=flags) == capi.LC_ERR_ARG
        assert _rope_name(kind, OK, flags=flags)[0] == capi.LC_ERR_ARG
    for i in range(10):                                             # Q, Knew, Vnew, Qout, the pools, cos_sin, cu_q, block_table, kv_len
        ptrs = [P] * nptr
        ptrs[i] = None
        assert _rope(kind, bad_shape, ptrs=ptrs) == capi.LC_ERR_ARG, i
    for T, mq in ((0, 1), (40, 0), (40, 41)):
        assert _rope(kind, (2, 8, 2, T, mq, 70, 16, 64, 96)) == capi.LC_ERR_SHAPE, (T, mq)
        assert _rope_name(kind, (2, 8, 2, T, mq, 70, 16, 64, 96))[0] == capi.LC_ERR_SHAPE
    for qs, ks in ((8 * 128 - 8, None), (8 * 128 + 4, None), (None, 2 * 128 - 8), (None, 2 * 128 + 2)):
        assert _rope(kind, OK, qs=qs, ks=ks) == capi.LC_ERR_SHAPE, (qs, ks)
        assert _rope_name(kind, OK, qs=qs, ks=ks)[0] == capi.LC_ERR_SHAPE
    for rot in (0, 8, 24, 144):
        assert _rope(kind, OK, rot=rot) == capi.LC_ERR_SHAPE, rot
    assert _rope(kind, OK, qs=8 * 128 + 8) == capi.LC_ERR_SHAPE     # in place (Q == Qout on the dummy pointers) needs the dense layout
    mis = [P] * nptr
    mis[3] = C.c_void_p(8)
    assert _rope(kind, (2, 8, 2, 40, 20, 70, 16, 64, 96), ptrs=mis) == capi.LC_ERR_SHAPE
    assert _rope_name(kind, (2, 8, 2, 40, 20, 70, 16, 64, 96))[0] == capi.LC_ERR_HEADDIM
    assert getattr(capi.load(), ROPE_NAME[kind])(2, 8, 2, 40, 20, 16, 64, 128, 64, 1024, 1024, 256, 0, None, 128) == capi.LC_ERR_ARG


def test_name_grid(knobs):
    """RB = 1 (RT 1 / 2 / 4) and RB > 1 x two caches x D x forced S; the window and the flags change no name: every kernel is LOCAL"""
    for D in vl.DS:
        for H, Hkv, mq in ((8, 2, 1), (8, 2, 4), (8, 2, 5), (8, 2, 8), (8, 2, 9), (8, 2, 16), (8, 2, 17), (8, 2, 130), (2, 2, 64), (2, 2, 65), (64, 1, 2)):
            for s in (1, 3, 64):
                capi.tune("attn_decode_split", s)
                for kind in vl.KINDS:
                    for B, T in ((1, 130), (6, 174), (64, 575)):
                        for w, flags in ((0, 0), (0, CAUSAL), (1, CAUSAL), (100, CAUSAL), (1 << 20, CAUSAL)):
                            assert vl.name(kind, B, H, Hkv, T, mq, D, w, flags) == (capi.LC_OK, vl.want_name(kind, H, Hkv, mq, D, s)), (kind, H, mq, w)
    assert capi.attn_varlen_paged_kernel_name(1, 8, 2, 40, 1, 16, 64, 128) == "attn_varlen_paged_kernel<128,1> x64"
    assert capi.attn_varlen_paged_kernel_name(1, 8, 2, 40, 5, 16, 64, 64, causal=True, window=9) == "attn_varlen_paged_kernel<64,2> x64"
    assert capi.attn_varlen_paged_kernel_name(1, 8, 2, 40, 16, 16, 64, 64, kv8=True) == "attn_varlen_paged_kv8_kernel<64,4> x64"
    assert capi.attn_varlen_paged_kernel_name(1, 8, 2, 40, 17, 16, 64, 128, kv8=True) == "attn_varlen_chunk_paged_kv8_kernel<128> x64"
    capi.tune("attn_decode_split", 1)
    assert capi.attn_varlen_paged_kernel_name(1, 8, 2, 40, 17, 16, 64, 128) == "attn_varlen_chunk_paged_kernel<128>"


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_auto_split_rule_follows_B_T_max_nq_and_the_window(knobs, cus):
    """S from (Hkv x min(B RB, ceil(G T / 64) + B) groups, the tiles of Ncap — of min(Ncap, W + max_nq - 1 + 63) keys with a window —, the CU
    count) alone: the same for the two caches, any flags; the workspace is S x T H x (D + 1) floats"""
    capi.tune("rule_cus", cus)
    seen = set()
    for B, H, Hkv, T, mq, ncap, D in ((64, 32, 8, 64, 1, 4096, 128), (64, 32, 8, 575, 512, 4096, 128), (8, 32, 8, 8000, 2048, 4096, 128),
                                      (1, 8, 2, 40, 1, 32768, 64), (1, 8, 1, 1, 1, 8192, 64), (6, 8, 2, 174, 130, 1024, 64), (2, 2, 1, 260, 130, 1 << 16, 128),
                                      (4, 8, 2, 4, 1, 1 << 15, 64), (4, 8, 2, 64, 16, 1 << 15, 64), (4, 8, 2, 64, 64, 1 << 15, 64)):
        G = H // Hkv
        groups = Hkv * min(B * ((G * mq + 63) // 64), (G * T + 63) // 64 + B)
        assert groups == vl.groups(B, H, Hkv, T, mq)
        for w in (0, 1, 64, 200, 4096, (1 << 31) - 1):
            s = vl.auto_split(B, H, Hkv, T, mq, ncap, w, cus)
            seen.add(s)
            assert s == dl.auto_split(groups, min(ncap, w + mq - 1 + 63) if w > 0 else ncap, cus)
            want_bytes = s * T * H * (D + 1) * 4 if s > 1 else 0
            for kind in vl.KINDS:
                for flags in ((0, CAUSAL) if w == 0 else (CAUSAL,)):
                    assert vl.name(kind, B, H, Hkv, T, mq, D, w, flags, ncap=ncap) == (capi.LC_OK, vl.want_name(kind, H, Hkv, mq, D, s)), (B, T, mq, w)
                assert vl.nbytes(kind, B, H, Hkv, T, mq, D, w, ncap=ncap) == want_bytes
                for ps in (64, 256):                                # the page size decides nothing
                    assert vl.name(kind, B, H, Hkv, T, mq, D, w, CAUSAL, ncap=ncap, ps=ps)[1] == vl.want_name(kind, H, Hkv, mq, D, s)
    assert len(seen) >= 4 and 1 in seen
    if cus == 256:      # by hand: a pure decode step of 64 sequences, Hkv = 8: 512 groups -> 1; one sequence of one token, Hkv = 2, 512 tiles: 128 -> 64
        assert vl.auto_split(64, 32, 8, 64, 1, 4096, 0, cus) == 1 and vl.auto_split(1, 8, 2, 40, 1, 32768, 0, cus) == 64
        # 63 decoding sequences and one chunk of 512: B RB = 64 x 32 = 2048 row blocks in the grid, at most ceil(4 x 575 / 64) + 64 = 100 with work
        assert vl.groups(64, 32, 8, 575, 512) == 8 * 100 and vl.groups(64, 32, 8, 64, 1) == 8 * 64


def test_the_restated_clamps_are_what_the_header_states():
    assert vl.cu_of((1, 0, 37)) == [0, 1, 1, 38]
    assert vl.owned([0, 1, 1, 38], 38, 37) == [(0, 1), (1, 0), (1, 37)]
    assert vl.owned([0, 1, 1, 38], 38, 8) == [(0, 1), (1, 0), (1, 8)]                          # Nq_b > max_nq
    assert vl.owned([-4, 5, 30, 28, 48, 900], 60, 20) == [(0, 5), (5, 20), (30, 0), (28, 20), (48, 12)]
    assert vl.owned([70, 80], 60, 20) == [(60, 0)] and vl.owned([-9, -2], 60, 20) == [(0, 0)]
    for cu in ([1 << 30, -(1 << 31), (1 << 31) - 1], [5, 5, 5], [59, 61, 60]):
        for q0, n in vl.owned(cu, 60, 20):
            assert 0 <= q0 <= 60 and 0 <= n <= 20 and q0 + n <= 60
    assert vl.rb_of(8, 2, 16) == 1 and vl.rb_of(8, 2, 17) == 2 and vl.rb_of(32, 8, 512) == 32


def test_audit_knows_the_varlen_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    for unit, mid, extra in (("tu_attn_varlen_paged", "_paged", 2), ("tu_attn_varlen_paged_kv8", "_paged_kv8", 0)):
        rep = json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text())
        names = " ".join(r["kernel"] for r in rep)
        for d in (64, 128):
            assert f"attn_varlen_chunk{mid}_kernelILi{d}EE" in names, (unit, d)
            for rt in (1, 2, 4):
                assert f"attn_varlen{mid}_kernelILi{d}ELi{rt}EE" in names, (unit, d, rt)
            assert (f"attn_varlen_combine_kernelILi{d}EE" in names) == (extra == 2)
        assert len(rep) == 8 + extra
    rep_rope = json.loads((obj / build.AUDIT_OWN_REPORT["tu_rope_append_varlen"]).read_text())
    names = " ".join(r["kernel"] for r in rep_rope)
    for d in (64, 128):
        for il in (0, 1):
            assert f"rope_append_varlen_kernelILi{d}ELb{il}EE" in names and f"rope_append_varlen_kv8_kernelILi{d}ELb{il}EE" in names
    assert len(rep_rope) == 8
    for unit in ("tu_attn_varlen_paged", "tu_attn_varlen_paged_kv8", "tu_rope_append_varlen"):
        for r in json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text()):
            for other in ("attn_decode", "attn_chunk", "attn_local", "rope_append_paged", "kv_append"):      # the other reports are read by those strings
                assert other not in r["kernel"], r["kernel"]
            assert r["scratch"] == 0 and not r["violations"], r
            assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]                       # plain HIP: listed for rule R2 only
            assert r["asm_loads"] == 0
    # the existing reports keep their entry counts and know nothing of the new units
    counts = {"isa_audit.json": None, build.AUDIT_OWN_REPORT["tu_attn_decode_paged"]: 6, build.AUDIT_OWN_REPORT["tu_attn_decode_paged_kv8"]: 6,
              build.AUDIT_OWN_REPORT["tu_attn_chunk"]: 6, build.AUDIT_OWN_REPORT["tu_attn_local"]: 8, build.AUDIT_OWN_REPORT["tu_attn_local_paged"]: 8,
              build.AUDIT_OWN_REPORT["tu_attn_local_paged_kv8"]: 8, build.AUDIT_OWN_REPORT["tu_rope_append"]: 8, build.AUDIT_OWN_REPORT["tu_kv_append"]: 4}
    for other, n in counts.items():
        text = (obj / other).read_text()
        assert "varlen" not in text, other
        assert n is None or len(json.loads(text)) == n, other


def test_capi_wrappers_refuse_bad_arguments_without_a_gpu(built):
    T, H, Hkv, D = 12, 8, 2, 64
    g = torch.Generator().manual_seed(1)
    q = torch.randn(T, H, D, generator=g).half()
    o = torch.empty_like(q)
    _, k, v = dl.decode_inputs(3, H, Hkv, 1, 128, D, seed=1)
    kp, vp, table = dl.paginate(k, v, (100, 17, 5), 16, seed=2)
    kp8, vp8 = (x.view(torch.uint8)[..., :64].contiguous() for x in (kp, vp))
    lens = torch.tensor([100, 17, 5], dtype=torch.int32)
    cu = torch.tensor([0, 5, 5, 12], dtype=torch.int32)
    calls = (lambda **kw: capi.attn_varlen_paged(kw.pop("q", q), kp, vp, kw.pop("o", o), kw.pop("cu", cu), table, kw.pop("lens", lens),
                                                 kw.pop("max_nq", 7), causal=True, **kw),
             lambda **kw: capi.attn_varlen_paged_kv8(kw.pop("q", q), kp8, vp8, kw.pop("o", o), kw.pop("cu", cu), table, kw.pop("lens", lens),
                                                     kw.pop("max_nq", 7), causal=True, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="window"):
            call(window=-1)
        with pytest.raises(ValueError, match="max_nq"):
            call(max_nq=0)
        with pytest.raises(ValueError, match="max_nq"):
            call(max_nq=T + 1)
        with pytest.raises(TypeError, match="sinks must be float32"):
            call(sinks=torch.zeros(8, dtype=torch.half))
        with pytest.raises(TypeError, match="int32"):
            call(cu=cu.long())
        for bad in (dict(cu=cu[:3]), dict(cu=torch.zeros(5, dtype=torch.int32)), dict(lens=lens[:2]), dict(sinks=torch.zeros(2)),
                    dict(q=q.view(1, T, H, D)), dict(o=o[:T - 1]), dict(q=q[:, :3], o=o[:, :3])):
            with pytest.raises(RuntimeError, match="Tensor size mismatch"):
                call(**bad)
        with pytest.raises(TypeError, match="float16"):
            call(q=q.float())
        with pytest.raises(RuntimeError, match="MI355X"):           # everything checked: only the device is missing
            call(window=3, sinks=torch.zeros(8))
    with pytest.raises(TypeError, match="float8_e4m3fn or uint8"):
        capi.attn_varlen_paged_kv8(q, kp, vp, o, cu, table, lens, 7)
    with pytest.raises(TypeError, match="float16"):
        capi.attn_varlen_paged(q, kp8, vp8, o, cu, table, lens, 7)
    # the rope call
    cs = capi.rope_table(128, D)
    qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=g).half()
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D), qkv[:, (H + Hkv) * D:].view(T, Hkv, D)
    assert capi._rope_varlen_args(qv, kv, vv, kp, vp, cs, cu, table, lens, 7, None) == (3, H, Hkv, T, 7, kp.shape[0], 16, 8, D, D, 128, 768, 768)
    assert capi._rope_varlen_args(q, kv.contiguous(), vv.contiguous(), kp8, vp8, cs, cu, table, lens, 7, q, kv8=True)[-2:] == (H * D, Hkv * D)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.rope_append_varlen(qv, kv, vv, kp, vp, cs, cu, table, lens, 7)
    with pytest.raises(RuntimeError, match="in place"):
        capi.rope_append_varlen(qv, kv, vv, kp, vp, cs, cu, table, lens, 7, q_out=qv)
    with pytest.raises(RuntimeError, match="one stride"):
        capi.rope_append_varlen(qv, kv, vv.contiguous(), kp, vp, cs, cu, table, lens, 7)
    with pytest.raises(RuntimeError, match="row stride|dense"):
        capi.rope_append_varlen(qv.transpose(0, 1).contiguous().transpose(0, 1), kv, vv, kp, vp, cs, cu, table, lens, 7)
    with pytest.raises(ValueError, match="max_nq"):
        capi.rope_append_varlen(qv, kv, vv, kp, vp, cs, cu, table, lens, T + 1)
    with pytest.raises(TypeError, match="float16"):
        capi.rope_append_varlen(qv, kv, vv, kp8, vp8, cs, cu, table, lens, 7)
    with pytest.raises(TypeError, match="fp8 pools"):
        capi._rope_varlen_args(qv, kv, vv, kp, vp, cs, cu, table, lens, 7, None, k_scale=torch.ones(2))
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi.rope_append_varlen(qv, kv[:, :1], vv[:, :1], kp, vp, cs, cu, table, lens, 7)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi.rope_append_varlen_kv8(qv, kv, vv, kp8, vp8, cs, cu[:3], table, lens, 7)


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference of the GPU tests

def test_ragged64_of_a_uniform_batch_is_local64():
    B, H, Nq, D = 3, 8, 5, 64
    q, k, v = dl.decode_inputs(B, H, 2, Nq, 256, D, seed=21)
    lens = (256, 129, 3)
    sinks = torch.tensor([0.5, -1.0, 2.0, -float("inf"), 0.0, 1.0, -2.0, 3.0])
    for window, sk in ((0, None), (7, None), (33, sinks)):
        want, nv = ll.local64(q, k.double(), v.double(), lens, True, window=window, sinks=sk)
        got, nvis = vl.ragged64(vl.to_tokens(q), k.double(), v.double(), vl.cu_of([Nq] * B), lens, Nq, True, window=window, sinks=sk)
        assert np.abs(vl.from_tokens(torch.from_numpy(got), B, Nq).numpy() - want).max() <= 1e-13
        assert (nvis.reshape(B, Nq) == nv).all()
    assert torch.equal(vl.from_tokens(vl.to_tokens(q), B, Nq), q)


def test_ragged64_by_hand():
    H, D = 4, 64
    _, k, v = dl.decode_inputs(3, H, 2, 1, 64, D, seed=22)
    nqs, lens = (2, 0, 3), (40, 9, 2)
    cu = vl.cu_of(nqs)
    q = torch.randn(cu[-1] + 2, H, D, generator=torch.Generator().manual_seed(3)).half()      # two rows nobody owns
    sinks = torch.tensor([0.5, -1.0, 2.0, -float("inf")])
    got, nvis = vl.ragged64(q, k.double(), v.double(), cu, lens, 3, True, window=7, sinks=sinks)
    assert nvis.tolist() == [7, 7, 0, 1, 2, -1, -1] and (got[5:] == 0).all()
    for t, b, i in ((0, 0, 0), (1, 0, 1), (2, 2, 0), (3, 2, 1), (4, 2, 2)):
        p = lens[b] - nqs[b] + i                                    # the position of query i of sequence b
        keys = [j for j in range(64) if p - 7 < j <= p and j >= 0]
        assert len(keys) == nvis[t]
        for h in range(H):
            if not keys:
                assert (got[t, h] == 0).all()
                continue
            s = torch.tensor([float(q[t, h].double() @ k[b, h // 2, j].double()) / 8.0 for j in keys], dtype=torch.float64)
            den = torch.exp(s).sum() + torch.exp(sinks[h].double())
            want = sum((torch.exp(s[n]) / den) * v[b, h // 2, j].double() for n, j in enumerate(keys))
            assert np.abs(got[t, h] - want.numpy()).max() <= 1e-12, (t, h)
    # max_nq cuts sequence 2 to its first two rows, which then sit at positions L - 2 + i
    got2, nvis2 = vl.ragged64(q, k.double(), v.double(), cu, lens, 2, True, window=1)
    assert nvis2.tolist() == [1, 1, 1, 1, -1, -1, -1]
    assert np.abs(got2[3, 3] - v[2, 1, 1].double().numpy()).max() <= 1e-15 and np.abs(got2[0, 0] - v[0, 0, 38].double().numpy()).max() <= 1e-15
