"""CPU tests of the boundary of the bfloat16 ragged-batch entries (lc_attn_varlen_paged_bf16 / _kv8_bf16, lc_rope_append_varlen_bf16 / _kv8_bf16
and their four name calls; no call here reaches a device): header, capi.SYMBOLS and exports agree; every bad-argument
case of tests/test_abi_cpu_varlen.py's tables gives a bf16 entry the status of its fp16 twin; the name calls report the fp16 plan with the bf16
kernel in it; the Python wrappers refuse float16 and float32 and accept bfloat16 up to the missing device; the three new audit reports; and the
helpers of tests/bf16_lib.py that the GPU module's bounds rest on."""
import ctypes as C
import json
import re
from pathlib import Path

import pytest
import torch

from leetcuda_amd import capi
from tests import bf16_lib as bl
from tests import decode_lib as dl
from tests import varlen_lib as vl

P = C.c_void_p(16)
CAUSAL = capi.ATTN_CAUSAL
BF = torch.bfloat16
# fp16 twin -> bf16 entry; pointers in front of the shape
RUN = {"paged": ("lc_attn_varlen_paged_f16", "lc_attn_varlen_paged_bf16", 7), "kv8": ("lc_attn_varlen_paged_kv8", "lc_attn_varlen_paged_kv8_bf16", 9)}
NAME = {"paged": ("lc_attn_varlen_paged_kernel_name", "lc_attn_varlen_paged_bf16_kernel_name"),
        "kv8": ("lc_attn_varlen_paged_kv8_kernel_name", "lc_attn_varlen_paged_kv8_bf16_kernel_name")}
BYTES = {"paged": "lc_attn_varlen_paged_workspace_bytes", "kv8": "lc_attn_varlen_paged_kv8_workspace_bytes"}      # one query serves both
ROPE = {"paged": ("lc_rope_append_varlen_f16", "lc_rope_append_varlen_bf16", 10), "kv8": ("lc_rope_append_varlen_kv8", "lc_rope_append_varlen_kv8_bf16", 12)}
ROPE_NAME = {"paged": ("lc_rope_append_varlen_kernel_name", "lc_rope_append_varlen_bf16_kernel_name"),
             "kv8": ("lc_rope_append_varlen_kv8_kernel_name", "lc_rope_append_varlen_kv8_bf16_kernel_name")}
OK = (2, 8, 2, 40, 20, 70, 16, 64, 128)                        # B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D
BAD = (2, 8, 3, 40, 20, 70, 16, 64, 256)


@pytest.fixture
def knobs(built):
    yield from dl.reset_knobs()


def _run(sym, nptr, shape, window, flags, sinks=None, ptrs=None, ws=(None, 0)):
    """status of a run call on dummy pointers (only ever used on calls a check refuses: nothing reaches a device)"""
    return getattr(capi.load(), sym)(*([P] * nptr if ptrs is None else ptrs), *shape, window, sinks, flags, *ws, None)


def _name(sym, shape, window, flags):
    B, H, Hkv, T, max_nq, _, ps, mp, D = shape
    return vl._rc_name(sym, B, H, Hkv, T, max_nq, ps, mp, D, window, flags)


def _rope(sym, nptr, shape, rot=64, max_pos=1024, qs=None, ks=None, flags=0, ptrs=None):
    B, H, Hkv, T, max_nq, npg, ps, mp, D = shape
    return getattr(capi.load(), sym)(*([P] * nptr if ptrs is None else ptrs), B, H, Hkv, T, max_nq, npg, ps, mp, D, rot, max_pos,
                                     H * D if qs is None else qs, Hkv * D if ks is None else ks, flags, None)


def _rope_name(sym, shape, rot=64, max_pos=1024, qs=None, ks=None, flags=0):
    B, H, Hkv, T, max_nq, _, ps, mp, D = shape
    return vl._rc_name(sym, B, H, Hkv, T, max_nq, ps, mp, D, rot, max_pos, H * D if qs is None else qs, Hkv * D if ks is None else ks, flags)


def test_header_symbols_and_exports_agree(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()

    def params(sym):
        m = re.search(r"\b" + sym + r"\(([^)]*)\)", header)
        assert m, sym
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]

    pairs = [RUN[k][:2] for k in RUN] + [NAME[k] for k in NAME] + [ROPE[k][:2] for k in ROPE] + [ROPE_NAME[k] for k in ROPE_NAME]
    assert len(pairs) == 8
    for twin, sym in pairs:
        assert hasattr(lib, sym), sym
        # argument for argument the fp16 entry: the same parameter list in the header, the same ctypes signature
        assert params(sym) == params(twin), sym
        assert capi.SYMBOLS[sym] == capi.SYMBOLS[twin], sym
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays
    for sym in ("lc_attn_varlen_paged_bf16_workspace_bytes", "lc_attn_varlen_paged_kv8_bf16_workspace_bytes",      # the fp16 queries serve both
                "lc_kv_append_paged_bf16", "lc_attn_decode_paged_bf16", "lc_attn_local_paged_bf16", "lc_rope_append_paged_bf16"):
        assert not hasattr(lib, sym), sym
        assert sym not in capi.SYMBOLS


@pytest.mark.parametrize("kind", list(RUN))
def test_every_bad_argument_gets_the_status_of_the_fp16_twin(built, kind):
    """tests/test_abi_cpu_varlen.py::test_statuses_and_their_order, case for case, on both entries"""
    twin, sym, nptr = RUN[kind]
    tname, sname = NAME[kind]
    seen = []

    def both(want, shape, w, flags, **kw):
        got = [_run(s, nptr, shape, w, flags, **kw) for s in (twin, sym)]
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


@pytest.mark.parametrize("kind", list(RUN))
def test_a_small_or_misaligned_workspace_is_refused_as_the_fp16_twin_refuses_it(knobs, kind):
    """the existing workspace query serves both element types: a bf16 call needs the fp16 call's bytes"""
    twin, sym, nptr = RUN[kind]
    capi.tune("attn_decode_split", 4)
    for shape in ((2, 8, 2, 90, 40, 70, 16, 64, 128), (2, 8, 2, 9, 4, 70, 16, 64, 64)):      # RB = 3 and RB = 1
        B, H, Hkv, T, mq, _, ps, mp, D = shape
        need = getattr(capi.load(), BYTES[kind])(B, H, Hkv, T, mq, ps, mp, D, 33)
        assert need == 4 * (T * H) * (D + 1) * 4
        for s in (twin, sym):
            for nb in (0, 16, need - 1):
                assert _run(s, nptr, shape, 33, CAUSAL, ws=(C.c_void_p(256), nb)) == capi.LC_ERR_ARG, (s, nb)
            assert _run(s, nptr, shape, 33, CAUSAL, ws=(C.c_void_p(8), need)) == capi.LC_ERR_ARG, s


@pytest.mark.parametrize("kind", list(ROPE))
def test_every_bad_rope_argument_gets_the_status_of_the_fp16_twin(built, kind):
    """tests/test_abi_cpu_varlen.py::test_rope_statuses_and_their_order, case for case, on both entries"""
    twin, sym, nptr = ROPE[kind]
    tname, sname = ROPE_NAME[kind]

    def both(want, shape, **kw):
        got = [_rope(s, nptr, shape, **kw) for s in (twin, sym)]
        assert got == [want, want], (shape, kw, got)

    def both_names(want, shape, **kw):
        got = [_rope_name(s, shape, **kw)[0] for s in (tname, sname)]
        assert got == [want, want], (shape, kw, got)

    mid = "_kv8" if kind == "kv8" else ""
    assert _rope_name(sname, OK) == (capi.LC_OK, f"rope_append_varlen{mid}_bf16_kernel<128,false>")
    assert _rope_name(sname, OK, flags=capi.ROPE_INTERLEAVED) == (capi.LC_OK, f"rope_append_varlen{mid}_bf16_kernel<128,true>")
    assert _rope_name(sname, (2, 8, 2, 40, 20, 70, 16, 64, 64), rot=32)[1] == f"rope_append_varlen{mid}_bf16_kernel<64,false>"
    both_names(capi.LC_OK, OK, qs=(8 + 4) * 128, ks=(8 + 4) * 128)      # three pointers into one projection output
    for flags in (capi.ROPE_PACKED_SRC, capi.ROPE_PACKED_SRC | capi.ROPE_INTERLEAVED, 4):
        both(capi.LC_ERR_ARG, BAD, flags=flags)
        both_names(capi.LC_ERR_ARG, OK, flags=flags)
    for i in range(10):                                             # Q, Knew, Vnew, Qout, the pools, cos_sin, cu_q, block_table, kv_len
        ptrs = [P] * nptr
        ptrs[i] = None
        both(capi.LC_ERR_ARG, BAD, ptrs=ptrs)
    for T, mq in ((0, 1), (40, 0), (40, 41)):
        both(capi.LC_ERR_SHAPE, (2, 8, 2, T, mq, 70, 16, 64, 96))
        both_names(capi.LC_ERR_SHAPE, (2, 8, 2, T, mq, 70, 16, 64, 96))
    for qs, ks in ((8 * 128 - 8, None), (8 * 128 + 4, None), (None, 2 * 128 - 8), (None, 2 * 128 + 2)):
        both(capi.LC_ERR_SHAPE, OK, qs=qs, ks=ks)
        both_names(capi.LC_ERR_SHAPE, OK, qs=qs, ks=ks)
    for rot in (0, 8, 24, 144):
        both(capi.LC_ERR_SHAPE, OK, rot=rot)
    both(capi.LC_ERR_SHAPE, OK, qs=8 * 128 + 8)                     # in place (Q == Qout on the dummy pointers) needs the dense layout
    mis = [P] * nptr
    mis[3] = C.c_void_p(8)
    both(capi.LC_ERR_SHAPE, (2, 8, 2, 40, 20, 70, 16, 64, 96), ptrs=mis)
    both_names(capi.LC_ERR_HEADDIM, (2, 8, 2, 40, 20, 70, 16, 64, 96))
    for s in (tname, sname):
        assert getattr(capi.load(), s)(2, 8, 2, 40, 20, 16, 64, 128, 64, 1024, 1024, 256, 0, None, 128) == capi.LC_ERR_ARG


def test_the_name_calls_report_the_fp16_plan_with_the_bf16_kernel(knobs):
    """<D,RT>, the chunk kernel past 64 rows and the " xS" suffix are the twin's — forced S and the automatic rule at two CU counts"""
    seen = set()
    for D in vl.DS:
        for H, Hkv, mq in ((8, 2, 1), (8, 2, 4), (8, 2, 5), (8, 2, 9), (8, 2, 16), (8, 2, 17), (8, 2, 130), (2, 2, 64), (2, 2, 65), (64, 1, 2)):
            for s in (1, 3, 64):
                capi.tune("attn_decode_split", s)
                for kind in vl.KINDS:
                    for B, T in ((1, 130), (6, 174)):
                        for w, flags in ((0, 0), (0, CAUSAL), (100, CAUSAL)):
                            shape = (B, H, Hkv, T, mq, 1, 16, vl.NCAP // 16, D)
                            rc, twin = _name(NAME[kind][0], shape, w, flags)
                            assert rc == capi.LC_OK and twin == vl.want_name(kind, H, Hkv, mq, D, s)
                            assert _name(NAME[kind][1], shape, w, flags) == (capi.LC_OK, bl.want_name(kind, H, Hkv, mq, D, s)), (kind, H, mq, w)
                            seen.add(re.sub(r"<.*", "", twin))
    assert len(seen) == 4
    capi.tune("attn_decode_split", 0)
    for cus in (64, 304):
        capi.tune("rule_cus", cus)
        for B, H, Hkv, T, mq, ncap, D in ((64, 32, 8, 64, 1, 4096, 128), (64, 32, 8, 575, 512, 4096, 128), (1, 8, 2, 40, 1, 32768, 64)):
            for w in (0, 200):
                s = vl.auto_split(B, H, Hkv, T, mq, ncap, w, cus)
                for kind in vl.KINDS:
                    got = _name(NAME[kind][1], (B, H, Hkv, T, mq, 1, 16, ncap // 16, D), w, CAUSAL)
                    assert got == (capi.LC_OK, bl.want_name(kind, H, Hkv, mq, D, s)), (cus, B, T, mq, w)
    capi.tune("rule_cus", 0)
    capi.tune("attn_decode_split", 1)
    assert capi.attn_varlen_paged_bf16_kernel_name(1, 8, 2, 40, 17, 16, 64, 128) == "attn_varlen_chunk_paged_bf16_kernel<128>"
    assert capi.attn_varlen_paged_bf16_kernel_name(1, 8, 2, 40, 5, 16, 64, 64, causal=True, window=9, kv8=True) == "attn_varlen_paged_kv8_bf16_kernel<64,2>"
    assert capi.rope_append_varlen_bf16_kernel_name(2, 8, 2, 40, 20, 16, 64, 128, 64, 1024) == "rope_append_varlen_bf16_kernel<128,false>"
    assert capi.rope_append_varlen_bf16_kernel_name(2, 8, 2, 40, 20, 16, 64, 64, 64, 1024, interleaved=True, kv8=True) == \
        "rope_append_varlen_kv8_bf16_kernel<64,true>"


def test_audit_knows_the_bf16_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    for unit, mid, extra in (("tu_attn_varlen_paged_bf16", "_paged", 2), ("tu_attn_varlen_paged_kv8_bf16", "_paged_kv8", 0)):
        rep = json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text())
        names = " ".join(r["kernel"] for r in rep)
        for d in (64, 128):
            assert f"attn_varlen_chunk{mid}_bf16_kernelILi{d}EE" in names, (unit, d)
            for rt in (1, 2, 4):
                assert f"attn_varlen{mid}_bf16_kernelILi{d}ELi{rt}EE" in names, (unit, d, rt)
            assert (f"attn_varlen_combine_bf16_kernelILi{d}EE" in names) == (extra == 2)
        assert len(rep) == 8 + extra
    rep_rope = json.loads((obj / build.AUDIT_OWN_REPORT["tu_rope_append_varlen_bf16"]).read_text())
    names = " ".join(r["kernel"] for r in rep_rope)
    for d in (64, 128):
        for il in (0, 1):
            assert f"rope_append_varlen_bf16_kernelILi{d}ELb{il}EE" in names and f"rope_append_varlen_kv8_bf16_kernelILi{d}ELb{il}EE" in names
    assert len(rep_rope) == 8
    for unit in ("tu_attn_varlen_paged_bf16", "tu_attn_varlen_paged_kv8_bf16", "tu_rope_append_varlen_bf16"):
        for r in json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text()):
            assert "bf16_kernel" in r["kernel"], r["kernel"]         # no fp16 kernel is instantiated a second time in a bf16 unit
            assert r["scratch"] == 0 and not r["violations"], r
            assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]                       # plain HIP: listed for rule R2 only
            assert r["asm_loads"] == 0
    # the fp16 ragged units keep their kernels and know nothing of the new ones
    for unit, n in (("tu_attn_varlen_paged", 10), ("tu_attn_varlen_paged_kv8", 8), ("tu_rope_append_varlen", 8)):
        text = (obj / build.AUDIT_OWN_REPORT[unit]).read_text()
        assert "bf16" not in text and len(json.loads(text)) == n, unit


def test_capi_wrappers_want_bfloat16_and_nothing_else(built):
    T, H, Hkv, D = 12, 8, 2, 64
    g = torch.Generator().manual_seed(1)
    q = torch.randn(T, H, D, generator=g).to(BF)
    o = torch.empty_like(q)
    _, k, v = dl.decode_inputs(3, H, Hkv, 1, 128, D, seed=1)
    kp, vp, table = dl.paginate(k.to(BF), v.to(BF), (100, 17, 5), 16, seed=2)
    kp8, vp8 = (x.view(torch.uint8)[..., :64].contiguous() for x in (kp, vp))
    lens = torch.tensor([100, 17, 5], dtype=torch.int32)
    cu = torch.tensor([0, 5, 5, 12], dtype=torch.int32)
    calls = (lambda **kw: capi.attn_varlen_paged_bf16(kw.pop("q", q), kw.pop("kp", kp), kw.pop("vp", vp), kw.pop("o", o), kw.pop("cu", cu), table,
                                                      lens, kw.pop("max_nq", 7), causal=True, **kw),
             lambda **kw: capi.attn_varlen_paged_kv8_bf16(kw.pop("q", q), kp8, vp8, kw.pop("o", o), kw.pop("cu", cu), table, lens,
                                                          kw.pop("max_nq", 7), causal=True, **kw))
    for call in calls:
        for wrong in (torch.half, torch.float32):
            with pytest.raises(TypeError, match="bfloat16"):
                call(q=q.to(wrong))
            with pytest.raises(TypeError, match="bfloat16"):
                call(o=o.to(wrong))
        with pytest.raises(ValueError, match="window"):
            call(window=-1)
        with pytest.raises(ValueError, match="max_nq"):
            call(max_nq=T + 1)
        with pytest.raises(TypeError, match="sinks must be float32"):
            call(sinks=torch.zeros(8, dtype=BF))
        for bad in (dict(cu=cu[:3]), dict(q=q.view(1, T, H, D)), dict(o=o[:T - 1])):
            with pytest.raises(RuntimeError, match="Tensor size mismatch"):
                call(**bad)
        with pytest.raises(RuntimeError, match="MI355X"):           # everything checked: only the device is missing
            call(window=3, sinks=torch.zeros(8))
    with pytest.raises(TypeError, match="bfloat16"):
        calls[0](kp=kp.half(), vp=vp.half())
    with pytest.raises(TypeError, match="bfloat16"):
        capi.attn_varlen_paged_bf16(q, kp8, vp8, o, cu, table, lens, 7)
    with pytest.raises(TypeError, match="float8_e4m3fn or uint8"):
        capi.attn_varlen_paged_kv8_bf16(q, kp, vp, o, cu, table, lens, 7)
    # the fp16 wrappers still refuse bf16, in their own words
    with pytest.raises(TypeError, match="float16"):
        capi.attn_varlen_paged(q, kp, vp, o, cu, table, lens, 7)
    # the rope call
    cs = capi.rope_table(128, D)
    qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=g).to(BF)
    qv, kv, vv = qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D), qkv[:, (H + Hkv) * D:].view(T, Hkv, D)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.rope_append_varlen_bf16(qv, kv, vv, kp, vp, cs, cu, table, lens, 7)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.rope_append_varlen_kv8_bf16(qv, kv, vv, kp8, vp8, cs, cu, table, lens, 7, k_scale=torch.ones(2), v_scale=torch.ones(2))
    for wrong in (torch.half, torch.float32):
        with pytest.raises(TypeError, match="bfloat16"):
            capi.rope_append_varlen_bf16(qv.to(wrong), kv.to(wrong), vv.to(wrong), kp, vp, cs, cu, table, lens, 7)
        with pytest.raises(TypeError, match="bfloat16"):
            capi.rope_append_varlen_kv8_bf16(qv.to(wrong), kv.to(wrong), vv.to(wrong), kp8, vp8, cs, cu, table, lens, 7)
        with pytest.raises(TypeError, match="bfloat16"):
            capi.rope_append_varlen_bf16(qv, kv, vv, kp, vp, cs, cu, table, lens, 7, q_out=torch.empty(T, H, D, dtype=wrong))
    with pytest.raises(TypeError, match="bfloat16"):
        capi.rope_append_varlen_bf16(qv, kv, vv, kp.half(), vp.half(), cs, cu, table, lens, 7)
    with pytest.raises(TypeError, match="bfloat16"):
        capi.rope_append_varlen_bf16(qv, kv, vv, kp8, vp8, cs, cu, table, lens, 7)
    with pytest.raises(TypeError, match="float32"):
        capi.rope_append_varlen_bf16(qv, kv, vv, kp, vp, cs.to(BF), cu, table, lens, 7)      # the table stays fp32
    with pytest.raises(RuntimeError, match="in place"):
        capi.rope_append_varlen_bf16(qv, kv, vv, kp, vp, cs, cu, table, lens, 7, q_out=qv)
    with pytest.raises(ValueError, match="max_nq"):
        capi.rope_append_varlen_bf16(qv, kv, vv, kp, vp, cs, cu, table, lens, T + 1)
    with pytest.raises(TypeError, match="float16"):
        capi.rope_append_varlen(qv, kv, vv, kp, vp, cs, cu, table, lens, 7)


# ------------------------------------------------------------------------------------------------------------------------------------
# what the GPU module's checks rest on

def test_half_ulp_bf16_is_half_the_spacing_of_the_bf16_values():
    a = torch.tensor([1.0, 1.99, 2.0, 3.0e38, 1e-30, 2.0 ** -126, 2.0 ** -130, 0.0], dtype=torch.float64)
    want = [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** (127 - 8), 2.0 ** (-100 - 8), 2.0 ** -134, 2.0 ** -134, 2.0 ** -134]
    assert bl.half_ulp_bf16(a).tolist() == want
    # against the format itself: the distance from a bf16 value to its upper neighbour is two half ulps
    x = torch.tensor([1.0, 1.5, 100.0, 2.0 ** -126, 2.0 ** -133, 0.0]).to(BF)
    up = (x.view(torch.int16) + 1).view(BF)
    assert torch.equal((up.double() - x.double()), 2 * bl.half_ulp_bf16(x.double()))
    # a correctly rounded value never leaves the bound, one a whole ulp off does
    g = torch.Generator().manual_seed(8)
    exact = torch.randn(4096, generator=g, dtype=torch.float64) * torch.pow(torch.tensor(2.0, dtype=torch.float64),
                                                                          torch.randint(-60, 60, (4096,), generator=g).double())
    exact = exact.float().double()                                  # fp32 values: one rounding on the way to bf16
    zero = torch.zeros_like(exact)
    got = exact.float().to(BF)
    assert not bl.rope_violations(got, exact, zero).any()
    off = (got.view(torch.int16) + 1).view(BF)
    assert bl.rope_violations(off, exact, zero).all()


def test_every_e4m3_value_is_a_bf16_value_and_the_sentinels_are_bf16_values():
    codes = dl.FINITE_CODES
    for s in dl.K_SCALES + dl.V_SCALES:
        assert torch.equal(bl.dequant_bf16(codes, s).double(), dl.OCP[codes.long()].double() * s)
        assert torch.equal(dl.quantize(bl.dequant_bf16(codes, s), s), codes)                 # and back: the code a bf16 pool would quantise to
    assert float(torch.tensor(bl.SENTINEL).to(BF)) == bl.SENTINEL
    assert torch.isfinite(torch.tensor([bl.SENT16], dtype=torch.int16).view(BF)).all()


def test_token_positions_and_pool_rows_restate_the_append_rule():
    cu, lens, T = [0, 3, 3, 10], (40, 9, 5), 12
    seq, pos = bl.token_positions(cu, lens, T, 7)
    assert seq.tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 2, 2, -1, -1]
    assert pos[:3].tolist() == [37, 38, 39] and pos[3:10].tolist() == [-2, -1, 0, 1, 2, 3, 4]
    _, k, v = dl.decode_inputs(3, 8, 2, 1, 64, 64, seed=4)
    kp, _, table = dl.paginate(k.to(BF), v.to(BF), (40, 9, 5), 16, seed=3)
    rows = bl.pool_rows(kp, table, seq, pos)
    assert torch.equal(rows[1], k.to(BF)[0, :, 38]) and torch.equal(rows[9], k.to(BF)[2, :, 4])
    w = bl.written_mask(kp, table, seq, pos)
    assert int(w.sum()) == 2 * (3 + 5)
