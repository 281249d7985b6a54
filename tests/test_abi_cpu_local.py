"""CPU tests of sliding-window / attention-sink attention's boundary (lc_attn_local_f16 / _paged_f16 / _paged_kv8 and their name and workspace
calls; no call here reaches a device): the nine exports and their argument counts, the two new error statuses and where they stand in the order
of the checks, the name grid, window = 0 without sinks named and sized as the chunk call, the split rule's dependence on the window and on
nothing else new, the audit reports of the three new units, the Python wrappers' checks — and the float64 reference of the GPU tests against
decode_lib.softmax64, with its low edge and sink term checked by hand.

Inputs, truth and plan restatement are shared with tests/test_gpu_local.py: tests/local_lib.py (on top of tests/decode_lib.py)."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import chunk_lib as cl
from tests import decode_lib as dl
from tests import local_lib as ll

P = C.c_void_p(16)
CAUSAL = capi.ATTN_CAUSAL
# per kind: (run symbol, pointers in front of the shape, ints between the pointers and `window`)
RUN = {"flat": ("lc_attn_local_f16", 5, 6), "paged": ("lc_attn_local_paged_f16", 6, 8), "kv8": ("lc_attn_local_paged_kv8", 8, 8)}
QUERY = {"flat": "lc_attn_local", "paged": "lc_attn_local_paged", "kv8": "lc_attn_local_paged_kv8"}


@pytest.fixture
def knobs(built):
    yield from dl.reset_knobs()


def _geo(kind):
    return (1000,) if kind == "flat" else (70, 16, 64)


def _run(kind, shape, window, flags, sinks=None, ptrs=None, ws=(None, 0)):
    """status of the run call on dummy pointers (only ever used on calls a check refuses: nothing reaches a device)"""
    sym, nptr, _ = RUN[kind]
    if ptrs is None:
        ptrs = [P] * nptr
    return getattr(capi.load(), sym)(*ptrs, *shape, window, sinks, flags, *ws, None)


def _name(kind, shape, window, flags):
    B, H, Hkv, Nq, *geo, D = shape
    if kind == "flat":
        return ll._rc_name("lc_attn_local_kernel_name", B, H, Hkv, Nq, geo[0], D, window, flags)
    return ll._rc_name(QUERY[kind] + "_kernel_name", B, H, Hkv, Nq, geo[1], geo[2], D, window, flags)


def test_the_nine_symbols_are_exported_with_their_argument_counts(built):
    lib = C.CDLL(str(built["abi"]))
    header = (Path(__file__).resolve().parent.parent / "include" / "lc_abi.h").read_text()
    want = {}
    for kind, (sym, nptr, nint) in RUN.items():
        want[sym] = nptr + nint + 1 + 1 + 1 + 3                    # pointers, ints, window, sinks, flags, workspace + bytes + stream
        want[QUERY[kind] + "_workspace_bytes"] = nint - (kind != "flat") + 1
        want[QUERY[kind] + "_kernel_name"] = nint - (kind != "flat") + 1 + 1 + 2
    assert len(want) == 9
    for sym, n in want.items():
        assert hasattr(lib, sym), sym
        m = re.search(r"\b" + sym + r"\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == n == len(capi.SYMBOLS[sym][1]), (sym, n)
        params = [p.strip() for p in m.group(1).split(",")]
        if sym in (r[0] for r in RUN.values()):                     # window, sinks right in front of flags
            i = params.index("int flags")
            assert params[i - 2:i] == ["int window", "const float* sinks"], sym
    assert lib.lc_abi_version() == 2                                # additive: the ABI version stays


@pytest.mark.parametrize("kind", list(RUN))
def test_new_errors_and_their_place_in_the_order(built, kind):
    geo = _geo(kind)
    ok = (1, 8, 2, 4, *geo, 128)
    bad_shape = (1, 8, 3, 4, *geo, 256)
    nreq = 4 if kind == "flat" else 6
    # the two new statuses, run call and name call, with and without sinks
    for sinks in (None, P):
        for w in (-1, -4096, -(1 << 31)):
            for flags in (0, CAUSAL):
                assert _run(kind, ok, w, flags, sinks) == capi.LC_ERR_ARG, w
                assert _name(kind, ok, w, flags)[0] == capi.LC_ERR_ARG
        for w in (1, 64, (1 << 31) - 1):
            assert _run(kind, ok, w, 0, sinks) == capi.LC_ERR_ARG, w                       # a window without LC_ATTN_CAUSAL
            assert _name(kind, ok, w, 0)[0] == capi.LC_ERR_ARG
            assert _name(kind, ok, w, CAUSAL)[0] == capi.LC_OK
    assert getattr(capi.load(), QUERY[kind] + "_workspace_bytes")(*ok[:4], *ok[4 + (kind != "flat"):], -1) == 0
    # ... among the flag checks: before null pointers, shape, alignment and head dim; an unknown flag and a bad window have the same status
    nul = [P] * RUN[kind][1]
    nul[0] = None
    for w, flags in ((-1, CAUSAL), (5, 0), (5, capi.ATTN_V_TRANSPOSED), (0, 4)):
        assert _run(kind, ok, w, flags, ptrs=nul) == capi.LC_ERR_ARG
        assert _run(kind, bad_shape, w, flags) == capi.LC_ERR_ARG
        assert _name(kind, bad_shape, w, flags)[0] == capi.LC_ERR_ARG
        assert _run(kind, (1, 8, 2, 4, *geo, 96), w, flags) == capi.LC_ERR_ARG
    mis = [P] * RUN[kind][1]
    mis[1] = C.c_void_p(8)
    assert _run(kind, ok, -1, CAUSAL, ptrs=mis) == capi.LC_ERR_ARG
    # a good window changes nothing of the chunk entries' order: null pointer, shape, alignment, head dim, workspace
    for w, flags, sinks in ((0, 0, None), (0, 0, P), (7, CAUSAL, None), (7, CAUSAL, P)):
        for i in range(nreq):
            ptrs = [P] * RUN[kind][1]
            ptrs[i] = None
            assert _run(kind, bad_shape, w, flags, sinks, ptrs=ptrs) == capi.LC_ERR_ARG, i
        assert _run(kind, bad_shape, w, flags, sinks) == capi.LC_ERR_SHAPE
        assert _run(kind, (1, 8, 2, 40, *geo, 96), w, flags, sinks, ptrs=mis) == capi.LC_ERR_SHAPE
        assert _run(kind, (1, 8, 2, 40, *geo, 96), w, flags, sinks) == capi.LC_ERR_HEADDIM    # R > 64 is no error: the head dim is
        assert _name(kind, (1, 8, 2, 40, *geo, 96), w, flags)[0] == capi.LC_ERR_HEADDIM
        assert _run(kind, (1, 8, 2, 40, *geo, 96), w, flags, sinks, ws=(C.c_void_p(256), 0)) == capi.LC_ERR_HEADDIM
    name_sym = getattr(capi.load(), QUERY[kind] + "_kernel_name")
    dims = ok[:4] + ok[4 + (kind != "flat"):]
    assert name_sym(*dims, 0, 0, None, 128) == capi.LC_ERR_ARG
    assert name_sym(*dims, 0, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG


@pytest.mark.parametrize("kind", list(RUN))
def test_a_small_or_misaligned_workspace_is_refused_before_any_device_work(knobs, kind):
    capi.tune("attn_decode_split", 4)
    for shape in ((1, 8, 2, 40, *_geo(kind), 128), (1, 8, 2, 4, *_geo(kind), 64)):      # R = 160 and R = 16
        B, H, _, Nq = shape[:4]
        need = ll.nbytes(kind, B, H, 2, Nq, shape[-1], 33, ncap=1024 if kind != "flat" else 1000)
        assert need == 4 * (B * H * Nq) * (shape[-1] + 1) * 4
        for sinks in (None, P):
            for nb in (0, 16, need - 1):
                assert _run(kind, shape, 33, CAUSAL, sinks, ws=(C.c_void_p(256), nb)) == capi.LC_ERR_ARG, nb
            assert _run(kind, shape, 33, CAUSAL, sinks, ws=(C.c_void_p(8), need)) == capi.LC_ERR_ARG


def test_name_grid(knobs):
    """RB = 1 (every RT) / RB > 1 x three caches x D x forced S; window = 0 names the chunk call (R <= 64: the decode call)"""
    for D in ll.DS:
        for H, Hkv, Nq in ((8, 1, 1), (8, 2, 5), (8, 2, 9), (2, 2, 64), (2, 2, 65), (4, 2, 48), (64, 1, 2)):
            for s in (1, 3, 64):
                capi.tune("attn_decode_split", s)
                for kind in ll.KINDS:
                    for B in (1, 3):
                        for w in (1, 100, 1 << 20):
                            assert ll.name(kind, B, H, Hkv, Nq, D, w, CAUSAL) == (capi.LC_OK, ll.want_name(kind, H, Hkv, Nq, D, s)), (kind, H, Nq, w)
                        for flags in (0, CAUSAL):
                            assert ll.name(kind, B, H, Hkv, Nq, D, 0, flags) == (capi.LC_OK, ll.want_name(kind, H, Hkv, Nq, D, s, local=False))
    assert capi.attn_local_kernel_name(1, 8, 2, 5, 1000, 128, causal=True, window=9) == "attn_local_kernel<128,2> x64"
    assert capi.attn_local_paged_kernel_name(1, 8, 2, 40, 16, 64, 64, causal=True, window=9) == "attn_local_chunk_paged_kernel<64> x64"
    assert capi.attn_local_paged_kv8_kernel_name(1, 8, 2, 5, 16, 64, 64, causal=True, window=9) == "attn_local_paged_kv8_kernel<64,2> x64"


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_no_window_and_no_sinks_is_the_chunk_call(knobs, cus):
    """the chunk call's name and workspace bytes, under the auto rule and under a forced split"""
    capi.tune("rule_cus", cus)
    for s in (0, 1, 3):
        capi.tune("attn_decode_split", s)
        for B, H, Hkv, Nq, D in ((1, 32, 8, 1, 128), (3, 8, 2, 5, 64), (2, 4, 4, 64, 64), (1, 8, 2, 40, 128), (2, 2, 1, 130, 64)):
            for causal in (False, True):
                for ncap in (1024, 8192):
                    assert capi.attn_local_kernel_name(B, H, Hkv, Nq, ncap, D, causal=causal) == capi.attn_chunk_kernel_name(B, H, Hkv, Nq, ncap, D, causal=causal)
                    assert capi.attn_local_workspace_bytes(B, H, Hkv, Nq, ncap, D) == capi.attn_chunk_workspace_bytes(B, H, Hkv, Nq, ncap, D)
                    for ps in (16, 256):
                        mp = ncap // ps
                        assert (capi.attn_local_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=causal)
                                == capi.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=causal))
                        assert (capi.attn_local_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=causal)
                                == capi.attn_chunk_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=causal))
                        assert capi.attn_local_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == capi.attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D)
                        assert (capi.attn_local_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D)
                                == capi.attn_chunk_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D))


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_auto_split_rule_follows_the_window(knobs, cus):
    """S from (groups, the tiles of min(Ncap, W + Nq - 1 + 63) keys, the CU count) alone: the same for the three caches, the workspace that of
    the named S, and a window at least as long as the cache is the rule without one"""
    capi.tune("rule_cus", cus)
    seen = set()
    for B, H, Hkv, Nq, ncap, D in ((1, 32, 8, 1, 32768, 128), (8, 64, 8, 1, 32768, 64), (1, 8, 1, 1, 8192, 64), (1, 32, 8, 128, 4096, 128),
                                   (2, 2, 1, 130, 1 << 16, 128), (1, 1, 1, 1, 1 << 20, 64), (3, 8, 2, 5, 1024, 64)):
        groups = B * Hkv * cl.rb_of(H, Hkv, Nq)
        for w in (1, 64, 128, 200, 1000, 4096, ncap, (1 << 31) - 1):
            s = ll.auto_split(groups, ncap, Nq, w, cus)
            seen.add(s)
            assert s <= dl.auto_split(groups, ncap, cus)
            if w >= ncap:
                assert s == dl.auto_split(groups, ncap, cus)
            bytes_ = s * B * H * Nq * (D + 1) * 4 if s > 1 else 0
            for kind in ll.KINDS:
                assert ll.name(kind, B, H, Hkv, Nq, D, w, CAUSAL, ncap=ncap) == (capi.LC_OK, ll.want_name(kind, H, Hkv, Nq, D, s)), (kind, B, H, Nq, ncap, w)
                assert ll.nbytes(kind, B, H, Hkv, Nq, D, w, ncap=ncap) == bytes_
    assert len(seen) >= 4 and 1 in seen
    # the figures of the rule, by hand: W = 4096, Nq = 1 walks at most 4096 + 63 keys = 65 tiles -> at most 16 ranges; W = 128: 3 tiles -> 1
    if cus == 256:
        assert ll.auto_split(8, 32768, 1, 4096, cus) == 16 and dl.auto_split(8, 32768, cus) == 32
        assert ll.auto_split(1, 32768, 1, 4096, cus) == 16 and ll.auto_split(8, 32768, 1, 128, cus) == 1


def test_the_restated_plan_is_what_the_issue_states():
    assert ll.span(1000, 1, 1024, True, 64, 0) == (936, 1000) and ll.span(1000, 5, 1024, True, 64, 0) == (932, 996)
    assert ll.span(10, 1, 1024, True, 64, 0) == (0, 10) and ll.span(3, 5, 1024, True, 2, 0) == (0, 0) and ll.span(3, 5, 1024, True, 2, 4) == (1, 3)
    assert ll.span(1000, 5, 1024, False, 0, 0) == (0, 1000) and ll.span(1000, 5, 1024, True, 0, 2) == (0, 998)
    assert ll.tile_lo(1000, 1, 1024, 64) == 14 and ll.tile_lo(1000, 1, 1024, 360) == 10 and ll.tile_lo(1000, 1, 1024, 0) == 0
    assert ll.tile_lo(1000, 17, 1024, 64) == (1000 - 17 + 1 - 64) // 64 and ll.tile_lo(50, 1, 1024, 64) == 0
    assert ll.tile_lo(1000, 48, 1024, 100, i_min=16) == (1000 - 48 + 16 + 1 - 100) // 64
    for place, (e0, _) in ll.EDGE_PLACES.items():
        for Nq in (1, 9, 17, 48):
            w, _ = ll.edge_window(place, Nq)
            assert ll.span(1000, Nq, 1024, True, w, 0)[0] == (e0 or 0), (place, Nq)


def test_audit_knows_the_local_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    for unit, mid in (("tu_attn_local", ""), ("tu_attn_local_paged", "_paged"), ("tu_attn_local_paged_kv8", "_paged_kv8")):
        rep = json.loads((obj / build.AUDIT_OWN_REPORT[unit]).read_text())
        names = " ".join(r["kernel"] for r in rep)
        for d in (64, 128):
            assert f"attn_local_chunk{mid}_kernelILi{d}EE" in names, (unit, d)
            for rt in (1, 2, 4):
                assert f"attn_local{mid}_kernelILi{d}ELi{rt}EE" in names, (unit, d, rt)
        assert len(rep) == 8
        for r in rep:
            assert "attn_decode" not in r["kernel"] and "attn_chunk" not in r["kernel"]      # the other reports are read by those strings
            assert r["scratch"] == 0 and not r["violations"], r
            assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]                       # plain HIP: listed for rule R2 only
            assert r["asm_loads"] == 0
    # the existing reports keep their entry counts and know nothing of the new units
    counts = {"isa_audit.json": None, build.AUDIT_OWN_REPORT["tu_attn_decode_paged"]: 6, build.AUDIT_OWN_REPORT["tu_attn_decode_paged_kv8"]: 6,
              build.AUDIT_OWN_REPORT["tu_attn_chunk"]: 6}
    for other, n in counts.items():
        text = (obj / other).read_text()
        assert "attn_local" not in text, other
        assert n is None or len(json.loads(text)) == n, other


def test_capi_wrappers_check_window_and_sinks_without_a_gpu(built):
    q, k, v = dl.decode_inputs(2, 8, 2, 5, 128, 64, seed=1)
    o = torch.empty_like(q)
    lens = torch.tensor([100, 17], dtype=torch.int32)
    kp, vp, table = dl.paginate(k, v, (100, 17), 16, seed=2)
    kp8, vp8 = (x.view(torch.uint8)[..., :64].contiguous() for x in (kp, vp))
    calls = (lambda **kw: capi.attn_local(q, k, v, o, lens, causal=True, **kw),
             lambda **kw: capi.attn_local_paged(q, kp, vp, o, table, lens, causal=True, **kw),
             lambda **kw: capi.attn_local_paged_kv8(q, kp8, vp8, o, table, lens, causal=True, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="window"):
            call(window=-1)
        with pytest.raises(ValueError, match="window"):
            call(window=1.5)
        with pytest.raises(TypeError, match="sinks must be float32"):
            call(sinks=torch.zeros(8, dtype=torch.half))
        for bad in (torch.zeros(2), torch.zeros(8, 1), torch.zeros(5)):                     # Hkv, a 2-D tensor, Nq elements: not H
            with pytest.raises(RuntimeError, match="Tensor size mismatch"):
                call(sinks=bad)
        with pytest.raises(RuntimeError, match="MI355X"):                                   # everything checked: only the device is missing
            call(window=3, sinks=torch.zeros(8))
    with pytest.raises(TypeError, match="float8_e4m3fn or uint8"):
        capi.attn_local_paged_kv8(q, kp, vp, o, table, lens, window=3, causal=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference of the GPU tests

def test_local64_without_window_and_sinks_is_softmax64():
    q, k, v = dl.decode_inputs(3, 8, 2, 5, 256, 64, seed=11)
    lens = (256, 129, 3)
    for causal in (False, True):
        want, nk = dl.softmax64(q, k.double(), v.double(), lens, causal)
        got, nvis = ll.local64(q, k.double(), v.double(), lens, causal)
        assert (nvis == nk).all() and np.abs(got - want).max() <= 1e-13
        got, nvis = ll.local64(q, k.double(), v.double(), lens, causal, sinks=torch.full((8,), -float("inf")))
        assert (nvis == nk).all() and np.abs(got - want).max() <= 1e-13
    got, nvis = ll.local64(q, k.double(), v.double(), lens, True, window=1 << 20)
    want, nk = dl.softmax64(q, k.double(), v.double(), lens, True)
    assert (nvis == nk).all() and np.abs(got - want).max() <= 1e-13


def test_local64_low_edge_and_sink_by_hand():
    q, k, v = dl.decode_inputs(2, 4, 2, 3, 64, 64, seed=12)
    lens = (40, 2)
    sinks = torch.tensor([0.5, -1.0, 2.0, -float("inf")])
    got, nvis = ll.local64(q, k.double(), v.double(), lens, True, window=7, sinks=sinks)
    assert nvis.tolist() == [[7, 7, 7], [0, 1, 2]]
    for b, h, i in ((0, 0, 0), (0, 1, 2), (0, 3, 1), (1, 2, 1), (1, 2, 2), (1, 3, 0)):
        p = lens[b] - 3 + i
        keys = [j for j in range(64) if p - 7 < j <= p and j >= 0]
        assert len(keys) == nvis[b, i]
        if not keys:
            assert (got[b, h, i] == 0).all()
            continue
        s = torch.tensor([float(q[b, h, i].double() @ k[b, h // 2, j].double()) / 8.0 for j in keys], dtype=torch.float64)
        den = torch.exp(s).sum() + torch.exp(sinks[h].double())
        want = sum((torch.exp(s[n]) / den) * v[b, h // 2, j].double() for n, j in enumerate(keys))
        assert np.abs(got[b, h, i] - want.numpy()).max() <= 1e-12, (b, h, i)
    # window = 1: the row's own key; K = 0 with a sink of 0: half of it
    got, _ = ll.local64(q, k.double(), v.double(), (40, 40), True, window=1)
    assert np.abs(got[0, 3, 2] - v[0, 1, 39].double().numpy()).max() <= 1e-15
    got, _ = ll.local64(q, torch.zeros_like(k).double(), v.double(), (40, 40), True, window=1, sinks=torch.zeros(4))
    assert np.abs(got[0, 3, 1] - v[0, 1, 38].double().numpy() / 2).max() <= 1e-15


def test_the_pinned_edge_inputs_are_what_the_docstring_says():
    for shape in ((8, 1, 1), (8, 2, 9), (2, 1, 48)):
        H, Hkv, Nq = shape
        for place in ll.EDGE_PLACES:
            for below in (False, True):
                q, k, v, w, _ = ll.edge_inputs(64, shape, place, below)
                assert (k.abs() == 1).all() and torch.isfinite(v).all()
                for b, L in enumerate(ll.EDGE_LENS):
                    s = (q[b, H - 1].double() @ k[b, Hkv - 1].double().T) / 8.0          # [Nq, Ncap]
                    for i in range(Nq):
                        lo, hi = ll.span(L, Nq, ll.NCAP, True, w, i)
                        t = hi - w - 1 if below else lo
                        if t < 0:
                            assert below and place == "clipped"
                            continue
                        assert abs(s[i, t].item() - dl.SCORE) <= dl.SCORE * 2.0 ** -11 and s[i].argmax().item() == t
                        assert (t < lo) == below and (not below or v[b, 0, t, 0].item() == 8.0)
