"""CPU tests of chunked-prefill attention's boundary (lc_attn_chunk_f16 / _paged_f16 / _paged_kv8 and their name and workspace calls; no call here
reaches a device): the error codes and their order — the decode entries' tuples with R > 64 no longer an error —, the decode entries still
refusing R > 64, the name grid and the " xS" suffix, R <= 64 named as the decode entry names it, the split rule with B x Hkv x RB groups, the
workspace bytes, the exports, the audit report of the six new kernels — and a test of the GPU tests' pinned inputs: on them a row-block kernel
that takes a row's limit from the block-local row index, uses L_blk as every row's limit, ends a straddling block's walk at its last row's
limit, or loads block 0's Q rows in every block leaves the bound by >= 20 x on EVERY row it touches.

Inputs, truth and the wrong kernels are shared with tests/test_gpu_chunk.py: tests/chunk_lib.py (on top of tests/decode_lib.py)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from leetcuda_amd import capi
from tests import chunk_lib as cl
from tests import decode_lib as dl
from tests.decode_lib import TEETH, reset_knobs, visible


@pytest.fixture
def knobs(built):
    yield from reset_knobs()


P = C.c_void_p(16)
# per cache kind: (run symbol, pointers in front of the shape, decode run symbol, shape tuples are (B, H, Hkv, Nq, *geometry, D))
KINDS = {"": ("lc_attn_chunk_f16", 5, "lc_attn_decode_f16"), "_paged": ("lc_attn_chunk_paged_f16", 6, "lc_attn_decode_paged_f16"),
         "_paged_kv8": ("lc_attn_chunk_paged_kv8", 8, "lc_attn_decode_paged_kv8")}


def _run(kind, shape, flags=0, ptrs=None, ws=(None, 0), decode=False):
    """status of the run call on dummy pointers (only ever used on calls a check refuses: nothing reaches a device)"""
    sym, nptr, dec = KINDS[kind]
    ptrs = list(ptrs) if ptrs is not None else [P] * min(nptr, 6)
    if kind == "" and len(ptrs) == 4:
        ptrs.append(None)                     # kv_len: optional
    if kind == "_paged_kv8" and len(ptrs) == 6:
        ptrs += [P, P]                        # the scales: never checked
    return getattr(capi.load(), dec if decode else sym)(*ptrs, *shape, flags, *ws, None)


def _geom(kind, geometry_flat=(1000,), geometry_paged=(70, 16, 64)):
    return geometry_flat if kind == "" else geometry_paged


def _name(kind, shape, flags=0):
    """(status, name) of the name call; a paged shape tuple carries num_pages, which the name call does not take"""
    B, H, Hkv, Nq, *geo, D = shape
    if kind == "":
        return cl.name_flat(B, H, Hkv, Nq, geo[0], D, flags)
    return (cl.name_paged if kind == "_paged" else cl.name_kv8)(B, H, Hkv, Nq, geo[1], geo[2], D, flags)


def _bytes(kind, shape):
    B, H, Hkv, Nq, *geo, D = shape
    lib = capi.load()
    if kind == "":
        return lib.lc_attn_chunk_workspace_bytes(B, H, Hkv, Nq, geo[0], D)
    return getattr(lib, f"lc_attn_chunk{kind}_workspace_bytes")(B, H, Hkv, Nq, geo[1], geo[2], D)


@pytest.mark.parametrize("kind", list(KINDS))
def test_chunk_errors_and_their_order(built, kind):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    c, vt = capi.ATTN_CAUSAL, capi.ATTN_V_TRANSPOSED
    geo = _geom(kind)
    ok = (1, 8, 2, 4, *geo, 128)
    bad_shape = (1, 8, 3, 4, *geo, 256)
    nreq = 4 if kind == "" else 6             # Q, K, V, O (, block_table, kv_len)
    for flags in (0, c):
        for nul in range(nreq):
            ptrs = [P] * nreq
            ptrs[nul] = None
            assert _run(kind, ok, flags, ptrs) == capi.LC_ERR_ARG, nul
            assert _run(kind, bad_shape, flags, ptrs) == capi.LC_ERR_ARG                     # null pointer before shape and head dim
        for hkv in (0, -1, 3, 5, 9, 16):
            assert _run(kind, (1, 8, hkv, 4, *geo, 128), flags) == capi.LC_ERR_SHAPE, hkv
        shapes = [(0, 8, 2, 4, *geo, 128), (1, 0, 0, 4, *geo, 128), (1, 8, 2, 0, *geo, 128), (1, 8, 2, 4, *geo, 0), (1 << 24, 8, 8, 1, *geo, 64)]
        if kind == "":
            shapes += [(1, 8, 2, 4, 0, 128), (1, 8, 2, 4, -5, 128), (1, 8, 2, 4, 1 << 23, 128), (1, 8, 2, 4, 1 << 24, 64)]
        else:
            big = (1 << 19, 1 << 20) if kind == "_paged" else (1 << 20, 1 << 21)
            shapes += [(1, 8, 2, 4, 0, 16, 64, 128), (1, 8, 2, 4, -3, 16, 64, 128), (1, 8, 2, 4, 70, 16, 0, 128), (1, 8, 2, 4, 70, 16, -1, 128),
                       (1, 8, 2, 4, 70, 8, 64, 128), (1, 8, 2, 4, 70, 24, 64, 128), (1, 8, 2, 4, 70, 0, 64, 128), (1, 8, 2, 4, 70, -16, 64, 128),
                       (1, 8, 2, 4, 70, 1, 64, 128), (1, 8, 2, 4, 70, 48, 64, 128), (1, 8, 2, 4, 70, 16, big[0], 128),
                       (1, 8, 2, 4, 70, big[1], 16, 64), (1, 8, 2, 4, 70, 1 << 16, 1 << 16, 64)]
        for shape in shapes:
            assert _run(kind, shape, flags) == capi.LC_ERR_SHAPE, shape
            paged_num_pages_only = kind != "" and shape[4] <= 0                                # (the name call takes no num_pages)
            assert _name(kind, shape, flags)[0] == capi.LC_ERR_SHAPE or paged_num_pages_only, shape
            assert _bytes(kind, shape) == 0 or paged_num_pages_only
        # the decode entries' R > 64 tuples: not an error here (the name call: nothing is launched), and the decode entries still refuse them
        for B, H, Hkv, Nq, D in ((1, 8, 2, 17, 128), (1, 8, 8, 65, 64), (1, 64, 1, 2, 64)):
            shape = (B, H, Hkv, Nq, *geo, D)
            rc, name = _name(kind, shape, flags)
            assert rc == capi.LC_OK and name.startswith(f"attn_chunk{kind}_kernel<{D}>"), (shape, rc, name)
            assert _run(kind, shape, flags, decode=True) == capi.LC_ERR_SHAPE, shape
            assert _run(kind, (B, H, Hkv, Nq, *geo, 96), flags) == capi.LC_ERR_HEADDIM          # R > 64 is no error: the head dim is
            assert _name(kind, (B, H, Hkv, Nq, *geo, 96), flags)[0] == capi.LC_ERR_HEADDIM
            assert _run(kind, (B, H, Hkv, Nq, *geo, 96), flags, decode=True) == capi.LC_ERR_SHAPE
        # the grid bound counts the row blocks: B x Hkv x RB x 64 <= 2^31 - 1
        assert _name(kind, (1 << 19, 1, 1, 64 * 63, *geo, 64), flags)[0] == capi.LC_OK
        assert _name(kind, (1 << 19, 1, 1, 64 * 64, *geo, 64), flags)[0] == capi.LC_ERR_SHAPE
        assert _name(kind, (1, 1 << 15, 1, 1 << 16, *geo, 64), flags)[0] == capi.LC_ERR_SHAPE    # R = 2^31: computed in 64 bits
        assert _run(kind, bad_shape, flags) == capi.LC_ERR_SHAPE                                 # shape before head dim
        for mis in range(4):                                                                     # Q, K, V, O: 16-byte aligned
            ptrs = [P] * nreq
            ptrs[mis] = C.c_void_p(8)
            assert _run(kind, ok, flags, ptrs) == capi.LC_ERR_SHAPE, mis
            assert _run(kind, (1, 8, 2, 40, *geo, 96), flags, ptrs) == capi.LC_ERR_SHAPE          # alignment before head dim
        for d in (32, 96, 256, 512, 1024, 16, 48):
            assert _run(kind, (1, 8, 2, 4, *geo, d), flags) == capi.LC_ERR_HEADDIM, d
            assert _name(kind, (1, 8, 2, 4, *geo, d), flags)[0] == capi.LC_ERR_HEADDIM
            assert _bytes(kind, (1, 8, 2, 4, *geo, d)) == 0
    for bad in (vt, c | vt, 4, -1, 1 << 30):
        assert _run(kind, ok, bad) == capi.LC_ERR_ARG, bad
        assert _run(kind, bad_shape, bad) == capi.LC_ERR_ARG                                     # flags before everything
        assert _name(kind, ok, bad)[0] == capi.LC_ERR_ARG
        assert _name(kind, bad_shape, bad)[0] == capi.LC_ERR_ARG
    name_sym = getattr(lib, f"lc_attn_chunk{kind}_kernel_name")
    dims = ok[:4] + ok[4 + (kind != ""):]
    assert name_sym(*dims, 0, None, 128) == capi.LC_ERR_ARG
    assert name_sym(*dims, 0, C.create_string_buffer(4), 4) == capi.LC_ERR_ARG


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_small_or_misaligned_workspace_is_refused_before_any_device_work(knobs, kind):
    geo = _geom(kind)
    capi.tune("attn_decode_split", 4)
    shape = (1, 8, 2, 40, *geo, 128)          # R = 160
    need = _bytes(kind, shape)
    assert need == 4 * (1 * 8 * 40) * 129 * 4
    for nbytes in (0, 16, need - 1):
        assert _run(kind, shape, 0, ws=(C.c_void_p(256), nbytes)) == capi.LC_ERR_ARG, nbytes
    assert _run(kind, shape, 0, ws=(C.c_void_p(8), need)) == capi.LC_ERR_ARG
    assert _run(kind, (1, 8, 2, 40, *geo, 96), 0, ws=(C.c_void_p(256), 0)) == capi.LC_ERR_HEADDIM      # head dim before the workspace


def test_name_grid_and_split_suffix(knobs):
    for D in cl.DS:
        for H, Hkv, Nq in cl.SHAPES + ((32, 8, 512), (8, 8, 65), (8, 2, 16), (8, 2, 4), (2, 2, 64), (2, 2, 33)):
            for flags in (0, capi.ATTN_CAUSAL):
                for s in (1, 2, 3, 8, 64):
                    capi.tune("attn_decode_split", s)
                    for B in (1, 3):
                        bytes_ = s * B * H * Nq * (D + 1) * 4 if s > 1 else 0
                        assert cl.name_flat(B, H, Hkv, Nq, cl.NCAP, D, flags) == (capi.LC_OK, cl.want_name("", H, Hkv, Nq, D, s))
                        assert capi.attn_chunk_kernel_name(B, H, Hkv, Nq, cl.NCAP, D, causal=bool(flags)) == cl.want_name("", H, Hkv, Nq, D, s)
                        assert capi.attn_chunk_workspace_bytes(B, H, Hkv, Nq, cl.NCAP, D) == bytes_
                        for ps, mp in ((16, 64), (256, 4)):
                            assert cl.name_paged(B, H, Hkv, Nq, ps, mp, D, flags) == (capi.LC_OK, cl.want_name("_paged", H, Hkv, Nq, D, s))
                            assert cl.name_kv8(B, H, Hkv, Nq, ps, mp, D, flags) == (capi.LC_OK, cl.want_name("_paged_kv8", H, Hkv, Nq, D, s))
                            assert capi.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D, causal=bool(flags)) == cl.want_name("_paged", H, Hkv, Nq, D, s)
                            assert capi.attn_chunk_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D) == cl.want_name("_paged_kv8", H, Hkv, Nq, D, s)
                            assert capi.attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == bytes_
                            assert capi.attn_chunk_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D) == bytes_


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_up_to_64_rows_a_chunk_entry_names_the_decode_call(knobs, cus):
    """R <= 64: the decode entry's name and bytes, under the auto rule and under a forced split"""
    capi.tune("rule_cus", cus)
    for s in (0, 1, 3):
        capi.tune("attn_decode_split", s)
        for B, H, Hkv, Nq, D in ((1, 32, 8, 1, 128), (16, 32, 8, 4, 128), (3, 8, 2, 5, 64), (2, 4, 4, 64, 64), (1, 64, 1, 1, 128), (2, 8, 2, 16, 128)):
            assert cl.rows_of(H, Hkv, Nq) <= 64
            for ncap in (1000, 8192):
                assert capi.attn_chunk_kernel_name(B, H, Hkv, Nq, ncap, D) == capi.attn_decode_kernel_name(B, H, Hkv, Nq, ncap, D)
                assert capi.attn_chunk_workspace_bytes(B, H, Hkv, Nq, ncap, D) == capi.attn_decode_workspace_bytes(B, H, Hkv, Nq, ncap, D)
            for ps, mp in ((16, 512), (256, 4)):
                assert capi.attn_chunk_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D) == capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, mp, D)
                assert capi.attn_chunk_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D) == capi.attn_decode_paged_kv8_kernel_name(B, H, Hkv, Nq, ps, mp, D)
                assert (capi.attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D)
                        == capi.attn_decode_paged_workspace_bytes(B, H, Hkv, Nq, ps, mp, D))
                assert (capi.attn_chunk_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D)
                        == capi.attn_decode_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, mp, D))


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_auto_split_rule_counts_the_row_blocks(knobs, cus):
    """S from (B x Hkv x RB, ceil(Ncap / 64), the CU count) alone; the workspace size is that of the named S"""
    capi.tune("rule_cus", cus)
    seen = set()
    for B, H, Hkv, Nq, ncap, D in ((1, 32, 8, 128, 4096, 128), (1, 32, 8, 512, 8192, 128), (4, 32, 8, 512, 4096, 128), (1, 32, 8, 2048, 2048, 128),
                                   (8, 64, 8, 16, 4096, 128), (2, 32, 32, 256, 4096, 64), (1, 2, 2, 65, 1024, 64), (1, 2, 1, 130, 1 << 16, 128),
                                   (3, 4, 2, 48, 1024, 64), (1, 8, 8, 65, 256, 64), (1, 1, 1, 65, 512, 128), (1, 1, 1, 65, 1 << 20, 64)):
        s = cl.auto_split(B, H, Hkv, Nq, ncap, cus)
        seen.add(s)
        want_bytes = s * B * H * Nq * (D + 1) * 4 if s > 1 else 0
        assert cl.name_flat(B, H, Hkv, Nq, ncap, D) == (capi.LC_OK, cl.want_name("", H, Hkv, Nq, D, s)), (B, H, Hkv, Nq, ncap, cus, s)
        assert capi.attn_chunk_workspace_bytes(B, H, Hkv, Nq, ncap, D) == want_bytes
        for ps in (16, 256):
            assert cl.name_paged(B, H, Hkv, Nq, ps, ncap // ps, D) == (capi.LC_OK, cl.want_name("_paged", H, Hkv, Nq, D, s))
            assert cl.name_kv8(B, H, Hkv, Nq, ps, ncap // ps, D) == (capi.LC_OK, cl.want_name("_paged_kv8", H, Hkv, Nq, D, s))
            assert capi.attn_chunk_paged_workspace_bytes(B, H, Hkv, Nq, ps, ncap // ps, D) == want_bytes
            assert capi.attn_chunk_paged_kv8_workspace_bytes(B, H, Hkv, Nq, ps, ncap // ps, D) == want_bytes
    assert len(seen) >= 4 and 1 in seen and max(seen) == min(64, -(-cus // 2))      # (the last shape: two groups, tiles to spare)
    # the row blocks are groups: at 256 CUs 8 K / V heads alone would get S = 32 of a 4096-key cache, with 8 row blocks each they get 4
    if cus == 256:
        assert cl.auto_split(1, 32, 8, 128, 4096, cus) == 4 and dl.auto_split(8, 4096, cus) == 16


def test_the_restated_plan_is_what_the_issue_states():
    assert [cl.rb_of(*s) for s in cl.SHAPES] == [2, 2, 2, 2, 5, 2]
    assert [cl.i_max(4, 2, 48, rb) for rb in range(2)] == [47, 47]                 # block 0 straddles; block 1 ends at token 47
    assert [cl.i_max(2, 1, 130, rb) for rb in range(5)] == [63, 127, 129, 125, 129]  # block 2 straddles
    assert [cl.i_max(2, 2, 128, rb) for rb in range(2)] == [63, 127]
    assert [cl.l_blk(1000, 2, 2, 128, rb, True, 1000) for rb in range(2)] == [936, 1000]
    assert [cl.l_blk(40, 2, 1, 130, rb, True, 1000) for rb in range(5)] == [0, 38, 40, 36, 40]    # a whole block without a visible key
    assert cl.l_blk(40, 2, 1, 130, 0, False, 1000) == 40


def test_new_symbols_are_exported(built):
    lib = C.CDLL(str(built["abi"]))
    for kind in KINDS:
        for sym in (KINDS[kind][0], f"lc_attn_chunk{kind}_workspace_bytes", f"lc_attn_chunk{kind}_kernel_name"):
            assert hasattr(lib, sym), sym
    assert lib.lc_abi_version() == 2


def test_capi_wrappers_run_the_decode_wrappers_shape_checks_without_a_gpu(built):
    q, k, v = dl.decode_inputs(2, 8, 2, 40, 128, 64, seed=1)
    o = torch.empty_like(q)
    lens = torch.tensor([100, 17], dtype=torch.int32)
    kp, vp, table = dl.paginate(k, v, (100, 17), 16, seed=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_chunk(q, k, v, o)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_chunk_paged(q, kp, vp, o, table, lens)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.attn_chunk_paged_kv8(q, kp.view(torch.uint8)[..., :64].contiguous(), vp.view(torch.uint8)[..., :64].contiguous(), o, table, lens)
    kp8, vp8 = (x.view(torch.uint8)[..., :64].contiguous() for x in (kp, vp))
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):        # (the fp8 wrapper checks shapes and dtypes before it asks for a GPU)
        capi.attn_chunk_paged_kv8(q, kp8, vp8, o, table[:1], lens)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        capi.attn_chunk_paged_kv8(q, kp8, vp8, o, table, lens, k_scale=torch.ones(3))
    with pytest.raises(TypeError, match="float8_e4m3fn or uint8"):
        capi.attn_chunk_paged_kv8(q, kp, vp, o, table, lens)


def test_audit_knows_the_chunk_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    rep = json.loads((built["abi"].parent / "obj" / build.AUDIT_OWN_REPORT["tu_attn_chunk"]).read_text())
    names = " ".join(r["kernel"] for r in rep)
    for d in (64, 128):
        for fam in ("attn_chunk_kernel", "attn_chunk_paged_kernel", "attn_chunk_paged_kv8_kernel"):
            assert f"{fam}ILi{d}E" in names, (fam, d)
    assert len(rep) == 6
    for r in rep:
        assert "attn_decode" not in r["kernel"]                             # isa_audit.json counts the decode kernels by that string
        assert r["scratch"] == 0 and not r["violations"], r
        assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]          # plain HIP: listed for rule R2 only
        assert r["asm_loads"] == 0
    main = json.loads((built["abi"].parent / "obj" / "isa_audit.json").read_text())
    assert not [r for r in main if "attn_chunk" in r["kernel"]]


# ------------------------------------------------------------------------------------------------------------------------------------
# a test of the GPU tests' inputs

@pytest.mark.parametrize("shape", cl.PIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", cl.DS)
def test_a_wrong_row_block_kernel_moves_every_row_it_touches(oracle, D, shape):
    """Causal.  A wrong limit that is too SHORT for a row loses the row's dominant key under `last`; one that is too LONG lets in the
    distinctive V row of `first_invisible`: each row a wrong kernel touches leaves the bound by >= TEETH x under the placement that pins its
    direction, and a row whose limit the wrong kernel happens to get right keeps its bits.  Block 0's Q rows: under `last`."""
    H, Hkv, Nq = shape
    B, G, R = len(cl.PIN_LENS), H // Hkv, cl.rows_of(*shape)
    lens = cl.PIN_LENS
    variants, right = cl.wrong_limits(shape, lens)
    rows = lambda f: np.array([[[f(b, (h % G) * Nq + i) for i in range(Nq)] for h in range(H)] for b in range(B)])      # noqa: E731
    right_nk = rows(right)
    assert (right_nk >= 1).all() and (right_nk < cl.NCAP).all()
    truths = {}
    for place in cl.PIN_PLACES:
        q, k, v = cl.pinned_inputs(D, shape, place)
        truths[place] = cl.truth_by_row(oracle, q, k, v, lens, True)
        assert (truths[place][1] == right_nk).all()
    for name, nk_row in variants.items():
        wrong_nk = rows(nk_row)
        touched_any = False
        for place, touched in (("last", wrong_nk < right_nk), ("first_invisible", wrong_nk > right_nk)):
            q, k, v = cl.pinned_inputs(D, shape, place)
            truth, nks = truths[place]
            wrong, _ = cl.truth_by_row(oracle, q, k, v, lens, True, nk_row=nk_row)
            ratio = _moved_by_row(truth, nks, wrong)
            if touched.any():
                touched_any = True
                assert ratio[touched].min() >= TEETH, (name, place, D, shape, float(ratio[touched].min()))
            assert ratio[wrong_nk == right_nk].max(initial=0.0) == 0.0, (name, place)
        assert touched_any, name
    # what each wrong kernel touches at these shapes, so that the proof above is not vacuous
    if shape == (4, 2, 48):
        assert (rows(variants["lim from the block-local row"]) != right_nk).reshape(B, Hkv, R)[:, :, 64:].all()       # block 1: every row
        assert (rows(variants["i_max from the last row of a straddling block"]) < right_nk).reshape(B, Hkv, R)[:, :, 16:48].all()
    assert (rows(variants["L_blk as every row's limit"]) > right_nk).any()
    # every block loads block 0's Q rows
    q, k, v = cl.pinned_inputs(D, shape, "last")
    truth, nks = truths["last"]
    wrong, _ = cl.truth_by_row(oracle, cl.block0_queries(q, Hkv), k, v, lens, True)
    ratio = _moved_by_row(truth, nks, wrong).reshape(B, Hkv, R)
    assert ratio[:, :, 64:].min() >= TEETH, (D, shape, float(ratio[:, :, 64:].min()))
    assert ratio[:, :, :64].max() == 0.0


def _moved_by_row(truth, nks, wrong):
    """[B, H, Nq]: largest |wrong - truth| / bound over a row's columns, the bound that of the row's visible keys (nks [B, H, Nq])"""
    from tests import tol
    atol = np.vectorize(lambda n: tol.attn_max_abs(int(n)))(nks)[..., None]
    bound = atol + tol.ATTN_RTOL_F16 * np.abs(truth.astype(np.float64))
    return (np.abs(wrong.astype(np.float64) - truth) / bound).max(axis=-1)


def test_the_pinned_inputs_are_what_the_docstring_says():
    for shape in cl.PIN_SHAPES:
        H, Hkv, Nq = shape
        G = H // Hkv
        for place in cl.PIN_PLACES:
            q, k, v = cl.pinned_inputs(64, shape, place)
            assert (k.abs() == 1).all() and torch.isfinite(v).all()
            for b, L in enumerate(cl.PIN_LENS):
                for h in range(0, H, max(1, H - 1)):
                    s = (q[b, h].double() @ k[b, h // G].double().T) / 8.0          # [Nq, Ncap]
                    for i in range(Nq):
                        lim = visible(L, Nq, cl.NCAP, True, i)
                        t = lim - 1 if place == "last" else lim
                        assert abs(s[i, t].item() - dl.SCORE) <= dl.SCORE * 2.0 ** -11 and s[i].argmax().item() == t
