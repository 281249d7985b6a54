"""CPU tests of the rotary-embedding + append boundary (lc_rope_append_paged_f16, lc_rope_append_paged_kv8 and their two name calls; no call here
reaches a device): the error codes and their order, the name grid, the exports, the Python wrappers' refusals, capi.rope_table against math.cos /
math.sin, the audit report of the eight kernels — then the proof that the bound of tests/rope_lib.py holds for the reference rounded once, and a
test of the GPU tests' inputs: on them each of twelve wrong kernels leaves the bound, and differs from the pinned reference — except the
two the quarter-turn table cannot show, because on it the table (table_fp16) and the rotated K (kv8_unrounded) are exact in fp16.

The reference, the bound, the wrong kernels and the inputs are shared with tests/test_gpu_rope.py: tests/rope_lib.py."""
import ctypes as C
import json
import math

import pytest
import torch

from leetcuda_amd import capi
from tests import append_lib as al
from tests import rope_lib as rl
from tests.decode_lib import K_SCALES, V_SCALES, scales

ENTRIES = ("f16", "kv8")
IL, PACKED = capi.ROPE_INTERLEAVED, capi.ROPE_PACKED_SRC
# B, H, Hkv, Nq, num_pages, page_size, max_pages, D, rot_dim, max_pos
OK = (2, 8, 2, 4, 70, 16, 64, 128, 64, 512)


def _run(lib, entry, ptrs, shape, stride=0, flags=0, sc=(None, None)):
    """ptrs: Q, Knew, Vnew, Qout, Kpool, Vpool, cos_sin, block_table, kv_len"""
    if entry == "kv8":
        return lib.lc_rope_append_paged_kv8(*ptrs, *sc, *shape, stride, flags, None)
    return lib.lc_rope_append_paged_f16(*ptrs, *shape, stride, flags, None)


def _name(entry, shape, stride=0, flags=0):
    """shape as OK (num_pages is dropped: the name calls take none)"""
    buf = C.create_string_buffer(128)
    fn = capi.load().lc_rope_append_paged_kv8_kernel_name if entry == "kv8" else capi.load().lc_rope_append_paged_kernel_name
    return fn(*shape[:4], *shape[5:], stride, flags, buf, 128), buf.value.decode()


def _with(**kw):
    names = ("B", "H", "Hkv", "Nq", "num_pages", "page_size", "max_pages", "D", "rot_dim", "max_pos")
    return tuple(kw.get(n, v) for n, v in zip(names, OK))


@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_and_their_order(built, entry):
    lib = capi.load()
    assert lib.lc_abi_version() == 2          # additive: the ABI version stays
    p = C.c_void_p(16)
    bad_shape = _with(Hkv=0, page_size=24, D=256)
    bad_dim = _with(D=96)
    for sc in ((p, p), (None, None)) if entry == "kv8" else ((None, None),):
        def f(ptrs, shape, stride=0, flags=0, sc=sc):
            return _run(lib, entry, ptrs, shape, stride, flags, sc)
        # 1. LC_ERR_ARG: a flag bit other than the two defined, before everything
        for bad in (4, 8, 5, 7 + 8, -1, 1 << 30):
            assert f([p] * 9, OK, 0, bad) == capi.LC_ERR_ARG, bad
            assert f([p] * 9, bad_shape, 0, bad) == capi.LC_ERR_ARG
            assert f([None] + [p] * 8, bad_dim, 0, bad) == capi.LC_ERR_ARG
            assert _name(entry, OK, 0, bad)[0] == capi.LC_ERR_ARG
            assert _name(entry, bad_shape, 0, bad)[0] == capi.LC_ERR_ARG
        for nul in range(9):                                     # ... then a null pointer, before shape and head dim
            ptrs = [p] * 9
            ptrs[nul] = None
            for shape in (OK, bad_shape, bad_dim, _with(rot_dim=24)):
                assert f(ptrs, shape) == capi.LC_ERR_ARG, (nul, shape)
                assert f(ptrs, shape, 8, 0) == capi.LC_ERR_ARG   # (a stride without the flag is a shape error: later)
        # 2. LC_ERR_SHAPE, every one of them before the head dim
        shapes = [_with(**{n: v}) for n in ("B", "H", "Hkv", "Nq", "num_pages", "max_pages", "D", "max_pos") for v in (0, -1)]
        shapes += [_with(H=3), _with(H=7, Hkv=2), _with(H=2, Hkv=4)]                                   # H % Hkv
        shapes += [_with(page_size=v) for v in (8, 24, 0, -16, 1, 48)]                                 # the append call's page ...
        shapes += [_with(page_size=1 << 16, max_pages=1 << 16, D=64, rot_dim=64),                      # ... and span bounds
                   _with(max_pages=1 << 21), _with(page_size=1 << 21, max_pages=16, D=64, rot_dim=64)]
        shapes += [_with(rot_dim=v) for v in (0, -16, 8, 24, 40, 100, 144, 256)]                       # not a multiple of 16, or not in [16, D]
        shapes += [_with(D=64, rot_dim=128), _with(D=64, rot_dim=80)]
        shapes += [_with(B=1 << 15, H=1 << 15, Hkv=1 << 15, Nq=64, D=64, rot_dim=64), _with(B=1 << 30, H=1, Hkv=1, Nq=17),      # the grid
                   _with(B=1 << 16, H=1 << 16, Hkv=1, Nq=1)]
        for shape in shapes:
            assert f([p] * 9, shape) == capi.LC_ERR_SHAPE, shape
            if shape[4] > 0:                                                                           # (the name call takes no num_pages)
                assert _name(entry, shape)[0] == capi.LC_ERR_SHAPE, shape
            if shape[7] == 128:                                                                        # shape before head dim
                d96 = shape[:7] + (96,) + shape[8:]
                assert f([p] * 9, d96) == capi.LC_ERR_SHAPE, d96
        # the grid bound counts the Q workgroups: a shape append takes (B x Hkv x blocks = 2^30) that B x (H + Hkv) x blocks pushes past an int
        big = _with(B=1 << 14, H=4, Hkv=2, Nq=1 << 19)
        assert capi.kv_append_paged_kernel_name(big[0], big[2], big[3], big[5], big[6], big[7]) == "kv_append_paged_kernel<128>"
        assert f([p] * 9, big) == capi.LC_ERR_SHAPE and _name(entry, big)[0] == capi.LC_ERR_SHAPE
        # src_row_stride: 0 without LC_ROPE_PACKED_SRC; with it a multiple of 8 and >= (H + 2 Hkv) D = 1536
        for stride, flags, want in ((8, 0, capi.LC_ERR_SHAPE), (1536, 0, capi.LC_ERR_SHAPE), (1536, IL, capi.LC_ERR_SHAPE), (-8, 0, capi.LC_ERR_SHAPE),
                                    (0, PACKED, capi.LC_ERR_SHAPE), (1528, PACKED, capi.LC_ERR_SHAPE), (1540, PACKED, capi.LC_ERR_SHAPE),
                                    (-1536, PACKED, capi.LC_ERR_SHAPE), (1537, PACKED | IL, capi.LC_ERR_SHAPE),
                                    (1536, PACKED, capi.LC_OK), (1544, PACKED | IL, capi.LC_OK), (1 << 40, PACKED, capi.LC_OK), (0, IL, capi.LC_OK)):
            assert _name(entry, OK, stride, flags)[0] == want, (stride, flags)
            if want != capi.LC_OK:
                assert f([p] * 9, OK, stride, flags) == want, (stride, flags)
                if not flags & PACKED or stride % 8 != 0 or stride <= 0:                               # (a bound that does not move with D)
                    assert f([p] * 9, bad_dim, stride, flags) == want, (stride, flags)
        for mis in range(6):                                     # the alignment of Q, Knew, Vnew, Qout and the pools
            ptrs = [p] * 9
            ptrs[mis] = C.c_void_p(8)
            assert f(ptrs, OK) == capi.LC_ERR_SHAPE, mis
            assert f(ptrs, bad_dim) == capi.LC_ERR_SHAPE
        for mis in (6, 7, 8):                                    # cos_sin, block_table and kv_len are 4-byte data: no 16-byte rule
            ptrs = [p] * 9
            ptrs[mis] = C.c_void_p(4)
            assert f(ptrs, bad_dim) == capi.LC_ERR_HEADDIM
        # 3. LC_ERR_HEADDIM
        for d in (32, 96, 256, 512, 16, 48, 80):
            shape = _with(D=d, rot_dim=16)
            assert f([p] * 9, shape) == capi.LC_ERR_HEADDIM, d
            assert _name(entry, shape)[0] == capi.LC_ERR_HEADDIM
    # Nq is unbounded, as in append
    for nq in (64, 65, 4096, 1 << 20):
        assert _name(entry, _with(Nq=nq))[0] == capi.LC_OK, nq


def test_names_for_every_head_dim_pairing_and_pool_kind(built):
    lib = capi.load()
    for entry, stem in (("f16", "rope_append_paged_kernel"), ("kv8", "rope_append_paged_kv8_kernel")):
        for D in (64, 128):
            for il in (False, True):
                want = f"{stem}<{D},{'true' if il else 'false'}>"
                for Bn, H, Hkv, Nq in ((3, 2, 2, 1), (3, 8, 2, 5), (64, 32, 8, 1), (8, 32, 8, 4096)):
                    for ps, mp in ((16, 64), (256, 4)):
                        for rot in rl.rot_dims(D):
                            for stride in (0, (H + 2 * Hkv) * D, (H + 2 * Hkv) * D + 64):
                                shape = (Bn, H, Hkv, Nq, 1, ps, mp, D, rot, 4096)
                                assert _name(entry, shape, stride, (IL if il else 0) | (PACKED if stride else 0)) == (capi.LC_OK, want)
                                assert capi.rope_append_paged_kernel_name(Bn, H, Hkv, Nq, ps, mp, D, rot, 4096, interleaved=il, kv8=entry == "kv8",
                                                                          src_row_stride=stride) == want
        fn = lib.lc_rope_append_paged_kv8_kernel_name if entry == "kv8" else lib.lc_rope_append_paged_kernel_name
        args = OK[:4] + OK[5:] + (0, 0)
        assert fn(*args, None, 128) == capi.LC_ERR_ARG
        for n in (4, 7, 0, -1):
            assert fn(*args, C.create_string_buffer(8), n) == capi.LC_ERR_ARG
        assert fn(*args, C.create_string_buffer(64), 64) == capi.LC_OK
    with pytest.raises(capi.LcError):
        capi.rope_append_paged_kernel_name(2, 8, 2, 4, 16, 64, 128, 24, 512)


def test_the_four_new_symbols_are_exported_and_the_old_ones_still_are(built):
    lib = capi.load()
    new = ("lc_rope_append_paged_f16", "lc_rope_append_paged_kv8", "lc_rope_append_paged_kernel_name", "lc_rope_append_paged_kv8_kernel_name")
    for name in new:
        assert name in capi.SYMBOLS and getattr(lib, name) is not None
    header = (capi.LIB_PATH.parent.parent.parent / "include" / "lc_abi.h").read_text()
    for name in capi.SYMBOLS:
        assert getattr(lib, name) is not None, name
        assert name + "(" in header, name
    assert len(capi.SYMBOLS) >= 67 and "#define LC_ROPE_INTERLEAVED 1" in header and "#define LC_ROPE_PACKED_SRC 2" in header
    assert lib.lc_abi_version() == 2


def test_capi_wrappers_check_shapes_dtypes_and_devices_without_a_gpu(built):
    Bn, H, Hkv, Nq, D, ps = 2, 4, 2, 4, 64, 16
    k_new, v_new = al.new_rows(Bn, Hkv, Nq, D, seed=1)
    q = torch.randn(Bn, H, Nq, D).half()
    table, P = al.make_table(Bn, 8, seed=2)
    lens = torch.tensor([100, 17], dtype=torch.int32)
    kp, vp = al.sentinel_pools(P, Hkv, ps, D, kv8=False)
    kp8, vp8 = al.sentinel_pools(P, Hkv, ps, D, kv8=True)
    ks, vs = scales(K_SCALES, Hkv), scales(V_SCALES, Hkv)
    cs = capi.rope_table(128, 32)
    want = (Bn, H, Hkv, Nq, P, ps, 8, D, 32, 128)
    assert capi._rope_append_args(q, k_new, v_new, kp, vp, cs, table, lens, None) == want
    assert capi._rope_append_args(q, k_new, v_new, kp, vp, cs, table, lens, q) == want
    assert capi._rope_append_args(q, k_new, v_new, kp8, vp8, cs, table, lens, torch.empty_like(q), ks, vs, kv8=True) == want
    with pytest.raises(RuntimeError, match="MI355X"):           # CPU tensors: no CPU path
        capi.rope_append_paged(q, k_new, v_new, kp, vp, cs, table, lens)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.rope_append_paged_kv8(q, k_new, v_new, kp8, vp8, cs, table, lens, k_scale=ks, v_scale=vs)
    for bad in ((q.float(), k_new, v_new, kp, vp, cs, table, lens, None), (q, k_new.float(), v_new, kp, vp, cs, table, lens, None),
                (q, k_new, v_new, kp, vp, cs.double(), table, lens, None), (q, k_new, v_new, kp, vp, cs.half(), table, lens, None),
                (q, k_new, v_new, kp, vp, cs, table, lens, q.float()), (q, k_new, v_new, kp8, vp8, cs, table, lens, None),
                (q, k_new, v_new, kp, vp, cs, table.long(), lens, None)):
        with pytest.raises(TypeError):
            capi._rope_append_args(*bad)
    for bad in ((q[:, :3].contiguous(), k_new, v_new, kp, vp, cs, table, lens, None), (q[:1], k_new, v_new, kp, vp, cs, table, lens, None),
                (q[:, :, :3].contiguous(), k_new, v_new, kp, vp, cs, table, lens, None), (q[..., :32].contiguous(), k_new, v_new, kp, vp, cs, table, lens, None),
                (q[0], k_new, v_new, kp, vp, cs, table, lens, None), (q, k_new, v_new, kp, vp, cs, table, lens, q[:, :2].contiguous()),
                (q, k_new, v_new, kp, vp, cs[:, :24].contiguous(), table, lens, None), (q, k_new, v_new, kp, vp, capi.rope_table(8, 128), table, lens, None),
                (q, k_new, v_new, kp, vp, cs[0], table, lens, None), (q, k_new, v_new[:, :, :3].contiguous(), kp, vp, cs, table, lens, None)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._rope_append_args(*bad)
    # the packed entry: [B,Nq,(H + 2 Hkv) D] or a row-strided view of it; the pool dtype picks the entry
    qkv = rl.pack_qkv(q, k_new, v_new)
    wide = rl.pack_qkv(q, k_new, v_new, pad=64)
    W = (H + 2 * Hkv) * D
    assert capi._rope_qkv_args(qkv, H, Hkv, kp, vp, cs, table, lens, None, None, None) == (want, W, False)
    assert capi._rope_qkv_args(wide[:, :, :W], H, Hkv, kp8, vp8, cs, table, lens, None, ks, vs) == (want, W + 64, True)
    with pytest.raises(RuntimeError, match="MI355X"):
        capi.rope_append_paged_qkv(qkv, H, Hkv, kp, vp, cs, table, lens)
    for bad in ((qkv.float(), H, Hkv, kp, vp, cs, table, lens, None, None, None), (qkv, H, Hkv, kp, vp, cs, table, lens, None, ks, vs),
                (qkv, H, Hkv, kp.float(), vp.float(), cs, table, lens, None, None, None)):
        with pytest.raises(TypeError):
            capi._rope_qkv_args(*bad)
    for bad in ((qkv, 3, Hkv, kp, vp, cs, table, lens, None, None, None), (qkv, H, 4, kp, vp, cs, table, lens, None, None, None),
                (qkv[:, :, :W - D], H, Hkv, kp, vp, cs, table, lens, None, None, None), (qkv[0], H, Hkv, kp, vp, cs, table, lens, None, None, None),
                (qkv.transpose(0, 1), H, Hkv, kp, vp, cs, table, lens, None, None, None),
                (rl.pack_qkv(q, k_new, v_new, pad=4)[:, :, :W], H, Hkv, kp, vp, cs, table, lens, None, None, None),
                (qkv, H, Hkv, kp, vp, cs, table, lens, torch.empty(Bn, H, Nq + 1, D).half(), None, None)):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            capi._rope_qkv_args(*bad)


def test_rope_table_against_math_cos_and_sin(built):
    for max_pos, rot_dim, base in ((64, 16, 10000.0), (4096, 128, 10000.0), (300, 64, 500000.0)):
        t = capi.rope_table(max_pos, rot_dim, base)
        assert t.dtype == torch.float32 and tuple(t.shape) == (max_pos, rot_dim) and t.is_contiguous()
        for pos in (0, 1, 7, max_pos // 2, max_pos - 1):
            for j in (0, 1, rot_dim // 4, rot_dim // 2 - 1):
                ang = pos * base ** (-2.0 * j / rot_dim)
                assert abs(float(t[pos, j]) - math.cos(ang)) <= 2.0 ** -23 + 1e-12 * max_pos, (pos, j)
                assert abs(float(t[pos, rot_dim // 2 + j]) - math.sin(ang)) <= 2.0 ** -23 + 1e-12 * max_pos, (pos, j)
    assert torch.equal(capi.rope_table(5, 16)[0], torch.tensor([1.0] * 8 + [0.0] * 8))


def test_audit_knows_the_eight_kernels_and_reports_no_scratch(built):
    from leetcuda_amd import build, isa_audit
    obj = built["abi"].parent / "obj"
    rep = json.loads((obj / build.AUDIT_OWN_REPORT["tu_rope_append"]).read_text())
    names = " ".join(r["kernel"] for r in rep)
    for d in (64, 128):
        for il in (0, 1):
            assert f"rope_append_paged_kernelILi{d}ELb{il}E" in names and f"rope_append_paged_kv8_kernelILi{d}ELb{il}E" in names, (d, il)
    assert len(rep) == 8
    for r in rep:
        assert r["scratch"] == 0 and not r["violations"], r
        assert isa_audit._owned(r["kernel"]) == set(), r["kernel"]          # plain HIP: listed for rule R2 only
        assert r["asm_loads"] == 0 and r["agpr"] == 0
    for other in ("isa_audit.json", build.AUDIT_OWN_REPORT["tu_kv_append"]):   # the other reports know nothing of the new unit
        assert "rope_append" not in (obj / other).read_text(), other


# ------------------------------------------------------------------------------------------------------------------------------------
# the bound's own proof, and a test of the GPU tests' inputs

def _case(D, ps, Nq, H, rot, il, pinned, fault=None, kv8=False, inputs=None, table=None, long_table=None):
    q, k_new, v_new, bt, P, lens = (inputs or rl.grid_inputs(D, ps, Nq, H))[:6]
    if table is None:
        table = rl.pinned_table(rot) if pinned else rl.random_table(rot)
    ks, vs = al.kind_scales("kv8") if kv8 else (None, None)
    return rl.rope_model(q, k_new, v_new, bt, P, lens, ps, table, il, kv8, ks, vs, fault, long_table)


def _judge(D, ps, Nq, H, rot, il, got, inputs=None, table=None):
    """(Q violations, K-pool violations on the written rows) of a model's fp16 outputs under the bound, on the random table"""
    q, k_new, v_new, bt, P, lens = (inputs or rl.grid_inputs(D, ps, Nq, H))[:6]
    table = rl.random_table(rot) if table is None else table
    qe, qb = rl.q_truth(q, lens, al.NCAP, table, il)
    pe, pb, written = rl.pool_truth(k_new, bt, P, lens, ps, table, il)
    return rl.violations(got[0], qe, qb), rl.violations(got[1][written], pe[written], pb[written])


def test_the_reference_rounded_once_holds_the_bound_and_the_pinned_table_is_exact():
    for D in rl.DS:
        for il in (False, True):
            for rot in rl.rot_dims(D):
                for Nq, H in ((100, 8), (5, 2)):
                    vq, vk = _judge(D, 64, Nq, H, rot, il, _case(D, 64, Nq, H, rot, il, False))
                    assert not vq.any() and not vk.any(), (D, il, rot, Nq)
                    # the quarter-turn table: exact = a signed permutation of the inputs, in fp16 already
                    q, k_new = rl.grid_inputs(D, 64, Nq, H)[:2]
                    pos = rl.positions(al.LENS, Nq)
                    exact, e = rl.rope_ref(k_new, pos, rl.pinned_table(rot), il)
                    assert torch.equal(exact.half().double(), exact)
                    assert torch.equal(exact.abs().sort(dim=-1).values, k_new.double().abs().sort(dim=-1).values)
    t = rl.pinned_table(16)
    assert not torch.equal(t[5], t[6]) and not torch.equal(t[5], t[9]) and float(t[5, 0]) != float(t[5, 1])      # neighbours, t and t + 4, two pairs
    assert all(not torch.equal(t[i], t[i + 1]) and not torch.equal(t[i], t[i + 4]) for i in range(60))
    assert set(t.flatten().tolist()) == {1.0, 0.0, -1.0}


GRID_FAULTS = ("pairing_swapped", "reverse", "pos_len_plus_i", "pos_i", "cos_sin_swapped", "table_fp16")


@pytest.mark.parametrize("D", rl.DS)
def test_each_wrong_kernel_leaves_the_bound_on_the_grid_and_differs_on_the_pinned_table(D):
    """the base-10000 table: on EVERY case of the grid a wrong kernel leaves the bound on more than 5 % of the elements it touches.  The
    quarter-turn table: its outputs differ from the reference's on the grid (not on every case: at Nq = 1 the three positions 776, 128 and 64
    are multiples of four, where every pair turns alike and the two pairings cannot be told apart)"""
    ps, H = 64, 8
    for il in (False, True):
        for rot in rl.rot_dims(D):
            shown = {}
            for Nq in rl.GRID_NQ:
                ref_pinned = _case(D, ps, Nq, H, rot, il, True)
                for fault in GRID_FAULTS:
                    vq, vk = _judge(D, ps, Nq, H, rot, il, _case(D, ps, Nq, H, rot, il, False, fault))
                    fq, fk = float(vq[..., :rot].float().mean()), float(vk.view(-1, D)[:, :rot].float().mean())      # of the rotated elements
                    assert fq > 0.05 and fk > 0.05, (fault, D, il, rot, Nq, fq, fk)
                    got = _case(D, ps, Nq, H, rot, il, True, fault)
                    shown[fault] = shown.get(fault, 0) + (not torch.equal(got[0], ref_pinned[0]) and not torch.equal(got[1], ref_pinned[1]))
                # Q position from the row index g Nq + i: heads with g > 0 only
                got = _case(D, ps, Nq, H, rot, il, False, "q_pos_row")
                vq, vk = _judge(D, ps, Nq, H, rot, il, got)
                assert not vk.any() and not vq[:, 0::4].any() and vq[:, 1::4].float().mean() > 0.05, ("q_pos_row", D, il, rot, Nq)
                shown["q_pos_row"] = shown.get("q_pos_row", 0) + (not torch.equal(_case(D, ps, Nq, H, rot, il, True, "q_pos_row")[0], ref_pinned[0]))
                if rot < D:                                                      # the partial-rotary tail rotated
                    vq, vk = _judge(D, ps, Nq, H, rot, il, _case(D, ps, Nq, H, rot, il, False, "tail_rotated"))
                    assert not vq[..., :rot].any() and vq[..., rot:].float().mean() > 0.05 and vk.any(), ("tail_rotated", D, il, rot, Nq)
                    shown["tail_rotated"] = shown.get("tail_rotated", 0) + (not torch.equal(_case(D, ps, Nq, H, rot, il, True, "tail_rotated")[0], ref_pinned[0]))
            assert shown.pop("table_fp16") == 0                                  # the quarter-turn table is exact in fp16: it cannot show this one
            assert all(n >= 2 for n in shown.values()), (D, il, rot, shown)


@pytest.mark.parametrize("D", rl.DS)
def test_the_fp8_faults_change_the_codes(D):
    """codes from the unrounded fp32 K (a double rounding: rare, so counted over the whole grid of Nq = 100 cases), and K unrotated"""
    moved = 0
    for il in (False, True):
        for rot in rl.rot_dims(D):
            for ps in rl.PAGE_SIZES:
                ref = _case(D, ps, 100, 8, rot, il, False, None, kv8=True)
                moved += int((_case(D, ps, 100, 8, rot, il, False, "kv8_unrounded", kv8=True)[1] != ref[1]).sum())
                un = _case(D, ps, 100, 8, rot, il, False, "kv8_k_unrotated", kv8=True)
                assert int((un[1] != ref[1]).sum()) > 1000 and torch.equal(un[2], ref[2]), (D, il, rot, ps)
                pin = _case(D, ps, 100, 8, rot, il, True, None, kv8=True)
                assert not torch.equal(_case(D, ps, 100, 8, rot, il, True, "kv8_k_unrotated", kv8=True)[1], pin[1])
                # the quarter-turn table cannot show the unrounded codes: its rotated K is exact in fp16, so both roundings give one code
                assert torch.equal(_case(D, ps, 100, 8, rot, il, True, "kv8_unrounded", kv8=True)[1], pin[1])
    print(f"[rope] D = {D}: {moved} fp8 codes of the Nq = 100 grid differ between rounding the rotated K to fp16 first and not")
    assert moved >= 1


@pytest.mark.parametrize("ps", rl.PAGE_SIZES)
def test_a_page_dropped_for_q_and_an_unclamped_table_row_show(ps):
    D, rot = 64, 32
    inputs = rl.table_inputs(D, ps)
    assert all(inputs[6])                                                        # every batch entry loses tokens
    for il in (False, True):
        ref = _case(D, ps, 100, 8, rot, il, False, None, inputs=inputs)
        got = _case(D, ps, 100, 8, rot, il, False, "q_page_dropped", inputs=inputs)
        vq, vk = _judge(D, ps, 100, 8, rot, il, got, inputs=inputs)
        lost = sum(len(d) for d in inputs[6])
        assert int(vq.any(dim=-1).any(dim=1).sum()) == lost and not vk.any() and not _judge(D, ps, 100, 8, rot, il, ref, inputs=inputs)[0].any()
        # ... and on the quarter-turn table (the unwritten rows holding the sentinel a GPU test prefills Qout with)
        sent = float(torch.tensor([al.SENT16], dtype=torch.int16).view(torch.half))
        pin = [rl.rope_model(*inputs[:6], ps, rl.pinned_table(rot), il, fault=f, unwritten=sent) for f in (None, "q_page_dropped")]
        assert int((pin[1][0] != pin[0][0]).any(dim=-1).any(dim=1).sum()) == lost and torch.equal(al.bits(pin[1][1]), al.bits(pin[0][1]))
        # a table of SHORT_MAX_POS rows: the positions behind it read its last row; an unclamped kernel reads what a longer table holds
        short = rl.random_table(rot)[:rl.SHORT_MAX_POS].contiguous()
        grid = rl.grid_inputs(D, ps, 100, 8)
        got = _case(D, ps, 100, 8, rot, il, False, "unclamped_row", table=short, long_table=rl.random_table(rot))
        vq, vk = _judge(D, ps, 100, 8, rot, il, got, table=short)
        pos = rl.positions(al.LENS, 100)
        behind = (pos >= rl.SHORT_MAX_POS)[:, None, :, None].expand_as(vq)
        assert not vq[~behind].any() and vq[behind].float().mean() > 0.05 and vk.float().mean() > 0.05
        assert not _judge(D, ps, 100, 8, rot, il, _case(D, ps, 100, 8, rot, il, False, None, table=short), table=short)[0].any()
        assert grid[5] == al.LENS
        # ... and on the quarter-turn table: its first SHORT_MAX_POS rows against the rows that lie behind them
        pshort = rl.pinned_table(rot)[:rl.SHORT_MAX_POS].contiguous()
        pref = _case(D, ps, 100, 8, rot, il, False, None, table=pshort)
        pgot = _case(D, ps, 100, 8, rot, il, False, "unclamped_row", table=pshort, long_table=rl.pinned_table(rot))
        assert not torch.equal(pgot[0], pref[0]) and not torch.equal(al.bits(pgot[1]), al.bits(pref[1]))
        assert torch.equal(pgot[0][~behind], pref[0][~behind])
