"""Decode attention on the GPU on inputs whose answer is exact (`uniform`), pinned to one key (`pinned`) or moved by a score step (`step`):
every (D, RT) instantiation of attn_decode_kernel, attn_decode_combine_kernel under split counts from 1 up to more ranges than tiles, and
attn_decode_paged_kernel — on EVERY element of a NaN-prefilled O that sits in the middle of a NaN-filled buffer (a guard of 64 D halves on
each side must stay NaN; rows without a visible key must be exactly 0; everything else finite and inside the class's bound).  Inputs, truths,
bounds and the fault locator live in tests/decode_lib.py, the CPU proof that the inputs have teeth in tests/test_abi_cpu_decode_exact.py; its docstring describes
the classes, what each cannot see, and the assumption behind `uniform`'s S > 1 bound (device log2f / exp2 within 8 fp32 ulps).

Every case asserts the kernel name first (attn_decode_kernel<D,RT> with the ` xS` suffix), forces the split through "attn_decode_split"
inside try / finally, and runs one launch with one batch entry per length.  `uniform` at S = 1 asserts torch.equal with E rounded once on
every row whose nk is a power of two; the paged cases assert torch.equal with the contiguous call on the gathered cache.

Measured on an MI355X (recorded values, not thresholds): worst |err| / bound per (RT, class, S) over D, mask and row shapes —
  class           RT   S = 1      2      3      4      8     16     64
  uniform          1   0.499  0.501  0.499      -  0.499  0.499  0.499      (S = 1: |err| / ulp16(E); S > 1: |err| / ulp16(max(|E|, 2^-6)))
  uniform          2   0.499  0.501  0.499      -  0.499  0.499  0.499
  uniform          4   0.499  0.500  0.501      -  0.499  0.499  0.499
  pinned           1   0.316      -  0.316      -  0.314      -      -      (worst over the six places)
  pinned           2   0.367      -  0.367      -  0.367      -      -
  pinned           4   0.524      -  0.524      -  0.524      -      -
  step             1   0.097  0.095      -  0.095  0.095      -      -
  step             2   0.097  0.097      -  0.097  0.097      -      -
  step             4   0.097  0.097      -  0.096  0.096      -      -
  paged uniform  1, 4  0.499      -      -  0.499      -      -      -
  paged step     1, 4  0.097      -      -  0.096      -      -      -
No launch missed bit-equality where it is asked (S = 1, nk a power of two), and every paged launch has the bits of the contiguous call.  Recorded,
not asserted: at L = 1024, non-causal, where every range holds a power of two of keys, all 48 split launches (S = 2, 8, 16; paged S = 4) are
bit-equal to E rounded once too — the device's log2f and exp2 are exact there.  `uniform`'s worst S > 1 case, 0.501 of its bound, is the
output's own half ulp: the combine's error stays far inside the assumed 2^-17.  No kernel needed a fix.
Wall time of the file on an MI355X: 7.2 s for the 746 tests (the slowest 0.34 s, the first launch); the 165 CPU tests of
tests/test_abi_cpu_decode_exact.py take 40 s."""
import functools

import numpy as np
import pytest
import torch

from tests import tol
from tests.decode_lib import EXACT_PIN_LENS as PIN_LENS
from tests.decode_lib import EXACT_PLACES as PLACES
from tests.decode_lib import NCAP_POW2 as NCAP
from tests.decode_lib import (GRID, LENS, PAGE_SIZES, PAGED_SHAPES, PINNED_SPLITS, ROW_SHAPES, STEP_LENS, STEP_SPLITS, UNIFORM_SPLITS, _capi, check_decode,
                              decode_bound, gather, judge, paginate, pinned_split_key, pinned_truth, rt_of, step_bound, step_inputs, step_truth,
                              uniform_bound, uniform_hint, uniform_inputs, uniform_truth)
from tests.decode_lib import exact_pinned_inputs as pinned_inputs
from tests.test_gpu_attn_exact import round_once

pytestmark = pytest.mark.gpu

MASKS = (False, True)


def _id(x):
    return "x".join(map(str, x)) if isinstance(x, tuple) else ("causal" if x is True else "full" if x is False else str(x))


@functools.lru_cache(maxsize=3)
def _on_gpu(kind, *key):
    """the CPU inputs of a class, moved over once per (class, shape)"""
    src = {"uniform": uniform_inputs, "pinned": pinned_inputs, "step": step_inputs}[kind](*key)
    return tuple(x.cuda() for x in src[:3])


def _launch(capi, q, k, v, lens, causal, S, D, paged=None):
    """(kernel name, O [B,H,Nq,D] on the GPU): asserts the name, runs one call under the forced split into a view in the middle of a NaN-filled
    buffer and asserts that the guard on both sides is still NaN.  paged = (table, page size): K / V are pools."""
    B, H, Nq, _ = q.shape
    Hkv = k.shape[1]
    n, guard = q.numel(), 64 * D
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.half, device="cuda")
    o = buf[guard:guard + n].view(q.shape)
    dl = torch.tensor(list(lens), dtype=torch.int32, device="cuda")
    capi.tune("attn_decode_split", S)
    try:
        if paged is None:
            name = capi.attn_decode_kernel_name(B, H, Hkv, Nq, NCAP, D, causal=causal)
            want = f"attn_decode_kernel<{D},{rt_of(H, Hkv, Nq)}>"
        else:
            table, ps = paged
            name = capi.attn_decode_paged_kernel_name(B, H, Hkv, Nq, ps, NCAP // ps, D, causal=causal)
            want = f"attn_decode_paged_kernel<{D},{rt_of(H, Hkv, Nq)}>"
        assert name == want + (f" x{S}" if S > 1 else ""), name
        if paged is None:
            capi.attn_decode(q, k, v, o, dl, causal=causal)
        else:
            capi.attn_decode_paged(q, k, v, o, table, dl, causal=causal)
    finally:
        capi.tune("attn_decode_split", 0)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all(), (name, "wrote outside O")
    return name, o


def _note(name, cls, shape, S, worst, extra=""):
    H, Hkv, Nq = shape
    print(f"[decode_exact] kernel={name} | class={cls} | RT={rt_of(H, Hkv, Nq)} | S={S} | worst_ratio={worst:.4f}{extra}")


def _judge_uniform(name, o, D, shape, causal, S):
    H, Hkv, Nq = shape
    E, nks, P = uniform_truth(D, H, Hkv, Nq, causal)
    out = o.double().cpu().numpy()
    worst = judge(name, "uniform", out, E, uniform_bound(E, S), nks, Hkv, strict=(S == 1), hint=uniform_hint(out, P, LENS, H, Hkv, Nq, causal, S))
    pow2 = (nks > 0) & (nks & (nks - 1) == 0)                                  # [B, Nq]
    rows = torch.from_numpy(np.broadcast_to(pow2[:, None, :], (len(LENS), H, Nq)).copy())
    want = torch.from_numpy(round_once(E, False)).half()
    extra = ""
    if S == 1:
        assert rows.any()
        assert torch.equal(o.cpu()[rows], want[rows]), (name, "nk a power of two: not E rounded once")
    elif not causal and S in (2, 4, 8, 16):                                    # L = 1024: every range holds a power of two of keys.  Recorded only.
        extra = f" | bit_equal_L1024={float((o.cpu()[0] == want[0]).float().mean()):.6f}"
    _note(name, "uniform", shape, S, worst, extra)


def _judge_step(name, o, D, shape, causal, S):
    H, Hkv, Nq = shape
    truth, nks = step_truth(D, H, Hkv, Nq, causal)
    out = o.double().cpu().numpy()
    _, _, _, tiles = step_inputs(D, H, Hkv, Nq)
    G = H // Hkv
    worst = judge(name, "step", out, truth, step_bound(truth, nks), nks, Hkv,
                  hint=lambda b, h, i: f"the max rises in key tile {tiles[b][h // G]} of {-(-STEP_LENS[b] // 64)}")
    for b in range(len(STEP_LENS)):                                             # (tol.attn_close itself, row by row)
        for i in range(Nq):
            ok, err, excess = tol.attn_close(out[b, :, i], truth[b, :, i], N=int(nks[b, i]), rtol=tol.ATTN_RTOL_SPIKE)
            assert ok, (name, b, i, err, excess)
    _note(name, "step", shape, S, worst)


# ------------------------------------------------------------------------------------------------------------------------------------
_UNIFORM = [(D, shape, causal, S) for D in (64, 128) for shape in GRID for causal in MASKS for S in UNIFORM_SPLITS]


@pytest.mark.parametrize("D,shape,causal,S", _UNIFORM, ids=lambda x: _id(x))
def test_uniform(D, shape, causal, S):
    """S = 16 and 64 exceed the tile count of most entries: ranges are empty"""
    capi = _capi()
    q, k, v = _on_gpu("uniform", D, *shape)
    name, o = _launch(capi, q, k, v, LENS, causal, S, D)
    _judge_uniform(name, o, D, shape, causal, S)


_PINNED = [(D, shape, place, causal, S) for D in (64, 128) for shape in ROW_SHAPES for place in PLACES for causal in MASKS for S in PINNED_SPLITS]


@pytest.mark.parametrize("D,shape,place,causal,S", _PINNED, ids=lambda x: _id(x))
def test_pinned(D, shape, place, causal, S):
    """one key per row outweighs the rest; step_seam pins the keys 64 t + 31 / 64 t + 32 between the two pipeline steps of <128,4>"""
    capi = _capi()
    H, Hkv, Nq = shape
    key = (D, place, causal, H, Hkv, Nq, pinned_split_key(place, S))
    q, k, v = _on_gpu("pinned", *key)
    name, o = _launch(capi, q, k, v, PIN_LENS, causal, S, D)
    truth, nks = pinned_truth(*key)
    out = o.double().cpu().numpy()
    targets = pinned_inputs(*key)[3]
    worst = judge(name, f"pinned {place}", out, truth, decode_bound(truth, nks), nks, Hkv, hint=lambda b, h, i: f"target key {targets[b][h][i]}")
    assert check_decode(out, truth.astype(np.float32), nks, name) <= 1.0
    _note(name, "pinned", shape, S, worst, f" | place={place}")


_STEP = [(D, shape, causal, S) for D in (64, 128) for shape in ROW_SHAPES for causal in MASKS for S in STEP_SPLITS]


@pytest.mark.parametrize("D,shape,causal,S", _STEP, ids=lambda x: _id(x))
def test_step(D, shape, causal, S):
    """the running max rises in mid-walk on one wave of one range: alpha, the merge's `mine` and the combine's weights all differ from 1"""
    capi = _capi()
    q, k, v = _on_gpu("step", D, *shape)
    name, o = _launch(capi, q, k, v, STEP_LENS, causal, S, D)
    _judge_step(name, o, D, shape, causal, S)


_PAGED = [(cls, D, shape, ps, causal, S) for cls in ("uniform", "step") for D in (64, 128) for shape in PAGED_SHAPES for ps in PAGE_SIZES
          for causal in MASKS for S in (1, 4)]


@functools.lru_cache(maxsize=2)
def _pools(cls, D, shape, ps):
    """(pools, table, gathered K / V) on the GPU: pages scattered over the pool, NaN at every position >= L_b and in the spare pages"""
    src, lens = (uniform_inputs, LENS) if cls == "uniform" else (step_inputs, STEP_LENS)
    _, k, v = src(D, *shape)[:3]
    kp, vp, table = paginate(k, v, lens, ps, seed=ps + D)
    return tuple(x.cuda() for x in (kp, vp, table, gather(kp, table), gather(vp, table)))


@pytest.mark.parametrize("cls,D,shape,ps,causal,S", _PAGED, ids=lambda x: _id(x))
def test_paged(cls, D, shape, ps, causal, S):
    """the same inputs through a block table: inside the class bound, and the bits of the contiguous call on the gathered cache"""
    capi = _capi()
    lens = LENS if cls == "uniform" else STEP_LENS
    q = _on_gpu(cls, D, *shape)[0]
    kp, vp, table, kflat, vflat = _pools(cls, D, shape, ps)
    name, o = _launch(capi, q, kp, vp, lens, causal, S, D, paged=(table, ps))
    (_judge_uniform if cls == "uniform" else _judge_step)(name, o, D, shape, causal, S)
    flat_name, flat = _launch(capi, q, kflat, vflat, lens, causal, S, D)
    assert name.replace("_paged", "") == flat_name
    assert torch.equal(o, flat), name


@pytest.mark.parametrize("D", [64, 128])
def test_uniform_with_a_nan_tail(D):
    """NaN in K and V at every position >= L_b: the bits of the launch with a zero tail (and inside `uniform`'s bound)"""
    capi = _capi()
    shape = (8, 2, 9)
    q, k, v = _on_gpu("uniform", D, *shape)
    tail = torch.arange(NCAP, device="cuda").view(1, 1, NCAP, 1) >= torch.tensor(LENS, device="cuda").view(-1, 1, 1, 1)
    for causal in MASKS:
        for S in (1, 3):
            name, ref = _launch(capi, q, k.masked_fill(tail, 0.0), v.masked_fill(tail, 0.0), LENS, causal, S, D)
            _, got = _launch(capi, q, k.masked_fill(tail, float("nan")), v.masked_fill(tail, float("nan")), LENS, causal, S, D)
            assert torch.equal(got, ref), (name, causal)
            _judge_uniform(name, got, D, shape, causal, S)
