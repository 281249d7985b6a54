"""The non-causal attention forward on inputs whose answer is exact or pinned to one key: every kernel behind lc_attn_fwd_f16 / _bf16 —
lock-step (8, 4, 2 waves), merged-phase in its three block walks and its ragged-N form, split-KV + combine, the generated kernel in both
schedules, attn_bigd2 / 3 / 4 / 6 / 7, the column-split kernel, bf16 and V-transposed forms, the XCD block maps and the D = 1024 KV-walk
stagger — on EVERY element of every head of a NaN-prefilled O.  The randn tests of tests/test_gpu_attn.py hold these kernels to 2e-3 ... 8e-3
absolute where |O| ~ 1 / sqrt(N) = 0.03 ... 0.06: several per cent of the signal.  Three input classes, each blind where another sees:

  uniform   Q = 0 (even heads, K random +-1) or K = 0 (odd heads, Q random +-1): every score is exactly 0, every key has weight exactly 1 and
            O is the plain mean of V over the keys, the same for every row.  V is drawn from {0.5, 1, 1.5, -1, 2, -0.5, 0.75, -2} (exact in
            fp16 and bf16; a sum over N <= 4096 keys is a multiple of 1/4 below 2^13: exact in fp32 in ANY order), so l = N and every partial
            sum are exact and the only rounding left is the output's.  Truth E = the fp64 mean.  With ulp(E) the spacing of the output type
            at |E|:  unsplit kernels  |out - E| < ulp(E) (out is one of E's two neighbours), and for N a power of two (1 / N exact too) out is
            BIT-EQUAL to E rounded once;  split-KV with S ranges (fp16 partials)  |out - E| <= 2^-11 mean_s |E_s| + ulp(E), E_s the mean
            over range s.  A key counted 0 or 2 times moves a column by |v - E| / (N -+ 1).  Cannot see: which key carries which weight (all
            weights are equal), a wrong rescale (the running max never moves).
            The draw is weighted so that the eight values have mean 0 (2 2 2 3 1 1 2 3 sixteenths in the order above): with equal weights
            E ~ 0.28 for every column, a bf16 ulp there is 2^-9, and one tile of N = 1152 keys moves the mean by less than 20 of them.
  pinned    test_gpu_causal_mask.build_inputs' construction without the mask: K random +-1, Q_i = (12 / sqrt(D)) K[pi(i)], V randn: key pi(i)
            scores 12 for row i, every other key about N(0, 144 / D) (<= 16).  Maps pi:  anywhere  uniform in [0, N), seeded per head;
            reverse  N - 1 - i (the first query block's keys sit in the last tile of the walk, the last split range, the ring's epilogue);
            edges  row i -> tile (i // 2) mod (N / 64), its key 0 for even i and key 63 for odd i (every tile's first and last key: both sides
            of every split-range seam).  Truth: the oracle on the rounded inputs.  Bound: fp16 8e-3 + tol.ATTN_RTOL_SPIKE |truth| (the causal
            file's); bf16 1.6e-2 + 2^-5 |truth| (the bf16 figure of test_full_width_large_head_dim_kernel on spiked inputs; 8 x the fp16 rtol
            for three mantissa bits fewer).  Cannot see: a tile walked TWICE — the dominant weight renormalises to 1, so a doubled tile
            (the target's or its neighbour) moves a row only by the share of the other keys: measured on the CPU at the shapes below,
            the WORST row of a case moves by 0.02 ... 0.9 x the bound at D >= 256 and D = 96, up to 2 x at D = 128 and 4 x at D = 64 (27 x
            at D = 32, in the few rows where a second key scores near 12), and the typical row by nothing — nor a skipped tile that is
            not the target's.  `uniform` exists for that reason.
  step      K[j] = u (random +-1 per head) for the 40 keys j in [N/2 + 24, N/2 + 64) and 0 elsewhere, Q_i = (c_i / sqrt(D)) u with
            c_i = (2, 3, 4)[i % 3]: those keys score c_i, the rest 0, so EVERY row raises its running max in the middle of the walk.  V from
            the set above (equal weights), except that the 40 step keys share one row w of it per head: with 40 independent draws |O| is
            about the mean of 40 values, 0.2, and a wrong l, which scales the row, cannot move it by 20 x the bf16 bound of >= 1.6e-2
            sqrt(256 / N); with w the rows reach |O| ~ 2 x the step keys' share of the weight.  Truth: the oracle.
            Bound: tol.attn_close(N, rtol=tol.ATTN_RTOL_SPIKE); bf16: tol.attn_close(N, bf16=True, rtol=2^-6), the form
            test_d256_n_multiple_of_128_runs_the_ring_kernel uses.  Cannot see: a dropped or doubled plain tile (no key of it weighs more than 1 / N of the row).

CPU tests (no gpu mark) prove at the shapes the GPU tests run, in fp64 torch, that the inputs have teeth — factor TEETH = 20 over the bound
that applies to the shape: `pinned` — zeroing the weights of the 64-key tile that holds pi(i) moves every row of every map; `uniform` — for
every 64-key tile t the mean without tile t and the mean with tile t twice both leave E in at least one column of every head; `step` — an
fp64 online softmax over 64-key tiles with the rescale factor left out of l, or out of O, moves every row.  The one shape with a single
KV tile (D = 1024, N = 64) has no tile to lose without losing the row and no rescale: it runs all classes on the GPU and only `pinned`'s
teeth on the CPU.

No unsplit path misses bit-equality where it is asked (63 launches with N a power of two, every element equal); at the other N the worst
element is at most half an ulp(E) off, a correctly rounded quotient.  Split-KV, held to its own bound (fp16 partials), is exact on these
inputs too.

Measured worst |err| / bound per (path, input class) over every case of the path (MI355X; recorded, not thresholds; `uniform`: |err| / ulp(E)
for the unsplit paths, 0 = bit-equal everywhere it is asked):
  path                      uniform   pinned-anywhere   pinned-reverse   pinned-edges   step
  lock-step                   0.400             0.093            0.078          0.080  0.153
  generated                   0.333             0.108            0.102          0.110  0.184
  split-KV                    0.000             0.160            0.156          0.150  0.287
  merged-phase walks          0.000             0.118            0.102          0.099  0.198
  merged-phase ragged         0.474             0.116            0.103          0.103  0.222
  column-split                0.333             0.076            0.078          0.061  0.138
  attn_bigd2                  0.500             0.118            0.109          0.122  0.260
  attn_bigd7                  0.500             0.106            0.109          0.106  0.235
  attn_bigd3                  0.000             0.112            0.080          0.109  0.164
  attn_bigd6                  0.500             0.081            0.082          0.067  0.269
  attn_bigd4                  0.000             0.082            0.082          0.077  0.163
  merged-phase block seam     0.000                 -                -              -      -
Wall time of the file on an MI355X: 10 s for the 484 GPU tests (the slowest, 130 heads through four walks, 0.6 s); the 219 CPU tests take a minute.
"""
import contextlib
import functools
from typing import NamedTuple

import numpy as np
import pytest
import torch

from tests import tol
from tests.test_gpu_causal import _capi, report_worst_row
from tests.test_gpu_causal_mask import SCORE, TEETH

BH = 3            # B x H: a head-index slip cannot cancel between two heads
V8 = (0.5, 1.0, 1.5, -1.0, 2.0, -0.5, 0.75, -2.0)
V16 = (0.5, 0.5, 1.0, 1.0, 1.5, 1.5, -1.0, -1.0, -1.0, 2.0, -0.5, 0.75, 0.75, -2.0, -2.0, -2.0)      # the same values, mean 0
MAPS = ("anywhere", "reverse", "edges")
INPUTS = ("uniform", "pinned-anywhere", "pinned-reverse", "pinned-edges", "step")
STEP_C = (2.0, 3.0, 4.0)


class Case(NamedTuple):
    path: str            # the row of the table above
    D: int
    N: int
    want: str            # the kernel name the case means to run
    knobs: tuple = ()    # ((key, value), ...)
    vt: bool = False
    bf: bool = False
    bh: int = BH
    split: int = 1       # KV ranges
    merged: bool = False      # a merged-phase kernel: counts its overflow slow path

    @property
    def id(self):
        k = "-".join(f"{a}={b}" for a, b in self.knobs) or "auto"
        return f"{self.path}-D{self.D}-N{self.N}-{'bf16' if self.bf else 'fp16'}-{'v_dn' if self.vt else 'v_nd'}-bh{self.bh}-{k}"


def _tf(b):
    return "true" if b else "false"


def _cases():
    cs = []
    for D in (32, 64, 96, 128):
        for N, nw, knob in ((320, 2, 0), (384, 4, 0), (512, 8, 8)):      # (auto hands N = 512 on this grid to the 4-wave form or the generated kernel)
            for vt in (False, True):
                cs.append(Case("lock-step", D, N, f"attn_fwd_kernel<{D},{nw},{_tf(vt)},0>", (("attn_nw", knob),) if knob else (), vt))
    for D in (64, 128):
        for vt in (False, True):
            for nw in (513, 515, 517):
                cs.append(Case("merged-phase walks", D, 1024, f"attn_fwd_w4u_kernel<{D},{_tf(vt)},{(nw - 513) // 2}>", (("attn_nw", nw),), vt, merged=True))
            for N in (1152, 1216):
                cs.append(Case("merged-phase ragged", D, N, f"attn_fwd_w4u_kernel<{D},{_tf(vt)},0>", (), vt, merged=True))
        for N, S, vt in [(256, 2, False)] + [(2048, S, False) for S in (2, 4, 8, 16)] + [(2048, 4, True)]:
            cs.append(Case("split-KV", D, N, f"attn_fwd_w4u_kernel<{D},{_tf(vt)},3>", (("attn_split", S),), vt, split=S, merged=True))
    for D in (32, 64, 96, 128):
        for sched in (0, 1):
            knobs = (("attn_w4i_sched", sched),) + ((("attn_nw", 514),) if D in (64, 128) else ())
            cs.append(Case("generated", D, 768, f"attn_fwd_w4i_kernel<{D},{sched}>", knobs, merged=True))
    for N in (512, 1152):
        for vt, bf in ((False, False), (True, False), (False, True)):
            cs.append(Case("attn_bigd7", 256, N, f"attn_fwd_bigd7_kernel<{_tf(bf)},{_tf(vt)}>", (("attn_d512", 4),), vt, bf))
    cs.append(Case("attn_bigd2", 256, 384, "attn_fwd_bigd2_kernel<256,false,false>"))
    for D, vt, bf in ((256, False, False), (256, True, False), (256, False, True), (512, False, False), (512, False, True)):
        cs.append(Case("attn_bigd2", D, 512, f"attn_fwd_bigd2_kernel<{D},{_tf(bf)},{_tf(vt)}>", (("attn_d512", 3),), vt, bf))
    for D in (256, 512):
        cs.append(Case("attn_bigd3", D, 512, f"attn_fwd_bigd3_kernel<{D},false>", (("attn_d512", 2),)))
    for N in (256, 1024):
        for bf in (False, True):
            cs.append(Case("attn_bigd6", 512, N, f"attn_fwd_bigd6_kernel<{_tf(bf)}>", bf=bf))
    # D = 1024: five heads put blocks on all eight XCDs (as test_bigd_block_map_knob_computes_the_same_bits)
    cs.append(Case("attn_bigd4", 1024, 512, "attn_fwd_bigd4_kernel<8>", bh=5))
    for m in (1, 2):
        for stag in (1, 2):
            cs.append(Case("attn_bigd4", 1024, 512, "attn_fwd_bigd4_kernel<8>", (("attn_bigd_map", m), ("attn_bigd_stagger", stag)), bh=5))
    for span in (2, 4, 6):
        cs.append(Case("attn_bigd4", 1024, 512, f"attn_fwd_bigd4_kernel<{span}>", (("attn_d1024", span),), bh=5))
    cs.append(Case("attn_bigd4", 1024, 64, "attn_fwd_bigd4_kernel<8>", bh=5))
    for D in (256, 512, 1024):
        cs.append(Case("column-split", D, 256, f"attn_fwd_bigd_kernel<{D},256,4,false,false>", (("attn_d512", 1),)))
    cs.append(Case("column-split", 256, 192, "attn_fwd_bigd_kernel<256,256,2,false,false>"))                 # ragged N: auto
    cs.append(Case("column-split", 512, 256, "attn_fwd_bigd_kernel<512,256,4,true,false>", vt=True))          # D = 512 with V as [B,H,D,N]: auto
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
SHAPES = sorted({(c.D, c.N, c.bf, c.bh) for c in CASES})                         # what `pinned` and `step` depend on
SEAM_BH, SEAM_N = 130, 512                                                       # test_uniform_across_the_block_seam_of_the_persistent_walks
UNIFORM_SHAPES = sorted({(c.D, c.N, c.bf, c.bh, c.split) for c in CASES} | {(D, SEAM_N, False, SEAM_BH, 1) for D in (64, 128)})      # ... and `uniform`'s bound


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs and truths

def _dt(bf):
    return torch.bfloat16 if bf else torch.half


def _seed(kind, D, N, bf, h):
    return 1000003 * D + 101 * N + 500000 * int(bf) + 1009 * INPUTS.index(kind) + h


def _draw(g, table, shape):
    return torch.tensor(table, dtype=torch.float32)[torch.randint(0, len(table), shape, generator=g)]


def _pm1(g, shape):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(torch.float32)


def target_map(name, N, seed):
    """pi: row -> the key that scores SCORE for it (int64 [N])"""
    i = torch.arange(N)
    if name == "anywhere":
        return torch.randint(0, N, (N,), generator=torch.Generator().manual_seed(seed))
    if name == "reverse":
        return N - 1 - i
    if name == "edges":
        return 64 * ((i // 2) % (N // 64)) + 63 * (i % 2)
    raise KeyError(name)


def step_keys(N):
    return N // 2 + 24, min(N, N // 2 + 64)


@functools.lru_cache(maxsize=6)
def build_inputs(kind, D, N, bf=False, bh=BH):
    """(q, k, v, pi): CPU tensors [1, bh, N, D] of the launch's type and — `pinned` — the maps [bh, N]; a different seed per head"""
    qs, ks, vs, pis = [], [], [], []
    for h in range(bh):
        seed = _seed(kind, D, N, bf, h)
        g = torch.Generator().manual_seed(seed)
        if kind == "uniform":
            v, r, z = _draw(g, V16, (N, D)), _pm1(g, (N, D)), torch.zeros(N, D)
            q, k = (z, r) if h % 2 == 0 else (r, z)
        elif kind == "step":
            v, u, w = _draw(g, V8, (N, D)), _pm1(g, (D,)), _draw(g, V8, (D,))
            lo, hi = step_keys(N)
            k = torch.zeros(N, D)
            k[lo:hi] = u
            v[lo:hi] = w
            q = (torch.tensor(STEP_C)[torch.arange(N) % 3] / D ** 0.5).unsqueeze(1) * u
        else:
            k, v = _pm1(g, (N, D)), torch.randn(N, D, generator=g)
            pi = target_map(kind[len("pinned-"):], N, seed + 1)
            q = (SCORE / D ** 0.5) * k[pi]
            pis.append(pi)
        qs.append(q)
        ks.append(k)
        vs.append(v)
    q, k, v = (torch.stack(x).unsqueeze(0).to(_dt(bf)) for x in (qs, ks, vs))
    return q, k, v, (torch.stack(pis) if pis else None)


def _oracle_attn(oracle, q, k, v, bf):
    _, bh, N, D = q.shape
    o = oracle.attn_bf16(q, k, v, 1, bh, N, D) if bf else oracle.attn(q, k, v, 1, bh, N, D, mode="f32")
    return o[0].astype(np.float64)


@functools.lru_cache(maxsize=6)
def _truth(kind, D, N, bf, bh):
    """[bh, N, D] fp64: the oracle on the rounded inputs, once per (input, shape, type), shared by every knob value"""
    from tests import oracle_lib
    q, k, v, _ = build_inputs(kind, D, N, bf, bh)
    return _oracle_attn(oracle_lib.load(), q, k, v, bf)


def uniform_truth(D, N, bf, bh, split=1):
    """E [bh, D] and E_s [split, bh, D]: the fp64 means of V over all keys / over each KV range"""
    v = build_inputs("uniform", D, N, bf, bh)[2][0].double()
    return v.mean(dim=1).numpy(), v.view(bh, split, N // split, D).mean(dim=2).transpose(0, 1).numpy()


def ulp(x, bf):
    """spacing of fp16 / bf16 at |x| (the subnormal spacing below the smallest normal number, and at 0)"""
    mant, emin = (7, -126) if bf else (10, -14)
    x = np.abs(np.asarray(x, np.float64))
    e = np.where(x == 0, emin, np.maximum(np.frexp(x)[1] - 1, emin))
    return np.ldexp(1.0, e - mant)


def round_once(x, bf):
    """fp64 -> the output type, one rounding (callers pass values that fp32 holds exactly) -> fp64"""
    return torch.from_numpy(np.array(x, np.float64)).float().to(_dt(bf)).double().numpy()


def uniform_bound(E, Es, bf, split):
    return ulp(E, bf) if split == 1 else 2.0 ** -11 * np.abs(Es).mean(axis=0) + ulp(E, bf)


def pinned_bound(truth, bf):
    return (1.6e-2 + 2.0 ** -5 * np.abs(truth)) if bf else (8e-3 + tol.ATTN_RTOL_SPIKE * np.abs(truth))


def step_rtol(bf):
    return 2.0 ** -6 if bf else tol.ATTN_RTOL_SPIKE


def step_bound(truth, N, bf):
    """tol.attn_close's bound as an array"""
    return tol.attn_max_abs(N, bf) + step_rtol(bf) * np.abs(truth)


# ------------------------------------------------------------------------------------------------------------------------------------
# teeth (CPU)

def _fp64_attention(q, k, v):
    """one head: scores [N, N] and the weights exp(s - rowmax), fp64"""
    s = q.double() @ k.double().T / q.shape[1] ** 0.5
    return s, torch.exp(s - s.max(dim=-1, keepdim=True).values)


def _smallest_row_move(truth, wrong, bound):
    """smallest over the rows of the largest |wrong - truth| / bound over the row's columns, and its row"""
    ratio = (np.abs(wrong - truth) / bound).max(axis=-1)
    return float(ratio.min()), int(ratio.argmin())


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("D,N,bf,bh", SHAPES)
def test_pinned_dropping_the_target_tile_moves_every_row(D, N, bf, bh, name):
    q, k, v, pi = build_inputs("pinned-" + name, D, N, bf, bh)
    j = torch.arange(N).view(1, N)
    for h in range(bh):
        _, p = _fp64_attention(q[0, h], k[0, h], v[0, h])
        truth = ((p / p.sum(-1, keepdim=True)) @ v[0, h].double()).numpy()
        p = p.masked_fill(j // 64 == (pi[h] // 64).view(-1, 1), 0.0)      # what skipping that tile does; a row left with no key is zeros
        l = p.sum(-1, keepdim=True)
        wrong = (torch.where(l > 0, p / l.clamp(min=1e-300), torch.zeros_like(p)) @ v[0, h].double()).numpy()
        worst, row = _smallest_row_move(truth, wrong, pinned_bound(truth, bf))
        assert worst >= TEETH, (h, worst, row)


@pytest.mark.parametrize("D,N,bf,bh,split", [s for s in UNIFORM_SHAPES if s[1] > 64])
def test_uniform_a_tile_left_out_or_counted_twice_moves_every_head(D, N, bf, bh, split):
    v = build_inputs("uniform", D, N, bf, bh)[2][0].double()
    E, Es = uniform_truth(D, N, bf, bh, split)
    bound = uniform_bound(E, Es, bf, split)[:, None, :]                      # [bh, 1, D]
    tiles = v.view(bh, N // 64, 64, D).sum(dim=2).numpy()                    # [bh, T, D]
    total = tiles.sum(axis=1, keepdims=True)
    for what, wrong in (("left out", (total - tiles) / (N - 64)), ("counted twice", (total + tiles) / (N + 64))):
        ratio = (np.abs(wrong - E[:, None, :]) / bound).max(axis=-1)         # [bh, T]: the best column of every (head, tile)
        assert ratio.min() >= TEETH, (what, float(ratio.min()), np.unravel_index(ratio.argmin(), ratio.shape))


def _online_softmax(s, v, skip):
    """fp64 online softmax over 64-key tiles in key order; skip = "l" / "O": that accumulator is never rescaled when the running max rises"""
    N = s.shape[0]
    m = torch.full((N, 1), -float("inf"), dtype=torch.float64)
    l = torch.zeros(N, 1, dtype=torch.float64)
    o = torch.zeros(N, v.shape[1], dtype=torch.float64)
    for t in range(0, s.shape[1], 64):
        st = s[:, t:t + 64]
        m2 = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
        a, p = torch.exp(m - m2), torch.exp(st - m2)
        l = (l if skip == "l" else l * a) + p.sum(-1, keepdim=True)
        o = (o if skip == "O" else o * a) + p @ v[t:t + 64]
        m = m2
    return (o / l).numpy()


@pytest.mark.parametrize("D,N,bf,bh", [s for s in SHAPES if s[1] > 64])
def test_step_a_rescale_left_out_moves_every_row(D, N, bf, bh):
    q, k, v, _ = build_inputs("step", D, N, bf, bh)
    for h in range(bh):
        s, p = _fp64_attention(q[0, h], k[0, h], v[0, h])
        vh = v[0, h].double()
        truth = ((p / p.sum(-1, keepdim=True)) @ vh).numpy()
        assert np.abs(_online_softmax(s, vh, None) - truth).max() <= 1e-12
        for skip in ("l", "O"):
            worst, row = _smallest_row_move(truth, _online_softmax(s, vh, skip), step_bound(truth, N, bf))
            assert worst >= TEETH, (h, skip, worst, row)


def test_the_inputs_are_what_the_docstring_says():
    assert abs(sum(V16)) == 0 and set(V16) == set(V8)
    for D, N, bf in ((32, 320, False), (128, 1024, False), (256, 1152, True), (1024, 512, False)):
        for name in MAPS:
            q, k, v, pi = build_inputs("pinned-" + name, D, N, bf)
            assert (k.abs() == 1).all() and torch.isfinite(v.float()).all()
            s = (q[0].double() @ k[0].double().transpose(-2, -1)) / D ** 0.5
            hit = s.gather(-1, pi.unsqueeze(-1)).squeeze(-1)
            assert (hit - SCORE).abs().max().item() <= SCORE * (2.0 ** -8 if bf else 2.0 ** -11)      # the one rounding of Q
            assert s.max().item() <= 16.0
            assert not torch.equal(k[0, 0], k[0, 1]) and not torch.equal(v[0, 1], v[0, 2])              # a seed per head
        q, k, v, _ = build_inputs("uniform", D, N, bf)
        assert ((q[0].double() @ k[0].double().transpose(-2, -1)) == 0).all()
        assert (q[0, 0] == 0).all() and (k[0, 1] == 0).all() and (k[0, 0].abs() == 1).all() and (q[0, 1].abs() == 1).all()
        assert set(v.double().unique().tolist()) <= set(V8) and not torch.equal(v[0, 0], v[0, 2])
        assert (v.double() * 4 == (v.double() * 4).round()).all()                                      # multiples of 1/4: exact sums
        q, k, v, _ = build_inputs("step", D, N, bf)
        s = (q[0].double() @ k[0].double().transpose(-2, -1)) / D ** 0.5
        lo, hi = step_keys(N)
        c = torch.tensor(STEP_C, dtype=torch.float64)[torch.arange(N) % 3].view(1, N, 1)
        assert ((s[:, :, lo:hi] - c).abs() <= c * (2.0 ** -8 if bf else 2.0 ** -11)).all() and hi - lo == 40
        assert (s[:, :, :lo] == 0).all() and (s[:, :, hi:] == 0).all()
        assert set(v.double().unique().tolist()) <= set(V8) and (v[0, :, lo:hi] == v[0, :, lo:lo + 1]).all()
        assert not torch.equal(k[0, 0, lo], k[0, 1, lo])
    for N in (192, 1216, 2048):
        e = target_map("edges", N, 0)
        assert set(e.tolist()) == {64 * t + x for t in range(N // 64) for x in (0, 63)}
        assert torch.equal(target_map("reverse", N, 0)[[0, N - 1]], torch.tensor([N - 1, 0]))
        a = target_map("anywhere", N, 3)
        assert a.min() >= 0 and a.max() < N and (a[:64] >= N // 2).any() and (a[N - 64:] < N // 2).any()
    assert ulp(1.0, False) == 2.0 ** -10 and ulp(0.75, False) == 2.0 ** -11 and ulp(0.0, False) == 2.0 ** -24 and ulp(-3.0, True) == 2.0 ** -6
    assert round_once(1.0 + 2.0 ** -11 + 2.0 ** -20, False) == 1.0 + 2.0 ** -10


def test_the_fp64_torch_truths_are_the_oracles(oracle):
    """the anchor: on small shapes the project's oracle says what the fp64 torch restatements above say"""
    for D, N, bf in ((64, 320, False), (256, 256, True)):
        q, k, v, _ = build_inputs("uniform", D, N, bf)
        E, _ = uniform_truth(D, N, bf, BH)
        o = _oracle_attn(oracle, q, k, v, bf)
        assert (np.abs(o - E[:, None, :]) <= 2.0 ** -23 * np.abs(E[:, None, :])).all()      # (the oracle returns fp32)
        for kind in ("pinned-edges", "step"):
            q, k, v, _ = build_inputs(kind, D, N, bf)
            o = _oracle_attn(oracle, q, k, v, bf)
            for h in range(BH):
                _, p = _fp64_attention(q[0, h], k[0, h], v[0, h])
                assert np.abs(((p / p.sum(-1, keepdim=True)) @ v[0, h].double()).numpy() - o[h]).max() <= 1e-6


def test_every_case_names_its_kernel(built):
    """the plan needs no GPU: every case of the table reaches the kernel it names under the rule of a 256-CU device, and every path of
    the table is among them"""
    from leetcuda_amd import capi
    capi.load()
    seen = set()
    capi.tune("rule_cus", 256)
    try:
        for c in CASES:
            with _knobs(capi, c.knobs):
                assert capi.attn_kernel_name(c.N, c.D, c.vt, c.bf, bh=c.bh) == c.want, c.id
            seen.add(c.want.split("<")[0] + ("<..,3>" if c.split > 1 else ""))
    finally:
        capi.tune("rule_cus", 0)
    assert seen == {"attn_fwd_kernel", "attn_fwd_w4u_kernel", "attn_fwd_w4u_kernel<..,3>", "attn_fwd_w4i_kernel", "attn_fwd_bigd7_kernel",
                    "attn_fwd_bigd2_kernel", "attn_fwd_bigd3_kernel", "attn_fwd_bigd6_kernel", "attn_fwd_bigd4_kernel", "attn_fwd_bigd_kernel"}
    walks = {c.want[-2] for c in CASES if c.path.startswith("merged-phase")}
    assert walks == {"0", "1", "2"}


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernels (GPU)

@contextlib.contextmanager
def _knobs(capi, knobs):
    try:
        for key, val in knobs:
            capi.tune(key, val)
        yield
    finally:
        for key, _ in knobs:
            capi.tune(key, 1 if key == "attn_w4i_sched" else 0)      # (the defaults)


def _single_tile_fault(row, v):
    """`uniform`: the one-tile fault that explains an output row best — (tile, "left out" / "counted twice", largest residual)"""
    N = v.shape[0]
    tiles = v.reshape(N // 64, 64, -1).sum(axis=1)
    total = tiles.sum(axis=0, keepdims=True)
    best = None
    for what, hyp in (("left out", (total - tiles) / max(N - 64, 1)), ("counted twice", (total + tiles) / (N + 64))):
        res = np.abs(hyp - row[None, :]).max(axis=-1)
        t = int(np.nanargmin(res)) if np.isfinite(res).any() else 0
        if best is None or res[t] < best[2]:
            best = (t, what, float(res[t]))
    return best


def _report(kernel, wrong, err, excess, N, key_tile):
    """Where a check failed (wrong: bool, err / excess: float, all [bh, N, D]): report_worst_row's kernel, head, row, query block and wave,
    then the 64-key tile that key_tile(head, row) blames and the share of wrong elements"""
    score = np.where(wrong, np.maximum(np.nan_to_num(excess, nan=np.inf), 1e-300), -1.0)
    h, i, _ = (int(x) for x in np.unravel_index(np.argmax(score), score.shape))
    return (report_worst_row(score, kernel, err) + f"; {key_tile(h, i)} (of {N // 64} 64-key tiles); wrong: {wrong.mean():.2%} of all elements, "
            f"{wrong[h].mean():.2%} of head {h}, {int(wrong.any(axis=-1).sum())} of {wrong.shape[0] * wrong.shape[1]} rows")


def _judge(case, kind, name, out, slow):
    """out [bh, N, D] fp64 against the truth of `kind` under its bound; prints the worst |err| / bound first"""
    D, N, bf, bh = case.D, case.N, case.bf, case.bh
    finite = np.isfinite(out)
    if kind == "uniform":
        v = build_inputs(kind, D, N, bf, bh)[2][0].double().numpy()
        E, Es = uniform_truth(D, N, bf, bh, case.split)
        truth, bound = np.broadcast_to(E[:, None, :], out.shape), uniform_bound(E, Es, bf, case.split)[:, None, :]

        def key_tile(h, i):
            t, what, res = _single_tile_fault(out[h, i], v[h])
            return f"closest one-tile fault: key tile {t} {what} (residual {res:.2e})"
    elif kind == "step":
        truth = _truth(kind, D, N, bf, bh)
        bound = step_bound(truth, N, bf)
        lo, hi = step_keys(N)

        def key_tile(h, i):
            return f"c = {STEP_C[i % 3]:g}, the max rises in key tile {lo // 64}" + (f" and {(hi - 1) // 64}" if (hi - 1) // 64 != lo // 64 else "")
    else:
        truth = _truth(kind, D, N, bf, bh)
        bound = pinned_bound(truth, bf)
        pi = build_inputs(kind, D, N, bf, bh)[3]

        def key_tile(h, i):
            return f"pi(row) = key {int(pi[h, i])} = key tile {int(pi[h, i]) // 64}, key {int(pi[h, i]) % 64} of it"
    err = np.abs(out - truth)
    excess = err - bound
    strict = kind == "uniform" and case.split == 1      # |out - E| < ulp(E)
    wrong = ~finite | ((err >= bound) if strict else (err > bound))
    exact = strict and N & (N - 1) == 0
    print(f"[attn_exact] path={case.path} | kernel={name} | id={case.id} | input={kind} | worst_err={np.nanmax(err):.3e} | "
          f"worst_ratio={np.nanmax(err / bound):.4f}" + (f" | bit_equal={np.mean(out == round_once(truth, bf)):.6f}" if exact else ""))
    assert finite.all(), "not written / not finite: " + _report(name, ~finite, err, np.where(finite, -1.0, np.inf), N, key_tile)
    assert not wrong.any(), _report(name, wrong, err, excess, N, key_tile)
    if kind == "step":
        ok, mx, ex = tol.attn_close(out, truth, N, bf16=bf, rtol=step_rtol(bf))
        assert ok, (name, mx, ex)
    if exact:
        miss = out != round_once(truth, bf)
        assert not miss.any(), "not E rounded once: " + _report(name, miss, err, err, N, key_tile)
    if kind == "uniform" and case.merged:
        assert slow[0] == 0, (name, slow)


def _run_case(capi, case, kind):
    q, k, v, _ = build_inputs(kind, case.D, case.N, case.bf, case.bh)
    with _knobs(capi, case.knobs):
        name = capi.attn_kernel_name(case.N, case.D, case.vt, case.bf, bh=case.bh)
        assert name == case.want, (case.id, name)
        qg, kg, vg = (x.cuda() for x in (q, k, v))
        o = torch.full_like(qg, float("nan"))
        capi.attn_slowpath_stats(reset=True)
        if case.bf:
            capi.attn_fwd_bf16(qg, kg, vg, o)
        else:
            capi.attn_fwd(qg, kg, vg.transpose(-2, -1).contiguous() if case.vt else vg, o, v_transposed=case.vt)
        torch.cuda.synchronize()
        slow = capi.attn_slowpath_stats(reset=True)
    _judge(case, kind, name, o[0].double().cpu().numpy(), slow)
    return o


# sorted by shape, then input: the cases that share a truth follow each other
_PARAMS = sorted(((c, kind) for c in CASES for kind in INPUTS), key=lambda p: (p[0].D, p[0].N, p[0].bf, p[0].bh, INPUTS.index(p[1])))


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", [pytest.param(c, kind, id=f"{c.id}-{kind}") for c, kind in _PARAMS])
def test_every_element_of_every_path(case, kind):
    _run_case(_capi(), case, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("vt", [False, True], ids=["v_nd", "v_dn"])
@pytest.mark.parametrize("D", [64, 128])
def test_uniform_across_the_block_seam_of_the_persistent_walks(D, vt):
    """260 blocks on 256 CUs: the persistent walks (515 static, 517 dynamic queue) pass from one block to the next inside a workgroup,
    with the next block's first tiles fetched under the current one.  `uniform` only (its truth costs nothing); the three walks give
    the same bits, the dynamic one twice."""
    capi = _capi()
    bh, N = SEAM_BH, SEAM_N
    assert torch.cuda.get_device_properties(0).multi_processor_count < bh * (N // 256)
    outs = []
    for nw in (513, 515, 517, 517):
        case = Case("merged-phase block seam", D, N, f"attn_fwd_w4u_kernel<{D},{_tf(vt)},{(nw - 513) // 2}>", (("attn_nw", nw),), vt, bh=bh, merged=True)
        outs.append((nw, _run_case(capi, case, "uniform")))
    for nw, o in outs[1:]:
        assert torch.equal(outs[0][1], o), (D, vt, nw)
