"""What the rotary-embedding + append test modules share (tests/test_abi_cpu_rope.py, tests/test_gpu_rope.py); not a test module and not a
conftest: nothing here is collected.  Built on tests/append_lib.py (geometry, tables, sentinels, placement) and tests/decode_lib.py (fp8 codes).

`rope_ref` is the exact rotation in float64 from the fp16 inputs and the fp32 table, with the error scale of every element; `violations` /
`check_bound` are the DERIVED check of a stored fp16 value:

    |got - exact| <= e + half_ulp16(|exact| + e),   e = 2^-22 (|x1 c| + |x2 s|),   half_ulp16(a) = 2^(max(floor(log2 a), -14) - 11)

Any fp32 evaluation of x1 c -+ x2 s, with or without FMA contraction, is within 2^-23 (|x1 c| + |x2 s|) of exact up to second-order terms, for
which e allows a factor of two; the single rounding to fp16 of a value of magnitude <= |exact| + e adds the second term.  Nothing in it comes
from what a kernel gives.  `rope_model` is the reference on Q, K and V together, or ONE wrong kernel restated (FAULTS), so that the CPU module
can prove that the GPU tests' inputs have teeth: each fault leaves the bound on the base-10000 table, and differs from the reference on the
quarter-turn table — except table_fp16 and kv8_unrounded, which that table cannot show (its entries, and the K it rotates, are exact in fp16)."""
import functools

import torch

from leetcuda_amd import capi
from tests import append_lib as al
from tests.decode_lib import quantize

B, HKV, NCAP, LENS = al.B, al.HKV, al.NCAP, al.LENS
HS = (2, 8)                              # G = 1 and 4
GRID_NQ = (1, 5, 16, 100)                # 5 and 100 leave a partial last workgroup; 100 > 65 gives left padding
DS, PAGE_SIZES, KINDS = al.DS, al.PAGE_SIZES, al.KINDS
MAX_POS = 1024
SHORT_MAX_POS = 100                      # the table shorter than the cache: positions up to 776 read row 99
QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))       # (cos, sin) of 0, 1, 2, 3 quarter turns, as literals
FAULTS = ("pairing_swapped", "reverse", "pos_len_plus_i", "pos_i", "q_pos_row", "tail_rotated", "cos_sin_swapped", "table_fp16",
          "kv8_unrounded", "kv8_k_unrotated", "q_page_dropped", "unclamped_row")


def rot_dims(D):
    return (D, D // 2, 16)


@functools.lru_cache(maxsize=16)
def random_table(rot_dim, max_pos=MAX_POS):
    """the base-10000 table (capi.rope_table): float32 [max_pos, rot_dim]"""
    return capi.rope_table(max_pos, rot_dim)


@functools.lru_cache(maxsize=16)
def pinned_table(rot_dim, max_pos=MAX_POS):
    """the quarter-turn table: (cos, sin) of position t, pair j is entry (t (2j + 1) + t // 4) mod 4 of QUARTER — every rotation an exact signed
    permutation that differs between neighbouring positions, between t and t + 4, and between pairs"""
    t = torch.arange(max_pos)[:, None]
    j = torch.arange(rot_dim // 2)[None, :]
    k = (t * (2 * j + 1) + t // 4) % 4
    quarter = torch.tensor(QUARTER, dtype=torch.float32)
    return torch.cat([quarter[k, 0], quarter[k, 1]], dim=1).contiguous()


def positions(lens, Nq, ncap=NCAP):
    """int64 [B, Nq]: p = clamp(kv_len, 0, ncap) - Nq + i"""
    L = torch.tensor([min(max(int(x), 0), ncap) for x in lens])
    return L[:, None] - Nq + torch.arange(Nq)[None, :]


def _pairs(x, rot_dim, interleaved):
    """(x1, x2): the two elements of every pair of [..., D]"""
    if interleaved:
        return x[..., 0:rot_dim:2], x[..., 1:rot_dim:2]
    return x[..., :rot_dim // 2], x[..., rot_dim // 2:rot_dim]


def _unpair(o1, o2, tail, interleaved):
    if interleaved:
        rot = torch.stack([o1, o2], dim=-1).flatten(-2)
    else:
        rot = torch.cat([o1, o2], dim=-1)
    return torch.cat([rot, tail], dim=-1)


def rope_ref(x, pos, table, interleaved):
    """(exact, e) float64 of x's shape: x fp16 [B,heads,Nq,D] rotated at positions pos (int [B,Nq] or [B,heads,Nq]; the row read is clamped to
    [0, max_pos - 1]) and e = 2^-22 (|x1 c| + |x2 s|) per element; elements behind rot_dim: exact = x, e = 0"""
    max_pos, rot_dim = table.shape
    if pos.dim() == 2:
        pos = pos[:, None, :]
    cs = table.double()[pos.clamp(0, max_pos - 1)]                      # [B, 1 or heads, Nq, rot_dim]
    c, s = cs[..., :rot_dim // 2], cs[..., rot_dim // 2:]
    xd = x.double()
    x1, x2 = _pairs(xd, rot_dim, interleaved)
    tail = xd[..., rot_dim:]
    exact = _unpair(x1 * c - x2 * s, x2 * c + x1 * s, tail, interleaved)
    e = _unpair((x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs(), torch.zeros_like(tail), interleaved) * 2.0 ** -22
    return exact, e


def half_ulp16(a):
    """2^(max(floor(log2 a), -14) - 11) for a >= 0 (float64); a = 0: 2^-25"""
    _, ex = torch.frexp(a)                                                # a = m 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    fl = torch.where(a > 0, ex - 1, torch.full_like(ex, -14)).clamp(min=-14)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (fl - 11).double())


def violations(got16, exact, e):
    """bool, got's shape: where the stored fp16 value leaves the bound (a NaN leaves it)"""
    tol = e + half_ulp16(exact.abs() + e)
    return ~((got16.double() - exact).abs() <= tol)


def check_bound(got16, exact, e, what):
    bad = violations(got16, exact, e)
    assert not bad.any(), (what, f"{int(bad.sum())} of {bad.numel()} elements leave the bound, the first at {tuple(int(v) for v in bad.nonzero()[0])}: "
                           f"got {float(got16[bad][0])}, exact {float(exact[bad][0])}, e {float(e[bad][0]):.3e}")


def place(pool, rows, table, lens):
    """al.append_ref on rows of the pool's own dtype (no quantisation): pool [P,Hkv,ps,D] written in place"""
    return al.append_ref(pool, rows, table, lens, None)


def zero_codes(codes):
    """e4m3 codes with -0 (0x80) folded onto +0: a signed permutation may give either zero"""
    return torch.where(codes == 0x80, torch.zeros_like(codes), codes)


@functools.lru_cache(maxsize=256)
def grid_inputs(D, ps, Nq, H):
    """(q [B,H,Nq,D], k_new, v_new [B,Hkv,Nq,D], table, P, lens): append_lib's grid inputs + a Q; shared, never written to"""
    k_new, v_new, table, P, lens = al.grid_inputs(D, ps, Nq)
    q = torch.randn(B, H, Nq, D, generator=torch.Generator().manual_seed(7919 * D + 17 * ps + 3 * Nq + H)).half()
    return q, k_new, v_new, table, P, lens


@functools.lru_cache(maxsize=16)
def edge_inputs(D, ps, H=8):
    k_new, v_new, table, P, lens = al.edge_inputs(D, ps)
    q = torch.randn(len(lens), H, al.EDGE_NQ, D, generator=torch.Generator().manual_seed(13 * D + ps)).half()
    return q, k_new, v_new, table, P, lens


@functools.lru_cache(maxsize=16)
def table_inputs(D, ps, H=8):
    """append_lib.table_inputs (bad and foreign page ids) + a Q; the last element: dropped positions per batch entry"""
    k_new, v_new, table, P, lens, dropped = al.table_inputs(D, ps)
    q = torch.randn(B, H, k_new.shape[2], D, generator=torch.Generator().manual_seed(29 * D + ps)).half()
    return q, k_new, v_new, table, P, lens, dropped


@functools.lru_cache(maxsize=1)
def all_values_inputs():
    """(q, k_new, v_new [1,4,512,128], table, P, lens): every head of K and of Q holds every FINITE fp16 bit pattern, denormals included (the
    2 048 non-finite patterns are replaced by finite ones), shuffled; append_lib.all_values_inputs' geometry"""
    k_new, v_new, table, P, lens, _, _ = al.all_values_inputs()
    g = torch.Generator().manual_seed(4242)

    def finite(x):
        b = al.bits(x).clone()
        nonfinite = (b & 0x7C00) == 0x7C00
        b[nonfinite] = (b[nonfinite] & ~0x4000).to(torch.int16)          # exponent 31 -> 15: a finite pattern, all finite ones stay present
        return b.view(torch.half)
    q = torch.stack([al.bits(k_new)[0, h].flatten()[torch.randperm(65536, generator=g)] for h in range(4)]).view(1, 4, 512, 128).view(torch.half)
    k_new, q, v_new = finite(k_new), finite(q), finite(v_new)
    assert all(len(set(al.bits(x)[0, h].flatten().tolist())) == 65536 - 2048 for x in (k_new, q) for h in range(4))
    return q, k_new, v_new, table, P, lens


def pack_qkv(q, k_new, v_new, pad=0):
    """[B,Nq,(H + 2 Hkv) D] token-major, a view of rows `pad` elements longer (pad: a multiple of 8) filled with a distinctive value"""
    Bn, H, Nq, D = q.shape
    rows = torch.cat([x.transpose(1, 2).reshape(Bn, Nq, -1) for x in (q, k_new, v_new)], dim=2)
    wide = torch.full((Bn, Nq, rows.shape[2] + pad), -9.0, dtype=torch.half)
    wide[:, :, :rows.shape[2]] = rows
    return wide


def rope_rows(x, pos, table, interleaved, fault=None, long_table=None):
    """fp16: what ONE kernel stores for rows x at positions pos — the reference rounded once (fault None), or a wrong kernel's rotation"""
    max_pos, rot_dim = table.shape
    if fault == "pairing_swapped":
        interleaved = not interleaved
    if fault == "cos_sin_swapped":
        table = torch.cat([table[:, rot_dim // 2:], table[:, :rot_dim // 2]], dim=1)
    if fault == "reverse":
        table = torch.cat([table[:, :rot_dim // 2], -table[:, rot_dim // 2:]], dim=1)
    if fault == "table_fp16":
        table = table.half().float()
    if fault == "unclamped_row":
        table = long_table                                              # what lies behind the table: here, the rows a longer table holds
    exact, _ = rope_ref(x, pos, table, interleaved)
    if fault == "tail_rotated" and rot_dim < x.shape[-1]:                 # the tail goes through the same pairs, in blocks of rot_dim
        for lo in range(rot_dim, x.shape[-1], rot_dim):
            blk = x[..., lo:lo + rot_dim]
            if blk.shape[-1] == rot_dim:
                exact[..., lo:lo + rot_dim] = rope_ref(blk, pos, table, interleaved)[0]
    return exact.half()


def rope_model(q, k_new, v_new, block_table, P, lens, ps, table, interleaved, kv8=False, k_scale=None, v_scale=None, fault=None, long_table=None,
               unwritten=float("nan")):
    """(q_out fp16 [B,H,Nq,D], k_pool, v_pool from sentinel pools) after one call; fault None: the reference rounded once; else ONE wrong
    kernel (FAULTS).  Q rows a wrong kernel leaves unwritten hold `unwritten`."""
    Bn, H, Nq, D = q.shape
    Hkv = k_new.shape[1]
    G = H // Hkv
    mp = block_table.shape[1]
    pos = positions(lens, Nq, mp * ps)
    L = pos[:, -1:] + 1
    i = torch.arange(Nq)[None, :]
    rot_pos = {"pos_len_plus_i": L + i, "pos_i": i.expand(Bn, Nq)}.get(fault, pos)
    qpos = rot_pos[:, None, :].expand(Bn, H, Nq)
    if fault == "q_pos_row":
        qpos = qpos + (torch.arange(H) % G)[None, :, None] * Nq          # row r = g Nq + i of the K / V head instead of token i
    rot_fault = fault if fault in ("pairing_swapped", "reverse", "tail_rotated", "cos_sin_swapped", "table_fp16", "unclamped_row") else None
    q_out = rope_rows(q, qpos, table, interleaved, rot_fault, long_table)
    q_out[(pos < 0)[:, None, :].expand(Bn, H, Nq)] = 0.0
    if fault == "q_page_dropped":
        for b in range(Bn):
            for t in range(Nq):
                p = int(pos[b, t])
                if p >= 0 and not 0 <= int(block_table[b, p // ps]) < P:
                    q_out[b, :, t] = unwritten
    kr = rope_rows(k_new, rot_pos, table, interleaved, rot_fault, long_table)
    kp, vp = al.sentinel_pools(P, Hkv, ps, D, kv8)
    if kv8:
        ks = 1.0 if k_scale is None else k_scale
        vs = 1.0 if v_scale is None else v_scale
        if fault == "kv8_unrounded":
            kc = quantize(rope_ref(k_new, rot_pos, table, interleaved)[0].float(), ks)       # the codes of the fp32 value
        elif fault == "kv8_k_unrotated":
            kc = quantize(k_new, ks)
        else:
            kc = quantize(kr, ks)
        place(kp, kc, block_table, lens)
        place(vp, quantize(v_new, vs), block_table, lens)
    else:
        place(kp, kr, block_table, lens)
        place(vp, v_new, block_table, lens)
    return q_out, kp, vp


def pool_truth(k_new, block_table, P, lens, ps, table, interleaved):
    """(exact, e, written) in the pool's layout [P,Hkv,ps,D]: the exact rotated K rows where a token lands, NaN (written False) elsewhere"""
    Hkv, Nq, D = k_new.shape[1:]
    exact, e = rope_ref(k_new, positions(lens, Nq, block_table.shape[1] * ps), table, interleaved)
    pe = place(torch.full((P, Hkv, ps, D), float("nan"), dtype=torch.float64), exact, block_table, lens)
    pb = place(torch.zeros((P, Hkv, ps, D), dtype=torch.float64), e, block_table, lens)
    return pe, pb, ~torch.isnan(pe)


def q_truth(q, lens, ncap, table, interleaved):
    """(exact, e) of Qout: the rotated rows, zeros (e = 0) where the position is negative"""
    Bn, H, Nq, D = q.shape
    pos = positions(lens, Nq, ncap)
    exact, e = rope_ref(q, pos, table, interleaved)
    pad = (pos < 0)[:, None, :, None].expand_as(exact)
    return exact.masked_fill(pad, 0.0), e.masked_fill(pad, 0.0)


def check_pool(got_pool, k_new, block_table, P, lens, ps, table, interleaved, what):
    """an fp16 K pool after a call from sentinel pools: the bound on every written element, bit-exact tails, the sentinel everywhere else"""
    pe, pb, written = pool_truth(k_new, block_table, P, lens, ps, table, interleaved)
    assert torch.equal(al.bits(got_pool)[~written], torch.full_like(al.bits(got_pool)[~written], al.SENT16)), (what, "a row nobody names was written")
    check_bound(got_pool[written], pe[written], pb[written], what)
    rot_dim = table.shape[1]
    if rot_dim < got_pool.shape[-1]:
        tail = written[..., rot_dim:]
        assert torch.equal(got_pool[..., rot_dim:][tail].double(), pe[..., rot_dim:][tail]), (what, "the partial-rotary tail is not a copy")
    return written
