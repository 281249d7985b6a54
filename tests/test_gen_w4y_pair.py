"""The pair loop of hgemm_w4y (tools/gen_hgemm_w4y.py -> hgemm_w4y_loop_pair.inc, the kernel's SCHED 2): both k-steps of an accumulator
block back to back.

The counts are read off the generated text; the dataflow is REPLAYED: the statement is interpreted as one wave executes it (scalar
registers, SCC, branches), LDS ring slots carry tile numbers, DMA pieces overwrite them, the barrier publishes, ds_reads copy
(operand, tile, k-step, fragment) tags into registers through the in-order LDS queue that s_waitcnt lgkmcnt(N) retires."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("lc_gen_w4y_pair", ROOT / "tools" / "gen_hgemm_w4y.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _vregs(tok):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    return tuple(range(int(m.group(1)), int(m.group(2)) + 1)) if m else (int(tok[1:]),)


def test_counts_per_k_tile(gen):
    for h in range(2):
        half = gen.gen_half(h)
        mf = [l for l in half if l.startswith("v_mfma")]
        assert len(mf) == 128
        assert sum(l.startswith("ds_read_b128") for l in half) == 32
        assert sum(l.startswith("buffer_load_dwordx4") for l in half) == 16
        assert half.count("s_barrier") == 1 and sum("vmcnt" in l for l in half) == 1
        # every accumulator block exactly twice, adjacent: SrcC of the second MFMA is the result of the first
        blocks = [l.split()[1].rstrip(",") for l in mf]
        assert blocks[0::2] == blocks[1::2] and len(set(blocks)) == 64
        assert all(l.split(",")[0].split()[1] == l.split(",")[3].strip() for l in mf)
        # the A fragment (SrcB) stays for the 8 pairs of a block row: 8 rows x 2 k-steps
        a_ops = [l.split(",")[2].strip() for l in mf]
        assert all(len(set(a_ops[16 * i + ks:16 * i + 16:2])) == 1 for i in range(8) for ks in range(2))
        assert len(set(a_ops)) == 16
        # the 16 DMA pieces keep their placement: B pieces one per 8 MFMAs from MFMA 4, A pieces one per 7 from the third MFMA behind the barrier
        pos, n = [], 0
        for l in half:
            n += l.startswith("v_mfma")
            if l.startswith("buffer_load"):
                pos.append(n)
        assert pos == [5 + 8 * p for p in range(8)] + [68 + 7 * g for g in range(8)]
    text = gen.render(2, pair=True)
    assert text == (ROOT / "leetcuda_amd" / "csrc" / "hgemm_w4y_loop_pair.inc").read_text()   # the committed file is current
    regs = {int(r) for r in re.findall(r'"v(\d+)"', text)}
    assert regs == set(range(60, 256))   # the clobber list names every literal VGPR (check_literal_vgprs ran inside render)


def _replay(gen, kt):
    """Interpret gen.gen_pair() for one C tile of `kt` K tiles (wave 0, stagger 0).  Returns the number of MFMAs executed."""
    lines = gen.gen_pair()
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    BLK = 1 << 20   # bytes between DMA pieces of the source: piece g of tile T comes from offset g * BLK + 128 T
    A0 = 0x1000
    s = {"kt": kt, "stg": 0, "a0": A0, "wv": 0, "blk": BLK}
    scc = 0
    slot_of = lambda addr: (addr - A0) // 0x8000
    # LDS: slot -> per piece [state, tile]; the prologue of the kernel staged tiles 0 / 1 into A slots 0 / 1 and B slots 0 / 1 (slots 2, 3)
    lds = {sl: [["ok", t] for _ in range(8)] for sl, t in ((0, 0), (1, min(1, kt - 1)), (2, 0), (3, min(1, kt - 1)))}
    lds[4] = [["junk", None] for _ in range(8)]
    dma_q = []          # issued LDS-DMA pieces, oldest first: (slot, piece, tile)
    landed = []         # landed but not yet published by a barrier
    read_since_barrier = set()   # slots this wave has read since the last barrier
    vaddr = {}          # address VGPR -> (slot, operand, k-step)
    tag = {}            # fragment VGPR -> (operand, tile, k-step, fragment) or None
    uses = {}           # tag -> MFMAs that consumed it
    lgkm = []           # outstanding ds_reads, oldest first: (regs, tag)
    inflight = set()    # VGPRs with an outstanding read
    hits = [0] * 64     # MFMAs per accumulator block
    n_mfma = 0

    def val(tok):
        tok = tok.strip()
        if tok.startswith("%["):
            return s[tok[2:-1]]
        if tok == "m0":
            return s["m0"]
        return int(tok, 0)

    def setr(tok, v):
        s[tok[2:-1] if tok.startswith("%[") else tok] = v & 0xffffffff

    pc = 0
    while pc < len(lines):
        ln = lines[pc]
        pc += 1
        if ln.endswith(":"):
            continue
        op, _, rest = ln.partition(" ")
        args = [a.strip() for a in rest.split(",")] if rest else []
        if op == "s_mov_b32":
            setr(args[0], val(args[1]))
        elif op == "s_add_u32":
            setr(args[0], val(args[1]) + val(args[2]))
        elif op == "s_sub_u32":
            setr(args[0], val(args[1]) - val(args[2]))
        elif op == "s_min_u32":
            setr(args[0], min(val(args[1]), val(args[2])))
        elif op == "s_lshl_b32":
            setr(args[0], val(args[1]) << val(args[2]))
        elif op == "s_cmp_ge_u32":
            scc = int(val(args[0]) >= val(args[1]))
        elif op == "s_cmp_lt_u32":
            scc = int(val(args[0]) < val(args[1]))
        elif op == "s_cselect_b32":
            setr(args[0], val(args[1]) if scc else val(args[2]))
        elif op in ("s_cbranch_scc0", "s_cbranch_scc1"):
            if scc == int(op[-1]):
                pc = labels[args[0]]
        elif op == "v_add_u32_e32":
            kind = args[2][2:-1]   # ar0 / ar1 / br0 / br1
            sl = slot_of(val(args[1]))
            assert (kind[0] == "a") == (sl < 2), ln
            vaddr[args[0]] = (sl, kind[0].upper(), int(kind[2]))
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", ln)
            if m:
                keep = int(m.group(1))
                assert keep <= 15   # a 4-bit counter
                for regs, tg in lgkm[:len(lgkm) - keep]:
                    for r in regs:
                        tag[r] = tg
                        inflight.discard(r)
                lgkm = lgkm[len(lgkm) - keep:] if keep else []
            m = re.search(r"vmcnt\((\d+)\)", ln)
            if m:
                keep = int(m.group(1))
                landed += dma_q[:len(dma_q) - keep]
                dma_q = dma_q[len(dma_q) - keep:] if keep else []
        elif op == "s_barrier":
            assert not lgkm, "a barrier with fragment reads outstanding does not say that this wave is done with the old tile"
            for sl, g, t in landed:
                lds[sl][g] = ["ok", t]
            landed = []
            read_since_barrier = set()
        elif op == "ds_read_b128":
            dst = _vregs(args[0])
            addr, off = args[1].split()
            sl, operand, ks = vaddr[addr]
            frag = int(off.split(":")[1]) // 2048
            assert 0 <= frag < 8
            pieces = lds[sl]
            ok = all(p[0] == "ok" and p[1] == pieces[0][1] for p in pieces)
            tg = (operand, pieces[0][1], ks, frag) if ok else None
            # no read lands in a register that a pending MFMA still has to read, or that has a read outstanding already
            for r in dst:
                assert r not in inflight, ln
                old = tag.get(r)
                assert old is None or old[1] >= kt or uses.get(old, 0) == 8, (ln, old, uses.get(old, 0))
                inflight.add(r)
            lgkm.append((dst, tg))
            read_since_barrier.add(sl)
        elif op == "buffer_load_dwordx4":
            assert args[-1].endswith("offen lds")
            operand = {"%[ra]": "A", "%[rb]": "B"}[args[1]]
            soff = val(args[2].split()[0])
            g, t = soff // BLK, (soff % BLK) // 128
            dstaddr = s["m0"]
            sl = slot_of(dstaddr)
            assert (operand == "A") == (sl < 2) and (dstaddr - A0) % 0x8000 == g * 4096, ln
            assert t == min(t, kt - 1) and 0 <= g < 8
            # the slot is dead for every wave: this wave's own reads of it lie before a barrier it has passed
            assert sl not in read_since_barrier, ln
            lds[sl][g] = ["flying", t]
            dma_q.append((sl, g, t))
        elif op == "v_mfma_f32_16x16x32_f16":
            acc_d, src_a, src_b, acc_c = args
            assert acc_d == acc_c
            blk = int(re.match(r"a\[(\d+):", acc_d).group(1)) // 4
            i, j = blk >> 3, blk & 7
            t, ks = hits[blk] // 2, hits[blk] % 2
            hits[blk] += 1
            n_mfma += 1
            for tok, want in ((src_a, ("B", t, ks, j)), (src_b, ("A", t, ks, i))):
                regs = _vregs(tok)
                assert len(regs) == 4
                for r in regs:
                    assert r not in inflight, (ln, "operand read still outstanding")
                    assert tag.get(r) == want, (ln, tag.get(r), want)
                uses[want] = uses.get(want, 0) + 1
        else:
            raise AssertionError("unknown instruction: " + ln)
    assert not lgkm and not dma_q   # the statement ends on vmcnt(0) lgkmcnt(0)
    assert hits == [2 * kt] * 64
    assert all(n == 8 for n in uses.values()) and len(uses) == 32 * kt
    return n_mfma


@pytest.mark.parametrize("kt", [1, 2, 3, 4, 5, 7, 8])
def test_replay_every_mfma_consumes_the_fragments_of_its_tile(gen, kt):
    """KT = 1 leaves after the first half at once, odd KT after the first half of a later trip, even KT after the second; 7 tiles walk
    the 2-slot A ring and the 3-slot B ring through one full cycle of their relative positions."""
    assert _replay(gen, kt) == 128 * kt


def test_the_k_step_outer_bodies_and_their_clobbers_are_untouched(gen):
    for sched in (0, 1, 2):
        mf = [l for l in gen.gen(sched) if l.startswith("v_mfma")]
        blocks = [l.split()[1] for l in mf]
        assert len(mf) == 128 and blocks[:64] == blocks[64:]
        assert {int(r) for r in re.findall(r'"v(\d+)"', gen.render(sched))} == set(range(124, 256))
