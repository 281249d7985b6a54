"""GPU tests of the rotary-embedding + append kernels (lc_rope_append_paged_f16, lc_rope_append_paged_kv8) on the MI355X.  Pools and Qout are
prefilled with a sentinel and sit between guard elements; every rotated element is judged by the DERIVED bound of tests/rope_lib.py against the
float64 reference (no exceptions), or — on the quarter-turn table — must equal it; V pools, untouched rows and guards are compared on bits.  The
inputs are those tests/test_abi_cpu_rope.py proves to have teeth."""
import pytest
import torch

from tests import append_lib as al
from tests import decode_lib as dl
from tests import rope_lib as rl
from tests.decode_lib import _capi, _oracle, check_decode, decode_truth, gather, quantize

pytestmark = pytest.mark.gpu
TGUARD = 4097                            # floats in front of a table on the GPU: an odd count, so the table is aligned as floats are and no more


def _guarded(t):
    """(buf, view): an fp16 / uint8 CPU tensor on the GPU between al.GUARD sentinel elements either side"""
    sent = al.SENT8 if t.dtype == torch.uint8 else al.SENT16
    raw = al.bits(t).flatten()
    guard = torch.full((al.GUARD,), sent, dtype=raw.dtype)
    buf = torch.cat([guard, raw, guard]).cuda()
    view = buf[al.GUARD:al.GUARD + raw.numel()].view(t.shape)
    return buf, (view.view(torch.half) if t.dtype == torch.half else view)


def _guards_hold(buf, what):
    sent = al.SENT8 if buf.dtype == torch.uint8 else al.SENT16
    got = buf.cpu()
    assert (got[:al.GUARD] == sent).all() and (got[-al.GUARD:] == sent).all(), (what, "a guard was written")


def _table_dev(table):
    """the table at the END of a guarded allocation, TGUARD floats in: nothing of the allocation lies behind its last row"""
    buf = torch.cat([torch.full((TGUARD,), 7.5), table.flatten()]).cuda()
    return buf, buf[TGUARD:].view(table.shape)


def _call(kind, inputs, ps, table, il, layout="dense", inplace=False):
    """one call from sentinel pools and a sentinel Qout: (q_out, k_pool, v_pool) on the CPU, after the guards and the sources were checked.
    layout: dense | packed (the minimal row stride) | padded (64 elements more)"""
    capi = _capi()
    q, k_new, v_new, bt, P, lens = inputs[:6]
    kv8 = kind != "f16"
    Bn, H, Nq, D = q.shape
    Hkv = k_new.shape[1]
    ks, vs = al.kind_scales(kind, Hkv)
    dks, dvs = (None, None) if ks is None else (ks.cuda(), vs.cuda())
    bufs, views = zip(*(_guarded(p) for p in al.sentinel_pools(P, Hkv, ps, D, kv8)))
    qbuf, qout = _guarded(torch.full(q.shape, al.SENT16, dtype=torch.int16).view(torch.half))
    tbuf, cs = _table_dev(table)
    btd, ld = bt.cuda(), torch.tensor(list(lens), dtype=torch.int32).cuda()
    scale_kw = dict(k_scale=dks, v_scale=dvs) if kv8 else {}
    if layout == "dense":
        qd, kd, vd = q.cuda(), k_new.cuda(), v_new.cuda()
        fn = capi.rope_append_paged_kv8 if kv8 else capi.rope_append_paged
        got = fn(qd, kd, vd, views[0], views[1], cs, btd, ld, q_out=qd if inplace else qout, interleaved=il, **scale_kw)
        assert got is (qd if inplace else qout)
        torch.cuda.synchronize()
        if inplace:
            qout = qd
        else:
            assert torch.equal(al.bits(qd.cpu()), al.bits(q))
        assert torch.equal(al.bits(kd.cpu()), al.bits(k_new)) and torch.equal(al.bits(vd.cpu()), al.bits(v_new))
    else:
        wide = rl.pack_qkv(q, k_new, v_new, pad=64 if layout == "padded" else 0)
        wd = wide.cuda()
        W = (H + 2 * Hkv) * D
        capi.rope_append_paged_qkv(wd[:, :, :W], H, Hkv, views[0], views[1], cs, btd, ld, q_out=qout, interleaved=il, **scale_kw)
        torch.cuda.synchronize()
        assert torch.equal(al.bits(wd.cpu()), al.bits(wide))
    for buf in (*bufs, qbuf):
        _guards_hold(buf, (kind, layout))
    assert torch.equal(tbuf.cpu()[:TGUARD], torch.full((TGUARD,), 7.5)) and torch.equal(cs.cpu(), table)
    assert torch.equal(btd.cpu(), bt) and [int(x) for x in ld.cpu()] == list(lens)
    return qout.cpu(), views[0].cpu(), views[1].cpu()


def _check_q(got, q, lens, table, il, pinned, what):
    qe, qb = rl.q_truth(q, lens, al.NCAP, table, il)
    if pinned:
        assert torch.equal(got.double(), qe), (what, "Qout differs from the exact signed permutation")
    else:
        rl.check_bound(got, qe, qb, (what, "Qout"))
    rot = table.shape[1]
    pad = (rl.positions(lens, q.shape[2]) < 0)[:, None, :, None].expand_as(got)
    assert (al.bits(got)[pad] == 0).all(), (what, "a left-padded Qout row is not zeros")
    keep = ~pad[..., rot:]
    assert torch.equal(al.bits(got[..., rot:])[keep], al.bits(q[..., rot:])[keep]), (what, "the partial-rotary tail of Qout is not a copy")


def _check_v(got_v, inputs, ps, kind, what):
    q, k_new, v_new, bt, P, lens = inputs[:6]
    kv8 = kind != "f16"
    _, vs = al.kind_scales(kind)
    want = al.append_ref(al.sentinel_pools(P, k_new.shape[1], ps, k_new.shape[3], kv8)[1], v_new, bt, lens, (1.0 if vs is None else vs) if kv8 else None)
    assert torch.equal(al.bits(got_v), al.bits(want)), (what, "the V pool is not append_ref's")


def _check_k16(got_k, inputs, ps, table, il, pinned, what):
    q, k_new, v_new, bt, P, lens = inputs[:6]
    written = rl.check_pool(got_k, k_new, bt, P, lens, ps, table, il, (what, "K pool"))
    if pinned:
        pe = rl.pool_truth(k_new, bt, P, lens, ps, table, il)[0]
        assert torch.equal(got_k[written].double(), pe[written]), (what, "the K pool differs from the exact signed permutation")
    return written


def _codes_of(k16_pool, written, kind, P, Hkv, ps, D):
    """the fp8 K pool the fp8 entry must write, from what the fp16 entry wrote: kv_append_paged_kv8's codes of the rows, the sentinel elsewhere"""
    ks, _ = al.kind_scales(kind)
    want = quantize(torch.where(written, k16_pool, torch.zeros_like(k16_pool)), 1.0 if ks is None else ks)
    return torch.where(written, want, torch.full_like(want, al.SENT8))


# ---- 1. the grid

@pytest.mark.parametrize("kind", rl.KINDS)
@pytest.mark.parametrize("ps", rl.PAGE_SIZES)
@pytest.mark.parametrize("D", rl.DS)
def test_grid_against_the_reference(D, ps, kind):
    """D x page size x {fp16, fp8 under scales, fp8 with NULL scales}, and inside: H in {2, 8} x Nq in {1, 5, 16, 100} x rot_dim in {D, D/2, 16} x
    both pairings x {base-10000 table: the bound; quarter-turn table: equal}, lens (777, 129, 65)"""
    capi = _capi()
    for H in rl.HS:
        for Nq in rl.GRID_NQ:
            inputs = rl.grid_inputs(D, ps, Nq, H)
            q, k_new, v_new, bt, P, lens = inputs
            for rot in rl.rot_dims(D):
                for il in (False, True):
                    assert capi.rope_append_paged_kernel_name(rl.B, H, rl.HKV, Nq, ps, al.NCAP // ps, D, rot, rl.MAX_POS, interleaved=il, kv8=kind != "f16") == \
                        f"rope_append_paged_{'' if kind == 'f16' else 'kv8_'}kernel<{D},{'true' if il else 'false'}>"
                    for pinned in (False, True):
                        what = (D, ps, kind, H, Nq, rot, il, pinned)
                        table = rl.pinned_table(rot) if pinned else rl.random_table(rot)
                        qo, kp, vp = _call(kind, inputs, ps, table, il)
                        _check_q(qo, q, lens, table, il, pinned, what)
                        _check_v(vp, inputs, ps, kind, what)
                        if kind == "f16":
                            _check_k16(kp, inputs, ps, table, il, pinned, what)
                        else:       # the identity: the codes of what the fp16 entry writes (which the f16 cases judge)
                            qo16, kp16, _ = _call("f16", inputs, ps, table, il)
                            written = _check_k16(kp16, inputs, ps, table, il, pinned, what)
                            assert torch.equal(al.bits(qo), al.bits(qo16)), (what, "Qout differs between the fp16 and the fp8 entry")
                            assert torch.equal(kp, _codes_of(kp16, written, kind, P, rl.HKV, ps, D)), (what, "fp8 K codes")


@pytest.mark.parametrize("kind", ("f16", "kv8"))
def test_every_finite_fp16_value_goes_through_q_and_k_unchanged_by_a_quarter_turn(kind):
    """B = 1, H = Hkv = 4, Nq = 512, D = 128: every head of Q and K holds every finite fp16 bit pattern, denormals included; on the quarter-turn
    table every output is an input of the same row, possibly negated — equal to the reference on the values, for both pairings and rot_dim 128 / 64"""
    inputs = rl.all_values_inputs()
    q, k_new, v_new, bt, P, lens = inputs
    for il in (False, True):
        for rot in (128, 64):
            table = rl.pinned_table(rot)
            qo, kp, vp = _call(kind, inputs, 64, table, il)
            _check_q(qo, q, lens, table, il, True, (kind, il, rot))
            if kind == "f16":
                _check_k16(kp, inputs, 64, table, il, True, (kind, il, rot))
                assert torch.equal(al.bits(vp), al.bits(rl.place(al.sentinel_pools(P, 4, 64, 128, False)[1], v_new, bt, lens)))
            else:
                exact = rl.rope_ref(k_new, rl.positions(lens, 512), table, il)[0].half()
                ks, _ = al.kind_scales(kind, 4)
                want = rl.place(al.sentinel_pools(P, 4, 64, 128, True)[0], quantize(exact, ks), bt, lens)
                assert torch.equal(rl.zero_codes(kp), rl.zero_codes(want)), (kind, il, rot)


# ---- 2. composition identities, on bits

def _rotated_rows(k16_pool, bt, lens, Nq, ps):
    """[B,Hkv,Nq,D]: the rows of the Nq newest tokens gathered back from an fp16 pool (zeros where nothing was written)"""
    P, Hkv, _, D = k16_pool.shape
    pos = rl.positions(lens, Nq, bt.shape[1] * ps)
    out = torch.zeros(len(lens), Hkv, Nq, D, dtype=torch.half)
    for b in range(len(lens)):
        for i in range(Nq):
            p = int(pos[b, i])
            if p >= 0 and 0 <= int(bt[b, p // ps]) < P:
                out[b, :, i] = k16_pool[int(bt[b, p // ps]), :, p % ps]
    return out


@pytest.mark.parametrize("il", (False, True), ids=("neox", "interleaved"))
@pytest.mark.parametrize("D", rl.DS)
def test_composition_identities(D, il):
    """(a) the V pool is kv_append_paged's / kv_append_paged_kv8's; (b) the fp8 K pool is kv_append_paged_kv8 fed with the rotated K gathered back
    from the fp16 entry's pool; (c) Qout and the pools are the same bits from the dense layout, the packed layout at the minimal stride and a
    padded one; (d) in place equals out of place; (e) Q heads given their K / V head's K row come out as the K row the pool holds"""
    capi = _capi()
    for ps, Nq, rot in ((16, 100, D // 2), (256, 5, D), (64, 16, 16)):
        inputs = rl.grid_inputs(D, ps, Nq, 8)
        q, k_new, v_new, bt, P, lens = inputs
        table = rl.random_table(rot)
        q16, k16, v16 = _call("f16", inputs, ps, table, il)
        q8, k8, v8 = _call("kv8", inputs, ps, table, il)
        ks, vs = al.kind_scales("kv8")
        # (a), (b)
        dev = [x.cuda() for x in (k_new, v_new, bt, torch.tensor(lens, dtype=torch.int32), ks, vs)]
        pa = [x.cuda() for x in al.sentinel_pools(P, rl.HKV, ps, D, False)]
        capi.kv_append_paged(dev[0], dev[1], pa[0], pa[1], dev[2], dev[3])
        krot = _rotated_rows(k16, bt, lens, Nq, ps)
        p8 = [x.cuda() for x in al.sentinel_pools(P, rl.HKV, ps, D, True)]
        capi.kv_append_paged_kv8(krot.cuda(), dev[1], p8[0], p8[1], dev[2], dev[3], dev[4], dev[5])
        torch.cuda.synchronize()
        assert torch.equal(al.bits(v16), al.bits(pa[1].cpu())) and torch.equal(v8, p8[1].cpu()), (ps, Nq, rot)
        assert torch.equal(k8, p8[0].cpu()), (ps, Nq, rot)
        # (c), (d)
        for kind, ref in (("f16", (q16, k16, v16)), ("kv8", (q8, k8, v8))):
            for layout, inplace in (("packed", False), ("padded", False), ("dense", True)):
                got = _call(kind, inputs, ps, table, il, layout, inplace)
                assert all(torch.equal(al.bits(a), al.bits(b)) for a, b in zip(got, ref)), (kind, layout, inplace, ps, Nq, rot)
        # (e): Q and K take the same position and the same arithmetic
        G = 8 // rl.HKV
        same = (k_new.repeat_interleave(G, dim=1), k_new, v_new, bt, P, lens)
        qs, kpool, _ = _call("f16", same, ps, table, il)
        rows = _rotated_rows(kpool, bt, lens, Nq, ps).repeat_interleave(G, dim=1)
        assert torch.equal(al.bits(qs), al.bits(rows)), (ps, Nq, rot)


# ---- 3. edges

@pytest.mark.parametrize("kind", ("f16", "kv8"))
@pytest.mark.parametrize("ps", rl.PAGE_SIZES)
@pytest.mark.parametrize("D", rl.DS)
def test_length_edges_and_bad_page_ids(D, ps, kind):
    """append_lib.EDGE_LENS in one launch (zeros in Qout and no pool write where the position is negative); then page ids -1, num_pages and
    2^31 - 1 on a needed page of each batch entry and foreign ids elsewhere: K and V dropped, Qout still rotated"""
    rot = D // 2
    for inputs in (rl.edge_inputs(D, ps), rl.table_inputs(D, ps)):
        q, k_new, v_new, bt, P, lens = inputs[:6]
        for il in (False, True):
            table = rl.random_table(rot)
            what = (D, ps, kind, il, len(lens))
            qo, kp, vp = _call(kind, inputs, ps, table, il)
            _check_q(qo, q, lens, table, il, False, what)
            _check_v(vp, inputs, ps, kind, what)
            if kind == "f16":
                _check_k16(kp, inputs, ps, table, il, False, what)
            else:
                _, kp16, _ = _call("f16", inputs, ps, table, il)
                written = _check_k16(kp16, inputs, ps, table, il, False, what)
                assert torch.equal(kp, _codes_of(kp16, written, kind, P, rl.HKV, ps, D)), what
    assert any(L <= 0 for L in al.EDGE_LENS) and all(rl.table_inputs(D, ps)[6])


@pytest.mark.parametrize("il", (False, True), ids=("neox", "interleaved"))
@pytest.mark.parametrize("D", rl.DS)
def test_a_table_shorter_than_the_cache_is_clamped_to_its_last_row(D, il):
    """max_pos = 100 with positions up to 776: the rows behind the table read row 99.  The table ends where its allocation ends (_table_dev)
    and starts at an odd float: nothing is read outside it, and nothing assumes more than a float's alignment"""
    for rot in (D, 16):
        inputs = rl.grid_inputs(D, 64, 100, 8)
        q, k_new, v_new, bt, P, lens = inputs
        short = rl.random_table(rot)[:rl.SHORT_MAX_POS].contiguous()
        qo, kp, vp = _call("f16", inputs, 64, short, il)
        _check_q(qo, q, lens, short, il, False, (D, il, rot))
        _check_k16(kp, inputs, 64, short, il, False, (D, il, rot))
        assert int(rl.positions(lens, 100).max()) == 776


@pytest.mark.parametrize("kind", ("f16", "kv8"))
@pytest.mark.parametrize("il", (False, True), ids=("neox", "interleaved"))
def test_a_nan_in_one_pair_changes_nothing_outside_that_pair(il, kind):
    D, ps, Nq, rot = 128, 64, 16, 64
    q, k_new, v_new, bt, P, lens = rl.grid_inputs(D, ps, Nq, 8)
    table = rl.random_table(rot)
    clean = _call(kind, (q, k_new, v_new, bt, P, lens), ps, table, il)
    j = 5
    pair = (2 * j, 2 * j + 1) if il else (j, j + rot // 2)
    qn, kn = q.clone(), k_new.clone()
    qn[1, 3, 7, pair[0]] = float("nan")
    kn[2, 1, 9, pair[1]] = float("inf")
    got = _call(kind, (qn, kn, v_new, bt, P, lens), ps, table, il)
    qmask = torch.ones_like(q, dtype=torch.bool)
    qmask[1, 3, 7, list(pair)] = False
    assert torch.equal(al.bits(got[0])[qmask], al.bits(clean[0])[qmask])
    p = int(rl.positions(lens, Nq)[2, 9])
    kmask = torch.ones_like(got[1], dtype=torch.bool)
    kmask[int(bt[2, p // ps]), 1, p % ps, list(pair)] = False
    assert torch.equal(al.bits(got[1])[kmask], al.bits(clean[1])[kmask]) and torch.equal(al.bits(got[2]), al.bits(clean[2]))


# ---- 4. a whole step, captured once and replayed

@pytest.mark.parametrize("kv8", (False, True), ids=("f16", "kv8"))
def test_a_whole_step_is_captured_once_and_replayed(kv8):
    """[kv_len += 1 on the device, rope_append_paged_qkv from a packed qkv, attn_decode_paged] captured as one chain, replayed three times after
    qkv, kv_len and the table were rewritten in place: Qout, the pools and O equal the eager calls on the same state each time"""
    capi = _capi()
    D, ps, Bn, H, Hkv, rot = 128, 16, al.B, 8, al.HKV, 64
    mp = al.NCAP // ps
    gen = torch.Generator().manual_seed(31)
    table, P = al.make_table(Bn, mp, seed=78, spare=40)
    ks, vs = al.kind_scales("kv8" if kv8 else "f16")
    dks, dvs = (ks.cuda(), vs.cuda()) if kv8 else (None, None)
    lens = [500, 129, 64]
    host = al.sentinel_pools(P, Hkv, ps, D, kv8)
    kn, vn = al.new_rows(Bn, Hkv, 500, D, seed=5)
    al.append_model(host[0], host[1], kn, vn, table, lens, ks, vs)          # a filled cache to attend over
    g_pools, e_pools = [x.cuda() for x in host], [x.cuda() for x in host]
    tg, cs = table.cuda(), rl.random_table(rot).cuda()
    g_len, e_len = (torch.tensor(lens, dtype=torch.int32, device="cuda") for _ in range(2))
    W = (H + 2 * Hkv) * D
    qkv = torch.randn(Bn, 1, W, generator=gen).half().cuda()
    g_q, e_q = (torch.full((Bn, H, 1, D), float("nan"), dtype=torch.half, device="cuda") for _ in range(2))
    g_o, e_o = torch.full_like(g_q, float("nan")), torch.full_like(g_q, float("nan"))

    def step(pools, lens_dev, out_q, out_o):
        lens_dev.add_(1)
        capi.rope_append_paged_qkv(qkv, H, Hkv, pools[0], pools[1], cs, tg, lens_dev, q_out=out_q, k_scale=dks, v_scale=dvs)
        if kv8:
            capi.attn_decode_paged_kv8(out_q, pools[0], pools[1], out_o, tg, lens_dev, dks, dvs, causal=True)
        else:
            capi.attn_decode_paged(out_q, pools[0], pools[1], out_o, tg, lens_dev, causal=True)

    capi.tune("attn_decode_split", 1)          # (what a captured call without a workspace runs anyway: the eager calls run the same kernel)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            warm = [x.clone() for x in g_pools]
            step(warm, g_len.clone(), torch.empty_like(g_q), torch.empty_like(g_o))      # warm-up on the capture stream, on state of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                step(g_pools, g_len, g_q, g_o)
        torch.cuda.synchronize()
        assert torch.isnan(g_o).all() and [int(x) for x in g_len.cpu()] == lens          # captured, not run
        for r in range(3):
            qkv.copy_(torch.randn(qkv.shape, generator=gen).half())
            if r == 1:                                                    # every page moves; the sequences jump ahead; new angles
                perm = torch.randperm(P, generator=gen)
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(P)
                for pools in (g_pools, e_pools):
                    for x in pools:
                        x.copy_(x[inv.cuda()])
                tg.copy_(perm[tg.cpu().long()].to(torch.int32))
                for x in (g_len, e_len):
                    x.copy_(torch.tensor([300, 40, 7], dtype=torch.int32))
                cs.copy_(rl.pinned_table(rot))
            g.replay()
            step(e_pools, e_len, e_q, e_o)
            torch.cuda.synchronize()
            assert torch.equal(g_len.cpu(), e_len.cpu())
            assert torch.isfinite(g_o).all() and torch.equal(al.bits(g_o), al.bits(e_o)) and torch.equal(al.bits(g_q), al.bits(e_q)), r
            assert all(torch.equal(al.bits(a), al.bits(b)) for a, b in zip(g_pools, e_pools)), r
            # ... and Qout is the reference's
            now = [int(x) for x in g_len.cpu()]
            qh = qkv.cpu()[:, :, :H * D].view(Bn, 1, H, D).transpose(1, 2)
            qe, qb = rl.q_truth(qh, now, al.NCAP, cs.cpu(), False)
            rl.check_bound(g_q.cpu(), qe, qb, ("replay", r))
    finally:
        capi.tune("attn_decode_split", 0)


# ---- 5. end to end

@pytest.mark.parametrize("kv8", (False, True), ids=("f16", "kv8"))
def test_a_prefill_in_chunks_end_to_end(kv8):
    """a 320-token prompt in chunks of 128, 128 and 64 through rope_append_paged_qkv + attn_chunk_paged(causal): Qout and the gathered K pool hold
    the bound against rope_ref; the concatenated O is the oracle's causal attention ON the Qout and the gathered K / V the GPU produced
    (tol.attn_close through check_decode, as tests/test_gpu_chunk.py uses it)"""
    capi = _capi()
    B, H, Hkv, D, ps, N, rot, mp = 2, 8, 2, 128, 16, 320, 64, 24
    q, k, v = dl.decode_inputs(B, H, Hkv, N, N, D, seed=321)
    cs_host = rl.random_table(rot, 512)
    cs = cs_host.cuda()
    perm = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(6))
    table = perm[:B * mp].view(B, mp).to(torch.int32).cuda()
    ks, vs = dl.scales(dl.K_SCALES, Hkv).cuda(), dl.scales(dl.V_SCALES, Hkv).cuda()
    kp16, vp16 = (torch.full((B * mp + 3, Hkv, ps, D), float("nan"), dtype=torch.half, device="cuda") for _ in range(2))
    kp8, vp8 = (torch.full((B * mp + 3, Hkv, ps, D), dl.NAN_BYTE, dtype=torch.uint8, device="cuda") for _ in range(2))
    outs, qouts, done = [], [], 0
    for n in (128, 128, 64):
        lens_dev = torch.full((B,), done + n, dtype=torch.int32, device="cuda")
        qkv = rl.pack_qkv(q[:, :, done:done + n], k[:, :, done:done + n], v[:, :, done:done + n]).cuda()
        qo = capi.rope_append_paged_qkv(qkv, H, Hkv, kp16, vp16, cs, table, lens_dev)
        o = torch.full_like(qo, float("nan"))
        if kv8:
            qo8 = capi.rope_append_paged_qkv(qkv, H, Hkv, kp8, vp8, cs, table, lens_dev, k_scale=ks, v_scale=vs)
            capi.attn_chunk_paged_kv8(qo8, kp8, vp8, o, table, lens_dev, ks, vs, causal=True)
            torch.cuda.synchronize()
            assert torch.equal(al.bits(qo8), al.bits(qo))
        else:
            capi.attn_chunk_paged(qo, kp16, vp16, o, table, lens_dev, causal=True)
        outs.append(o)
        qouts.append(qo)
        done += n
    torch.cuda.synchronize()
    out, qout = torch.cat(outs, dim=2).cpu(), torch.cat(qouts, dim=2).cpu()
    assert torch.isfinite(out).all()
    pos = torch.arange(N)[None, :].expand(B, N)
    kc16 = gather(kp16.cpu(), table.cpu())[:, :, :N].contiguous()
    vc16 = gather(vp16.cpu(), table.cpu())[:, :, :N].contiguous()
    for got, x in ((qout, q), (kc16, k)):
        exact, e = rl.rope_ref(x, pos, cs_host, False)
        rl.check_bound(got, exact, e, "prefill in chunks")
    assert torch.equal(al.bits(vc16), al.bits(v))
    if kv8:      # the cache as the pool holds it: the codes of the fp16 entry's rows
        k8, v8 = gather(kp8.cpu(), table.cpu())[:, :, :N], gather(vp8.cpu(), table.cpu())[:, :, :N]
        assert torch.equal(k8, quantize(kc16, ks.cpu())) and torch.equal(v8, quantize(v, vs.cpu()))
        kc, vc = dl.dequant(k8, ks.cpu()).contiguous(), dl.dequant(v8, vs.cpu()).contiguous()
    else:
        kc, vc = kc16, vc16
    truth, nks = decode_truth(_oracle(), qout, kc, vc, (N,) * B, True)
    worst = check_decode(out.float().numpy(), truth, nks, "chunked prefill behind rope_append_paged_qkv")
    print(f"[rope] prefill in chunks kv8={kv8}: worst |err| / bound {worst:.3f} (oracle on the GPU's Qout and cache)")
