"""GPU tests of the append-to-cache kernels (lc_kv_append_paged_f16, lc_kv_append_paged_kv8) on the MI355X.  Every pool is prefilled with a
sentinel and allocated with guard elements either side; every comparison is torch.equal on the raw bits of the WHOLE buffer — guards, pool, every
page nobody names — against tests/append_lib.append_ref run on the CPU from the same sentinel, so a stray write anywhere fails.  The inputs are
those tests/test_abi_cpu_kv_append.py proves to have teeth."""
import pytest
import torch

from tests import append_lib as al
from tests.decode_lib import _capi, decode_inputs, quantize

pytestmark = pytest.mark.gpu


def _guarded(pool):
    """(buf, view): the CPU pool on the GPU between GUARD sentinel elements either side; view is the pool inside buf"""
    sent = al.SENT8 if pool.dtype == torch.uint8 else al.SENT16
    raw = al.bits(pool).flatten()
    guard = torch.full((al.GUARD,), sent, dtype=raw.dtype)
    buf = torch.cat([guard, raw, guard]).cuda()
    view = buf[al.GUARD:al.GUARD + raw.numel()].view(pool.shape)
    return buf, (view.view(torch.half) if pool.dtype == torch.half else view)


def _expected(pool):
    sent = al.SENT8 if pool.dtype == torch.uint8 else al.SENT16
    raw = al.bits(pool).flatten()
    guard = torch.full((al.GUARD,), sent, dtype=raw.dtype)
    return torch.cat([guard, raw, guard])


def _append(capi, kv8, k_new, v_new, kp, vp, table, lens, ks=None, vs=None):
    if kv8:
        capi.kv_append_paged_kv8(k_new, v_new, kp, vp, table, lens, ks, vs)
    else:
        capi.kv_append_paged(k_new, v_new, kp, vp, table, lens)


def _run_case(capi, inputs, kv8, ks=None, vs=None, what=""):
    """one call from sentinel pools against append_ref: the whole buffers, and the inputs unchanged"""
    k_new, v_new, table, P, lens = inputs[:5]
    Hkv, D, ps = k_new.shape[1], k_new.shape[3], al.NCAP // table.shape[1]
    ref = al.append_model(*al.sentinel_pools(P, Hkv, ps, D, kv8), k_new, v_new, table, lens, ks, vs)
    bufs, views = zip(*(_guarded(p) for p in al.sentinel_pools(P, Hkv, ps, D, kv8)))
    dev = [x.cuda() for x in (k_new, v_new, table, torch.tensor(lens, dtype=torch.int32))] + [None if s is None else s.cuda() for s in (ks, vs)]
    _append(capi, kv8, dev[0], dev[1], views[0], views[1], dev[2], dev[3], dev[4], dev[5])
    torch.cuda.synchronize()
    for name, buf, want in (("K", bufs[0], ref[0]), ("V", bufs[1], ref[1])):
        got, exp = buf.cpu(), _expected(want)
        assert torch.equal(got, exp), (what, name, f"{int((got != exp).sum())} of {exp.numel()} elements differ, the first at "
                                       f"{int((got != exp).nonzero()[0]) - al.GUARD} (pool element; negative / beyond the pool: a guard)")
    return ref, dev


@pytest.mark.parametrize("kind", al.KINDS)
@pytest.mark.parametrize("ps", al.PAGE_SIZES)
@pytest.mark.parametrize("D", al.DS)
def test_grid_against_the_reference(D, ps, kind):
    """D x page size x Nq in {1, 4, 5, 16, 100} x {fp16, fp8 under per-head scales, fp8 with NULL scales}, lens (777, 129, 65): Nq = 100 drops
    the 35 left-padded tokens of the 65-token entry and crosses page seams of every size"""
    capi = _capi()
    ks, vs = al.kind_scales(kind)
    for Nq in al.GRID_NQ:
        assert capi.kv_append_paged_kernel_name(al.B, al.HKV, Nq, ps, al.NCAP // ps, D, kv8=kind != "f16") == \
            (f"kv_append_paged_kernel<{D}>" if kind == "f16" else f"kv_append_paged_kv8_kernel<{D}>")
        _run_case(capi, al.grid_inputs(D, ps, Nq), kind != "f16", ks, vs, (D, ps, Nq, kind))


@pytest.mark.parametrize("kind", ("f16", "kv8"))
@pytest.mark.parametrize("ps", al.PAGE_SIZES)
@pytest.mark.parametrize("D", al.DS)
def test_length_edges_in_one_launch(D, ps, kind):
    """twelve batch entries, Nq = 20: kv_len 0, negative, 1, Nq - 1, Nq, Nq + 1, a page boundary and its neighbours, Ncap - 1, Ncap and beyond
    (clamped) — left-padding drops, and calls whose tokens straddle a page seam onto a page far away in the pool"""
    capi = _capi()
    ks, vs = al.kind_scales(kind)
    inputs = al.edge_inputs(D, ps)
    table = inputs[2]
    assert al.EDGE_LENS[8] == 513 and abs(int(table[8, 512 // ps]) - int(table[8, 512 // ps - 1])) > 1      # the entry that straddles 512: pages far apart
    _run_case(capi, inputs, kind != "f16", ks, vs, (D, ps, kind))


@pytest.mark.parametrize("kind", ("f16", "kv8"))
@pytest.mark.parametrize("ps", al.PAGE_SIZES)
@pytest.mark.parametrize("D", al.DS)
def test_bad_page_ids_drop_their_tokens_and_foreign_entries_are_never_read(D, ps, kind):
    """page ids -1, num_pages and 2^31 - 1 on a needed page of each batch entry: exactly those tokens are missing (nothing is clamped onto
    another page); every table entry that holds none of the Nq positions names a page another sequence writes: those pages hold that
    sequence's rows and nothing else"""
    capi = _capi()
    ks, vs = al.kind_scales(kind)
    inputs = al.table_inputs(D, ps)
    ref, _ = _run_case(capi, inputs, kind != "f16", ks, vs, (D, ps, kind))
    sent = al.SENT8 if kind != "f16" else al.SENT16
    held = int((al.bits(ref[0]) != sent).any(dim=-1).any(dim=1).sum())                   # (page, row) pairs that hold a token
    assert held == sum(min(L, 100) - len(inputs[5][b]) for b, L in enumerate(al.LENS)) and all(inputs[5])


def test_every_fp16_value_is_quantised_as_the_reference_does():
    """B = 1, Hkv = 4, D = 128 and Nq = 512, so that each head's 65 536 elements are ALL fp16 bit patterns (shuffled; K and V shuffled
    differently) under that head's scale — {1, 2^-3, 4, 0.3} for K, {3, 4, 1.7 / 448, 2^-5} for V.  Every byte whose input is not a NaN
    equals decode_lib.quantize; where the input is a NaN (2 046 of 65 536 per head) the code is a NaN code.  No other element is left out."""
    capi = _capi()
    k_new, v_new, table, P, lens, ks, vs = al.all_values_inputs()
    Hkv, Nq, D, ps = 4, 512, 128, 64
    bufs, views = zip(*(_guarded(p) for p in al.sentinel_pools(P, Hkv, ps, D, True)))
    dev = [x.cuda() for x in (k_new, v_new, table, torch.tensor(lens, dtype=torch.int32), ks, vs)]
    capi.kv_append_paged_kv8(dev[0], dev[1], views[0], views[1], dev[2], dev[3], dev[4], dev[5])
    torch.cuda.synchronize()
    for name, x, s, buf in (("K", k_new, ks, bufs[0]), ("V", v_new, vs, bufs[1])):
        nan = torch.isnan(x.float())
        assert [int(n) for n in nan.sum(dim=(0, 2, 3))] == [2046] * Hkv
        want = quantize(x, s)
        want[nan] = 0x7F
        pool = al.sentinel_pools(P, Hkv, ps, D, True)[0]
        nanpool = torch.zeros_like(pool, dtype=torch.bool)
        for i in range(Nq):                                              # the reference placement, on the codes and on the NaN mask alike
            pid = int(table[0, i // ps])
            pool[pid, :, i % ps] = want[0, :, i]
            nanpool[pid, :, i % ps] = nan[0, :, i]
        got = buf.cpu()
        inner = got[al.GUARD:-al.GUARD].view(pool.shape)
        assert ((inner[nanpool] & 0x7F) == 0x7F).all(), name             # a NaN code, either sign
        fixed = torch.where(nanpool, pool, inner)
        assert torch.equal(fixed, pool), (name, int((fixed != pool).sum()))
        assert (got[:al.GUARD] == al.SENT8).all() and (got[-al.GUARD:] == al.SENT8).all()


@pytest.mark.parametrize("ps", (16, 256))
@pytest.mark.parametrize("D", al.DS)
def test_prefill_three_steps_and_decode_round_trip(D, ps):
    """from sentinel pools: ONE left-padded prefill call (prompts of lens - 3, Nq = 774), then three steps of kv_len += 1 on the device, append
    Nq = 1, decode.  Each step's pools, and each step's O (fp16 and fp8 pools, causal and not), are torch.equal to the same decode call on a
    pool laid out on the host"""
    capi = _capi()
    Bn, H, Hkv, mp = al.B, 8, al.HKV, al.NCAP // ps
    q_all, k, v = decode_inputs(Bn, H, Hkv, 3, al.NCAP, D, seed=97 + D + ps)
    table, P = al.make_table(Bn, mp, seed=ps + D)
    short = [x - 3 for x in al.LENS]
    nq0 = max(short)
    for kv8 in (False, True):
        ks, vs = al.kind_scales("kv8" if kv8 else "f16")
        host = al.sentinel_pools(P, Hkv, ps, D, kv8)
        bufs, views = zip(*(_guarded(p) for p in al.sentinel_pools(P, Hkv, ps, D, kv8)))
        dks, dvs = (ks.cuda(), vs.cuda()) if kv8 else (None, None)
        tg = table.cuda()
        dl = torch.tensor(short, dtype=torch.int32, device="cuda")
        kn, vn = al.left_padded(k, short, nq0), al.left_padded(v, short, nq0)
        al.append_model(host[0], host[1], kn, vn, table, short, ks, vs)
        _append(capi, kv8, kn.cuda(), vn.cuda(), views[0], views[1], tg, dl, dks, dvs)
        torch.cuda.synchronize()
        assert torch.equal(bufs[0].cpu(), _expected(host[0])) and torch.equal(bufs[1].cpu(), _expected(host[1]))
        for step in range(3):
            now = [x + step + 1 for x in short]
            dl += 1                                                       # on the device
            kn = torch.stack([k[b, :, now[b] - 1:now[b]] for b in range(Bn)])
            vn = torch.stack([v[b, :, now[b] - 1:now[b]] for b in range(Bn)])
            al.append_model(host[0], host[1], kn, vn, table, now, ks, vs)
            _append(capi, kv8, kn.cuda(), vn.cuda(), views[0], views[1], tg, dl, dks, dvs)
            torch.cuda.synchronize()
            assert torch.equal(bufs[0].cpu(), _expected(host[0])) and torch.equal(bufs[1].cpu(), _expected(host[1])), (kv8, step)
            q = q_all[:, :, step:step + 1].contiguous().cuda()
            hk, hv = host[0].cuda(), host[1].cuda()
            hl = torch.tensor(now, dtype=torch.int32, device="cuda")
            for causal in (False, True):
                o, oh = torch.full_like(q, float("nan")), torch.full_like(q, float("nan"))
                if kv8:
                    capi.attn_decode_paged_kv8(q, views[0], views[1], o, tg, dl, dks, dvs, causal=causal)
                    capi.attn_decode_paged_kv8(q, hk, hv, oh, tg, hl, dks, dvs, causal=causal)
                else:
                    capi.attn_decode_paged(q, views[0], views[1], o, tg, dl, causal=causal)
                    capi.attn_decode_paged(q, hk, hv, oh, tg, hl, causal=causal)
                torch.cuda.synchronize()
                assert torch.isfinite(o).all() and torch.equal(al.bits(o), al.bits(oh)), (kv8, step, causal)
        assert [int(x) for x in dl.cpu()] == list(al.LENS)


@pytest.mark.parametrize("kv8", (False, True), ids=("f16", "kv8"))
def test_a_whole_step_is_captured_once_and_replayed(kv8):
    """[append, decode] captured as one linear chain on one stream, replayed three times after Knew / Vnew, kv_len, the table and both scale
    arrays were rewritten in place: pools and O equal the eager calls on the same state each time"""
    capi = _capi()
    D, ps, Bn, H, Hkv = 128, 16, al.B, 8, al.HKV
    mp = al.NCAP // ps
    gen = torch.Generator().manual_seed(23)
    table, P = al.make_table(Bn, mp, seed=77, spare=40)
    ks, vs = al.kind_scales("kv8" if kv8 else "f16")
    dks, dvs = (ks.cuda(), vs.cuda()) if kv8 else (None, None)
    lens = [500, 129, 64]
    # a filled cache to attend over: one prefill call, mirrored on the host
    host = al.sentinel_pools(P, Hkv, ps, D, kv8)
    kn, vn = al.new_rows(Bn, Hkv, 500, D, seed=5)
    al.append_model(host[0], host[1], kn, vn, table, lens, ks, vs)
    g_pools = [x.cuda() for x in host]                                    # the pools the graph writes ...
    e_pools = [x.cuda() for x in host]                                    # ... and those of the eager calls
    tg, dl = table.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    k1, v1 = (x.cuda() for x in al.new_rows(Bn, Hkv, 1, D, seed=6))
    q = torch.randn(Bn, H, 1, D, generator=gen).half().cuda()
    o = torch.full_like(q, float("nan"))

    def step(pools, out):
        _append(capi, kv8, k1, v1, pools[0], pools[1], tg, dl, dks, dvs)
        if kv8:
            capi.attn_decode_paged_kv8(q, pools[0], pools[1], out, tg, dl, dks, dvs, causal=True)
        else:
            capi.attn_decode_paged(q, pools[0], pools[1], out, tg, dl, causal=True)

    capi.tune("attn_decode_split", 1)          # (what a captured call without a workspace runs anyway: the eager calls run the same kernel)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            warm = [x.clone() for x in g_pools]
            step(warm, torch.empty_like(q))                              # warm-up on the capture stream, on pools of its own
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                step(g_pools, o)
        torch.cuda.synchronize()
        assert torch.isnan(o).all() and all(torch.equal(al.bits(a), al.bits(b)) for a, b in zip(g_pools, e_pools))      # captured, not run
        for r in range(3):
            dl += 1
            k1.copy_(torch.randn(k1.shape, generator=gen).half())
            v1.copy_(torch.randn(v1.shape, generator=gen).half())
            q.copy_(torch.randn(q.shape, generator=gen).half())
            if r == 1:                                                    # every page moves: the table and BOTH pools are rewritten in place
                perm = torch.randperm(P, generator=gen)
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(P)
                for pools in (g_pools, e_pools):
                    for x in pools:
                        x.copy_(x[inv.cuda()])                           # new page perm[j] holds what page j held
                tg.copy_(perm[tg.cpu().long()].to(torch.int32))
            if kv8 and r == 2:                                            # new scales for the token of this step
                dks.copy_(torch.tensor([2.0 ** -1, 2.0 ** -5]))
                dvs.copy_(torch.tensor([2.0 ** -4, 2.0 ** 1]))
            g.replay()
            eager = torch.full_like(q, float("nan"))
            step(e_pools, eager)
            torch.cuda.synchronize()
            assert torch.isfinite(o).all() and torch.equal(al.bits(o), al.bits(eager)), r
            assert all(torch.equal(al.bits(a), al.bits(b)) for a, b in zip(g_pools, e_pools)), r
            # ... and the token of this replay sits where the host reference puts it
            now = [x + r + 1 for x in lens]
            hk, hv = al.sentinel_pools(P, Hkv, ps, D, kv8)
            cks, cvs = (dks.cpu(), dvs.cpu()) if kv8 else (None, None)
            al.append_model(hk, hv, k1.cpu(), v1.cpu(), tg.cpu(), now, cks, cvs)
            for got, want in zip(g_pools, (hk, hv)):
                sent = al.SENT8 if kv8 else al.SENT16
                mask = al.bits(want) != sent
                assert mask.any() and torch.equal(al.bits(got.cpu())[mask], al.bits(want)[mask]), r
    finally:
        capi.tune("attn_decode_split", 0)


@pytest.mark.parametrize("kv8", (False, True), ids=("f16", "kv8"))
def test_the_inputs_are_unchanged(kv8):
    capi = _capi()
    ks, vs = al.kind_scales("kv8" if kv8 else "f16")
    inputs = al.grid_inputs(128, 64, 100)
    _, dev = _run_case(capi, inputs, kv8, ks, vs)
    k_new, v_new, table, _, lens = inputs
    for got, want in zip(dev, (k_new, v_new, table, torch.tensor(lens, dtype=torch.int32), ks, vs)):
        if want is not None:
            assert torch.equal(al.bits(got.cpu()) if got.dtype == torch.half else got.cpu(), al.bits(want) if want.dtype == torch.half else want)
