"""Every device entry point of include/fec_hip.h at byte offsets past 2 and 4 GiB: block strides,
region distances (parity above and below the data) and shard strides that do not fit 32 bits, in the
layouts of far_cases.py, which cannot fault (a 32-bit mistake reads or writes canary inside the
arena). The batch lives in the sparse arena of far_arena.py: the host models the shard slots' windows,
compares them byte for byte after the call, and the device then checks every other byte of the
11.85 GiB for the canary. Expected bytes come from the oracle; routes among the kernels are forced with
the tune fixture.

The conventions are those of test_gpu_layouts.py: input slots hold canary from L on, erased slots
0x5A over [0, round_up(L, 16)), outputs change only in [0, L) plus zeros up to round_up(L, 16); each of
the five blocks is of another kind (intact, too few shards, one data shard lost, parity-only loss,
several lost, in this order: far_cases.far_lost places the kinds so that blocks 2 and 4, past 2^31
and 2^32 where the block stride is large, are rebuilt) and has contents of its own.
"""
import numpy as np
import pytest

import far_cases as fc
from arena import CANARY, MUL, STALE, codec, folded_parity, recover_statuses, rup16, torch  # noqa: F401
from far_arena import far  # noqa: F401
from test_gpu_layouts import ERASED, expect_sync

pytestmark = pytest.mark.gpu

B = fc.B


def params(*calls):
    return pytest.mark.parametrize("c", fc.cases_of(*calls), ids=fc.case_id)


def words(t, a):
    return t.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def stale(t, n, value=99):
    return t.full((n,), value, dtype=t.int32, device="cuda")


def layout_args(far, lay, L):
    """shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride."""
    d, p = lay.regions["data"], lay.regions["parity"]
    assert d.ss == p.ss
    return L, B, far.addr(d), d.bs, far.addr(p), p.bs, d.ss


def fill_inputs(pre, k, shards, lens, lost=None):
    """Bytes [0, lens[b]) of block b's data and parity slots from shards[b] ([n, >= lens[b]]); the lost
    shards' slots hold ERASED over their first round_up(lens[b], 16) bytes."""
    for b in range(B):
        Lb = int(lens[b])
        pre["data"][b, :, :Lb] = shards[b][:k, :Lb]
        pre["parity"][b, :, :Lb] = shards[b][k:, :Lb]
        if lost is not None:
            pre["data"][b, lost[b, :k], :rup16(Lb)] = ERASED
            pre["parity"][b, lost[b, k:], :rup16(Lb)] = ERASED


def copy_of(wins):
    return {name: w.copy() for name, w in wins.items()}


def put_output(win, b, j, row, Lb):
    """An output shard: bytes [0, Lb) and zeros up to round_up(Lb, 16)."""
    win[b, j, :Lb] = row[:Lb]
    win[b, j, Lb:rup16(Lb)] = 0


def model_encode(pre, k, shards, lens):
    model = copy_of(pre)
    for b in range(B):
        for i in range(model["parity"].shape[1]):
            put_output(model["parity"], b, i, shards[b][k + i], int(lens[b]))
    return model


def model_decode(fec, pre, k, lens, lost, rec, few, slots):
    """(windows after an in-place reconstruct (slots == 0) or a recover into `slots` out slots of the
    damaged batch, statuses): rec[b] is the oracle's reconstruct of block b."""
    model = copy_of(pre)
    e_d = lost[:, :k].sum(axis=1)
    if slots == 0:
        st = np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS, 0)
        rebuilt = ~few
    else:
        st = recover_statuses(fec, e_d, few, slots)
        rebuilt = st > 0
    for b in np.flatnonzero(rebuilt):
        for r, i in enumerate(np.flatnonzero(lost[b, :k])):
            if slots:
                put_output(model["out"], b, r, rec[b][i], int(lens[b]))
            else:
                put_output(model["data"], b, i, rec[b][i], int(lens[b]))
    return model, st


def run_decode(far, codec, fec, t, lay, k, L, lens, dmg, lost, rec, few, slots, masks, call, what):
    """One reconstruct or recover of any form: call(layout arguments, masks, out arguments, status)
    returns the entry point's return code."""
    pre = far.blank(lay)
    fill_inputs(pre, k, dmg, lens, lost)
    model, st_want = model_decode(fec, pre, k, lens, lost, rec, few, slots)
    far.write(lay, pre)
    dm, st = words(t, masks), stale(t, B)
    o = lay.regions.get("out")
    out_args = (far.addr(o), o.bs, slots) if slots else ()
    assert call(layout_args(far, lay, L), dm.data_ptr(), out_args, st.data_ptr()) == fec.FEC_OK
    expect_sync(codec, fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    far.check(lay, model, what)
    return st_want


# ---------------------------------------------------------------- the arena's own check

def test_the_arena_check_finds_a_stray_byte_and_a_wrong_window(far, torch):
    """One byte off the canary anywhere in the arena (first byte, last byte, past 2^32, in a slot's
    slack past its window) is reported at its offset; a window byte that differs from the model is
    reported at its arena offset; the arena is clean again afterwards."""
    lay = fc.far_layout("far_shards", 8, 4, fc.L_LONG, "out", 4)
    pre = far.blank(lay)
    pre["data"][...] = 7
    far.write(lay, pre)
    far.check(lay, pre, "nothing changed")
    d = lay.regions["data"]
    for off in (0, far.size - 1, (1 << 32) + 5, d.at(4, 7) + d.win, d.at(0, 4) - 1):
        far.dev[off] = 0
        assert far.first_dirty() == off
        far.write(lay, pre)
        with pytest.raises(AssertionError, match="outside every window was written, first at arena offset %d " % off):
            far.check(lay, pre, "stray")
        assert far.first_dirty() is None
    model = copy_of(pre)
    model["parity"][4, 3, 1201] ^= 1
    far.write(lay, pre)
    with pytest.raises(AssertionError, match="first at arena offset %d " % (lay.regions["parity"].at(4, 3) + 1201)):
        far.check(lay, model, "window")
    assert far.first_dirty() is None


# ---------------------------------------------------------------- encode

@params("fec_rs_encode_batch")
def test_encode(far, codec, oracle, torch, fec, tune, c):
    tune(**fc.ROUTES[c.route])
    lay = fc.layout_of(c)
    sh = plain_case(oracle, c.k, c.m, c.L)
    lens = [c.L] * B
    pre = far.blank(lay)
    fill_inputs(pre, c.k, sh, lens)
    pre["parity"][...] = CANARY
    model = model_encode(pre, c.k, sh, lens)
    far.write(lay, pre)
    assert fec.lib.fec_rs_encode_batch(codec.handle, c.k, c.m, *layout_args(far, lay, c.L), fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    far.check(lay, model, fc.case_id(c))


_plain = {}


def plain_case(oracle, k, m, L):
    """Encoded shards [B, n, L], every block with contents of its own."""
    if (k, m, L) not in _plain:
        sh = np.zeros((B, k + m, L), dtype=np.uint8)
        sh[:, :k] = np.random.default_rng(31 * k + m + L).integers(0, 256, (B, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        sh.setflags(write=False)
        _plain[(k, m, L)] = sh
    return _plain[(k, m, L)]


# ---------------------------------------------------------------- reconstruct, recover

@params("fec_rs_reconstruct_batch", "fec_rs_recover_batch")
def test_reconstruct_and_recover(far, codec, oracle, torch, fec, tune, c):
    tune(**fc.ROUTES[c.route])
    k, m, L = c.k, c.m, c.L
    cs = fc.far_rs_case(oracle, k, m, L, fc.mode_of(c))
    if c.route == "routed":      # which route word the routed kernel runs on
        assert (cs["e_d"][~cs["few"]] >= 2).any() == (c.opt != "single")
    slots = fc.slots_of(c)
    h = codec.handle

    def call(la, masks, out_args, status):
        if slots:
            return fec.lib.fec_rs_recover_batch(h, k, m, *la, masks, *out_args, status, fec.FEC_DEVICE)
        return fec.lib.fec_rs_reconstruct_batch(h, k, m, *la, masks, status, fec.FEC_DEVICE)

    st = run_decode(far, codec, fec, torch, fc.layout_of(c), k, L, [L] * B, cs["dmg"], cs["lost"], cs["rec"],
                    cs["few"], slots, cs["masks"], call, fc.case_id(c))
    assert (st == fec.FEC_ERR_TOO_FEW_SHARDS).sum() == 1


@params("fec_xor_encode_batch", "fec_xor_reconstruct_batch")
def test_xor(far, codec, oracle, torch, fec, c):
    k, L = c.k, c.L
    cs = fc.far_xor_case(oracle, k, L)
    lay = fc.layout_of(c)
    lens = [L] * B
    if c.step == "encode":
        pre = far.blank(lay)
        fill_inputs(pre, k, cs["sh"], lens)
        pre["parity"][...] = CANARY
        model = model_encode(pre, k, cs["sh"], lens)
        far.write(lay, pre)
        assert fec.lib.fec_xor_encode_batch(codec.handle, k, *layout_args(far, lay, L), fec.FEC_DEVICE) == fec.FEC_OK
        assert codec.lib_sync_rc() == fec.FEC_OK
        far.check(lay, model, fc.case_id(c))
        return

    def call(la, masks, out_args, status):
        return fec.lib.fec_xor_reconstruct_batch(codec.handle, k, *la, masks, status, fec.FEC_DEVICE)

    # a block that lost only its parity has nothing to rebuild; one that lost two shards fails
    run_decode(far, codec, fec, torch, lay, k, L, lens, cs["dmg"], cs["lost"], cs["rec"], cs["fail"], 0, cs["masks"],
               call, fc.case_id(c))


# ---------------------------------------------------------------- wide

_wide = {}


def wide_case(oracle, MUL, k, m, L):
    """Encoded shards, the lost shards of fc.far_lost, masks of fc.WIDE_W words, and the rebuilt
    batch: the oracle's for k + m <= 32, else the inverse-matrix reference of test_gpu_wide.py."""
    if (k, m, L) not in _wide:
        from test_gpu_wide import ref_reconstruct
        n, R = k + m, rup16(L)
        sh = np.zeros((B, n, R), dtype=np.uint8)
        sh[:, :, :L] = plain_case(oracle, k, m, L)
        pres = ~fc.far_lost(k, m)
        dmg = sh.copy()
        dmg[~pres] = ERASED
        rec = dmg.copy()
        masks = np.zeros((B, fc.WIDE_W), dtype=np.uint32)
        packed = np.packbits(pres, axis=1, bitorder="little")
        masks.view(np.uint8)[:, :packed.shape[1]] = packed
        if n <= 32:
            st = oracle.rs_reconstruct(k, m, rec, masks[:, 0].copy(), length=L)
        else:
            st = ref_reconstruct(oracle, MUL, k, m, rec, pres, L)
        few = st != 0
        assert few.tolist() == [False, True, False, False, False]
        assert np.array_equal(rec[~few][:, :k, :L], sh[~few][:, :k, :L])
        _wide[(k, m, L)] = dict(dmg=dmg, lost=~pres, rec=rec, few=few, masks=masks)
    return _wide[(k, m, L)]


@params("fec_rs_reconstruct_wide_batch", "fec_rs_recover_wide_batch")
def test_wide(far, codec, oracle, torch, fec, MUL, c):
    k, m, L = c.k, c.m, c.L
    cs = wide_case(oracle, MUL, k, m, L)
    slots = fc.slots_of(c)
    h = codec.handle

    def call(la, masks, out_args, status):
        if slots:
            return fec.lib.fec_rs_recover_wide_batch(h, k, m, *la, masks, fc.WIDE_W, *out_args, status, fec.FEC_DEVICE)
        return fec.lib.fec_rs_reconstruct_wide_batch(h, k, m, *la, masks, fc.WIDE_W, status, fec.FEC_DEVICE)

    run_decode(far, codec, fec, torch, fc.layout_of(c), k, L, [L] * B, cs["dmg"], cs["lost"], cs["rec"], cs["few"],
               slots, cs["masks"], call, fc.case_id(c))


# ---------------------------------------------------------------- ragged

@params("fec_rs_encode_ragged_batch", "fec_rs_reconstruct_ragged_batch", "fec_rs_recover_ragged_batch")
def test_ragged(far, codec, oracle, torch, fec, c):
    """Each block at its own length against the oracle at that length; bytes past a block's length in
    its slots (canary) stay unchanged."""
    k, m, L = c.k, c.m, c.L
    lens = list(fc.RAGGED_LENS)
    assert max(lens) == L and len(lens) == B
    cs = fc.far_rs_case(oracle, k, m, L)
    lay = fc.layout_of(c)
    dl = words(torch, lens)
    h = codec.handle
    if c.step == "encode":
        enc = []
        for b in range(B):
            one = cs["sh"][b:b + 1, :, :lens[b]].copy()
            one[:, k:] = 0
            enc.append(oracle.rs_encode(k, m, one)[0])
        pre = far.blank(lay)
        fill_inputs(pre, k, enc, lens)
        pre["parity"][...] = CANARY
        model = model_encode(pre, k, enc, lens)
        far.write(lay, pre)
        st = stale(torch, B)
        assert fec.lib.fec_rs_encode_ragged_batch(h, k, m, *layout_args(far, lay, L), dl.data_ptr(), st.data_ptr(),
                                                  fec.FEC_DEVICE) == fec.FEC_OK
        assert codec.lib_sync_rc() == fec.FEC_OK
        assert (st.cpu().numpy() == 0).all()
        far.check(lay, model, fc.case_id(c))
        return
    rec = []
    for b in range(B):
        one = cs["dmg"][b:b + 1, :, :lens[b]].copy()
        st = oracle.rs_reconstruct(k, m, one, cs["masks"][b:b + 1])
        assert (st[0] != 0) == cs["few"][b]
        rec.append(one[0])
    slots = fc.slots_of(c)

    def call(la, masks, out_args, status):
        if slots:
            return fec.lib.fec_rs_recover_ragged_batch(h, k, m, *la, masks, dl.data_ptr(), *out_args, status,
                                                       fec.FEC_DEVICE)
        return fec.lib.fec_rs_reconstruct_ragged_batch(h, k, m, *la, masks, dl.data_ptr(), status, fec.FEC_DEVICE)

    run_decode(far, codec, fec, torch, lay, k, L, lens, cs["dmg"], cs["lost"], rec, cs["few"], slots, cs["masks"],
               call, fc.case_id(c))


# ---------------------------------------------------------------- verify, locate: nothing is written

def corrupt(sh, hits, first=False):
    """sh with one byte flipped in the last chunk of shard j of block b (first: and one in its first
    chunk) for every (b, j) of hits."""
    out = sh.copy()
    L = sh.shape[2]
    for b, j in hits:
        out[b, j, L - 1] ^= 0x40
        if first:
            out[b, j, 3] ^= 0x01
    return out


def given(far, lay, k, shards, L, lost=None):
    """The windows of a batch whose shards are only read, written to the arena."""
    pre = far.blank(lay)
    fill_inputs(pre, k, shards, [L] * B, lost)
    far.write(lay, pre)
    return pre


@params("fec_rs_verify_batch")
def test_verify(far, codec, oracle, torch, fec, c):
    """Blocks 2 and 4 have a byte flipped in the last chunk of the farthest data and the farthest
    parity shard."""
    k, m, L = c.k, c.m, c.L
    lay = fc.layout_of(c)
    bad = corrupt(plain_case(oracle, k, m, L), [(2, k - 1), (4, k + m - 1)])
    pre = given(far, lay, k, bad, L)
    st, cnt = stale(torch, B, STALE), stale(torch, 1, STALE)
    assert fec.lib.fec_rs_verify_batch(codec.handle, k, m, *layout_args(far, lay, L), st.data_ptr(), cnt.data_ptr(),
                                       fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert st.cpu().numpy().tolist() == [1, 1, 0, 1, 0] and cnt.cpu().numpy().tolist() == [2]
    far.check(lay, pre, fc.case_id(c))


def heals(oracle, k, m, shards, present_out, want):
    """The returned present masks, given to the oracle's reconstruct, give the original data back."""
    rec = shards.copy()
    n = k + m
    lost = ((present_out[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & 1) == 0
    rec[lost] = ERASED
    st = oracle.rs_reconstruct(k, m, rec, present_out)
    assert (st == 0).all() and np.array_equal(rec[:, :k], want[:, :k])


@params("fec_rs_locate_batch", "fec_rs_locate_multi_batch", "fec_rs_locate_partial_batch")
def test_locate(far, codec, oracle, torch, fec, c):
    """The corrupt shards are the farthest data shard and the farthest parity shard, in blocks 2 and 4:
    one each for locate (and for locate-partial, whose blocks 1, 2 and 4 also miss a shard), both in
    both blocks for locate-multi."""
    k, m, L = c.k, c.m, c.L
    n, full = k + m, (1 << (k + m)) - 1
    lay = fc.layout_of(c)
    sh = plain_case(oracle, k, m, L)
    far_d, far_p = k - 1, n - 1
    res, pout = stale(torch, B, STALE), stale(torch, B, STALE)
    la = layout_args(far, lay, L)
    h = codec.handle
    if c.step == "locate":
        bad = corrupt(sh, [(2, far_d), (4, far_p)], first=True)
        pre = given(far, lay, k, bad, L)
        cnt = stale(torch, 2, STALE)
        rc = fec.lib.fec_rs_locate_batch(h, k, m, *la, res.data_ptr(), pout.data_ptr(), 1, cnt.data_ptr(),
                                         fec.FEC_DEVICE)
        want = [fec.FEC_LOCATE_CLEAN, fec.FEC_LOCATE_CLEAN, far_d, fec.FEC_LOCATE_CLEAN, far_p]
        masks = [full, full, full & ~(1 << far_d), full, full & ~(1 << far_p)]
        counts = [2, 0]
    elif c.step == "locate_multi":
        bad = corrupt(sh, [(2, far_d), (2, far_p), (4, far_d), (4, far_p)], first=True)
        pre = given(far, lay, k, bad, L)
        cnt = stale(torch, 2, STALE)
        rc = fec.lib.fec_rs_locate_multi_batch(h, k, m, *la, fec.FEC_LOCATE_MAX_BAD, res.data_ptr(), pout.data_ptr(),
                                               1, cnt.data_ptr(), fec.FEC_DEVICE)
        both = full & ~(1 << far_d) & ~(1 << far_p)
        want, masks, counts = [0, 0, 2, 0, 2], [full, full, both, full, both], [2, 0]
    else:
        bad = corrupt(sh, [(2, far_d), (4, far_p)], first=True)
        lost = fc.lost_of(c)
        present = fc.masks_of(lost)
        pre = given(far, lay, k, bad, L, lost)
        cnt = stale(torch, 3, STALE)
        dm = words(torch, present)
        rc = fec.lib.fec_rs_locate_partial_batch(h, k, m, *la, dm.data_ptr(), 1, fec.FEC_LOCATE_MAX_BAD,
                                                 res.data_ptr(), pout.data_ptr(), cnt.data_ptr(), fec.FEC_DEVICE)
        want = [0, 0, 1, 0, 1]
        masks = [int(present[0]), int(present[1]), int(present[2]) & ~(1 << far_d), int(present[3]),
                 int(present[4]) & ~(1 << far_p)]
        counts = [2, 0, 0]
    assert rc == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert res.cpu().numpy().tolist() == want
    got_masks = pout.cpu().numpy().view(np.uint32)
    assert got_masks.tolist() == masks
    assert cnt.cpu().numpy().tolist() == counts
    heals(oracle, k, m, bad, got_masks, sh)
    far.check(lay, pre, fc.case_id(c))


# ---------------------------------------------------------------- reconstruct-some, update, encode-idx

@params("fec_rs_reconstruct_some_batch")
def test_reconstruct_some(far, codec, oracle, torch, fec, c):
    """Every missing shard wanted, data and parity: the oracle's reconstruct followed by its encode."""
    from test_gpu_some import make_case
    k, m, L = c.k, c.m, c.L
    masks = fc.masks_of(fc.lost_of(c))
    cs = make_case(oracle, k, m, L, masks, 99)
    lay = fc.layout_of(c)
    lost, few = cs["lost"], cs["lost"].any(axis=1) & ~cs["ok"]
    assert few.tolist() == [False, True, False, False, False] and lost[4, :k].any() and lost[4, k:].any()
    pre = far.blank(lay)
    fill_inputs(pre, k, cs["dmg"], [L] * B, lost)
    model = copy_of(pre)
    for b in np.flatnonzero(~few):
        for i in np.flatnonzero(lost[b]):
            name, j = ("data", i) if i < k else ("parity", i - k)
            put_output(model[name], b, j, cs["full"][b, i], L)
    far.write(lay, pre)
    dm, st = words(torch, masks), stale(torch, B)
    assert fec.lib.fec_rs_reconstruct_some_batch(codec.handle, k, m, *layout_args(far, lay, L), dm.data_ptr(), None,
                                                 st.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
    st_want = np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS, 0)
    expect_sync(codec, fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    far.check(lay, model, fc.case_id(c))


@params("fec_rs_update_batch")
def test_update(far, codec, oracle, torch, fec, c):
    """old is a fourth base, placed like a recover's out. The parity starts as the oracle's encode of
    the old data; after the call it is the oracle's encode of the merged data."""
    k, m, L = c.k, c.m, c.L
    lay = fc.layout_of(c)
    old_sh = plain_case(oracle, k, m, L)
    new = np.random.default_rng(4).integers(0, 256, (B, k, L), dtype=np.uint8)
    cols = fc.column_sets(k)
    merged = np.zeros((B, k + m, L), dtype=np.uint8)
    merged[:, :k] = np.where(cols[:, :, None], new, old_sh[:, :k])
    oracle.rs_encode(k, m, merged)
    assert np.array_equal(folded_parity(oracle, k, m, old_sh[:, :k] ^ new, cols, old_sh[:, k:]), merged[:, k:])
    pre = far.blank(lay)
    pre["old"][:, :, :L] = old_sh[:, :k]
    pre["data"][:, :, :L] = new
    pre["parity"][:, :, :L] = old_sh[:, k:]
    model = copy_of(pre)
    for b in np.flatnonzero(cols.any(axis=1)):
        for i in range(m):
            put_output(model["parity"], b, i, merged[b, k + i], L)
    far.write(lay, pre)
    mk = words(torch, fec.wide_masks(cols))
    d, p, o = lay.regions["data"], lay.regions["parity"], lay.regions["old"]
    assert fec.lib.fec_rs_update_batch(codec.handle, k, m, L, B, far.addr(o), o.bs, far.addr(d), d.bs, far.addr(p),
                                       p.bs, d.ss, mk.data_ptr(), 1, fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    far.check(lay, model, fc.case_id(c))


@params("fec_rs_encode_idx_batch")
def test_encode_idx(far, codec, oracle, torch, fec, c):
    """One mask names two columns per block, the farthest among them; the zeroed parity becomes the
    oracle's parity of the block with its other columns zero."""
    k, m, L = c.k, c.m, c.L
    lay = fc.layout_of(c)
    sh = plain_case(oracle, k, m, L)
    cols = fc.idx_columns(k)
    zero = np.zeros((B, m, L), dtype=np.uint8)
    want = folded_parity(oracle, k, m, sh[:, :k], cols, zero)
    pre = far.blank(lay)
    pre["data"][:, :, :L] = sh[:, :k]
    pre["parity"][:, :, :rup16(L)] = 0
    model = copy_of(pre)
    model["parity"][:, :, :L] = want
    far.write(lay, pre)
    mk = words(torch, fec.wide_masks(cols))
    assert fec.lib.fec_rs_encode_idx_batch(codec.handle, k, m, *layout_args(far, lay, L), mk.data_ptr(), 1,
                                           fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    far.check(lay, model, fc.case_id(c))


# ---------------------------------------------------------------- what the header says about strides

def test_rebuild_calls_refuse_a_shard_stride_of_4gib(far, codec, torch, fec):
    """fec_hip.h: the calls that rebuild shards take shard strides below 2^32; 2^32 and 2^32 + 16 are
    refused before anything is enqueued (the return code, a clean sync, every status stale, the arena
    all canary)."""
    k, m, L = 8, 4, 1202
    h, D, INV = codec.handle, fec.FEC_DEVICE, fec.FEC_ERR_INVALID_ARG
    dm = words(torch, [(1 << (k + m)) - 2] * B)           # data shard 0 of every block to rebuild
    dl = words(torch, [L] * B)
    st = stale(torch, B)
    d, p, o = far.ptr + fc.LEAD, far.ptr + fc.LEAD + 4096, far.ptr + fc.LEAD + 8192
    lib = fec.lib
    for ss in (fc.REFUSED_STRIDE, fc.REFUSED_STRIDE + 16):
        la = (L, B, d, 1232, p, 1232, ss)
        refused = {
            "fec_rs_reconstruct_batch": lib.fec_rs_reconstruct_batch(h, k, m, *la, dm.data_ptr(), st.data_ptr(), D),
            "fec_rs_recover_batch": lib.fec_rs_recover_batch(h, k, m, *la, dm.data_ptr(), o, 1232, m, st.data_ptr(), D),
            "fec_rs_reconstruct_wide_batch": lib.fec_rs_reconstruct_wide_batch(h, k, m, *la, dm.data_ptr(), 2,
                                                                               st.data_ptr(), D),
            "fec_rs_recover_wide_batch": lib.fec_rs_recover_wide_batch(h, k, m, *la, dm.data_ptr(), 2, o, 1232, m,
                                                                       st.data_ptr(), D),
            "fec_rs_reconstruct_ragged_batch": lib.fec_rs_reconstruct_ragged_batch(h, k, m, *la, dm.data_ptr(),
                                                                                   dl.data_ptr(), st.data_ptr(), D),
            "fec_rs_recover_ragged_batch": lib.fec_rs_recover_ragged_batch(h, k, m, *la, dm.data_ptr(), dl.data_ptr(),
                                                                           o, 1232, m, st.data_ptr(), D),
            "fec_rs_reconstruct_some_batch": lib.fec_rs_reconstruct_some_batch(h, k, m, *la, dm.data_ptr(), None,
                                                                               st.data_ptr(), D),
        }
        assert set(refused) == {call for call, row in fc.TABLE.items() if row["refused"]}
        assert refused == {call: INV for call in refused}
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (st.cpu().numpy() == 99).all()
    assert far.first_dirty() is None
