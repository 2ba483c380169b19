"""Device layouts the C ABI (include/fec_hip.h) admits beyond the two compact block-major ones the
rest of the suite uses: shard slots with slack, block strides with gaps, parity below the data in
memory, and shard-major [k][B][S] regions. Every batch lives in one device arena pre-filled with a
canary, with guards at both ends; after each call the WHOLE arena is compared byte for byte with a
numpy model: the arena image before the call with only the bytes the header lets the call write
changed (bytes [0, L) of an output shard = the oracle's, [L, round_up(L, 16)) = 0). So a kernel
that computes the right shard but reads or writes one stride off, touches slack, a gap, a present
shard, an erased parity slot, a failed block or a guard, fails here.

Input shard slots hold canary bytes from L on (the header promises nothing about them), so a
kernel that lets the bytes of a partial tail chunk past L leak into its output fails too.
"""
import numpy as np
import pytest

from arena import CANARY, GUARD, Region, canary_image, check_arena, codec, place, recover_statuses, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

ERASED = 0x5A
B = 67          # waves straddle blocks, the last workgroup is ragged

LAYOUTS = ["interleaved_slack", "split_parity_first", "shard_major", "shard_major_split"]
# L = 1202: 76 chunks per shard ((16,8) and (20,10) take the compile-time-k rebuild, (8,4) in place
# the routed kernel, single-slot recovers the direct kernels); L = 33: the short-shard tile path
RS_CASES = [(2, 1, 1202), (6, 2, 1202), (8, 4, 1202), (16, 8, 1202), (20, 10, 1202),
            (3, 2, 33), (8, 4, 33), (16, 8, 33)]
STEPS = ["encode", "reconstruct", "recover_m", "recover_1"]


def make_layout(name, k, m, L, slots, B=B):
    """(arena, data region, parity region, out arena, out region) for one layout of B blocks; every
    offset and stride a multiple of 16, at least GUARD canary bytes before the first and after the
    last slot. The out region of a recover lies in an arena of its own, shard-major where the inputs
    are."""
    data, par = place(name, k, m, L, B)
    if name.startswith("shard_major"):
        out = Region(GUARD, data.bs, data.ss, slots, B)
    else:
        out = Region(GUARD, slots * data.ss + 32, data.ss, slots, B)
    return canary_image([data, par]), data, par, canary_image([out]), out


def make_masks(rng, k, m, B=B):
    """Present masks of B blocks over five kinds, every kind the code can have present: intact,
    parity-only loss, one data shard lost, 2..min(k, m) data shards lost, too few shards. The kinds
    are dealt in turn and then shuffled, so a batch of as many blocks as kinds holds one of each."""
    n = k + m
    kinds = [0, 1, 2, 4] + ([3] if min(k, m) >= 2 else [])
    kind = np.array((kinds * (B // len(kinds) + 1))[:B])
    rng.shuffle(kind)
    masks = np.empty(B, dtype=np.uint32)
    for b in range(B):
        if kind[b] == 0:
            lost = []
        elif kind[b] == 1:
            lost = list(k + rng.choice(m, size=int(rng.integers(1, m + 1)), replace=False))
        elif kind[b] == 2:
            lost = [int(rng.integers(0, k))] + list(k + rng.choice(m, size=int(rng.integers(0, m)), replace=False))
        elif kind[b] == 3:
            e = int(rng.integers(2, min(k, m) + 1))
            lost = list(rng.choice(k, size=e, replace=False)) + \
                list(k + rng.choice(m, size=int(rng.integers(0, m - e + 1)), replace=False))
        else:
            lost = list(rng.choice(n, size=m + 1, replace=False))   # more than the m parity shards: data among them
        masks[b] = ((1 << n) - 1) & ~sum(1 << int(i) for i in lost)
    return masks


def classify(masks, k, m):
    n = k + m
    lost = ((masks[:, None] >> np.arange(n)[None, :]) & 1) == 0
    e_d = lost[:, :k].sum(axis=1)
    few = (e_d > 0) & ((n - lost.sum(axis=1)) < k)
    kind = np.where(few, 4, np.where(e_d >= 2, 3, np.where(e_d == 1, 2, np.where(lost.any(axis=1), 1, 0))))
    return lost, e_d, few, kind


_cases = {}


def rs_case(oracle, k, m, L, B=B, single_only=False):
    """Host side of one (k, m, L, B) case, computed once: shards [B, n, L] with the oracle's parity,
    masks of all five kinds, and the oracle's in-place reconstruct of the damaged batch. single_only:
    the blocks of the fourth kind lose one data shard too, so no recoverable block loses two."""
    key = (k, m, L, B, single_only)
    if key not in _cases:
        n = k + m
        rng = np.random.default_rng(100000 * k + 1000 * m + L)
        sh = np.zeros((B, n, L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        masks = make_masks(rng, k, m, B)
        if single_only:
            lost, e_d, few, kind = classify(masks, k, m)
            for b in np.flatnonzero(kind == 3):   # all its lost data shards but the lowest are present again
                extra = np.flatnonzero(lost[b, :k])[1:]
                masks[b] |= np.uint32(sum(1 << int(i) for i in extra))
        lost, e_d, few, kind = classify(masks, k, m)
        want_kinds = {0, 1, 2, 4} | ({3} if min(k, m) >= 2 and not single_only else set())
        assert set(kind.tolist()) == want_kinds, "every block kind the code can have must be present"
        if 3 in want_kinds:
            assert (e_d[kind == 3] >= 2).all() and e_d[~few].max() <= min(k, m)
        dmg = sh.copy()
        dmg[lost] = ERASED
        rec = dmg.copy()
        st_ref = oracle.rs_reconstruct(k, m, rec, masks)
        # the oracle agrees with the host-side classification and gives back the original data
        assert np.array_equal(st_ref != 0, few)
        assert np.array_equal(rec[~few][:, :k], sh[~few][:, :k])
        assert np.array_equal(rec[few], dmg[few]) and np.array_equal(rec[:, k:], dmg[:, k:])
        for a in (sh, masks, lost, e_d, few, dmg, rec):
            a.setflags(write=False)
        _cases[key] = dict(sh=sh, masks=masks, lost=lost, e_d=e_d, few=few, dmg=dmg, rec=rec)
    return _cases[key]


def fill_damaged(arena, data, par, c, k, L):
    """The encoded batch with its erased shards overwritten (bytes [0, round_up(L, 16)))."""
    R = rup16(L)
    data.view(arena, 0, L)[...] = c["dmg"][:, :k]
    par.view(arena, 0, L)[...] = c["dmg"][:, k:]
    for reg, lost in ((data, c["lost"][:, :k]), (par, c["lost"][:, k:])):
        reg.view(arena, L, R)[lost] = ERASED


def expect_sync(codec, fec, st_want):
    rc = codec.lib_sync_rc()
    want = (fec.FEC_ERR_TOO_FEW_SHARDS if (st_want == fec.FEC_ERR_TOO_FEW_SHARDS).any() else
            fec.FEC_ERR_INVALID_ARG if (st_want == fec.FEC_ERR_INVALID_ARG).any() else fec.FEC_OK)
    assert rc == want
    assert codec.lib_sync_rc() == fec.FEC_OK   # reported once, then cleared


def run_rs_step(codec, fec, torch, c, layout, k, m, L, step, masks=None):
    """One call on one layout; checks the whole arena(s), the statuses and the sticky code. The batch
    is as many blocks as the case c holds. (The slots are reached through strided views of the
    arenas, not index arrays: those would take eight bytes per shard byte.)"""
    R = rup16(L)
    B = len(c["masks"])
    slots = 1 if step == "recover_1" else m
    arena, data, par, oarena, out = make_layout(layout, k, m, L, slots, B)
    masks = c["masks"] if masks is None else masks
    h = codec.handle
    if step == "encode":
        data.view(arena, 0, L)[...] = c["sh"][:, :k]
        model = arena.copy()
        par.view(model, 0, L)[...] = c["sh"][:, k:]
        par.view(model, L, R)[...] = 0
        dev = torch.from_numpy(arena).cuda()
        p = dev.data_ptr()
        assert p % 16 == 0
        rc = fec.lib.fec_rs_encode_batch(h, k, m, L, B, p + data.off, data.bs, p + par.off, par.bs, data.ss,
                                         fec.FEC_DEVICE)
        assert rc == fec.FEC_OK
        assert codec.lib_sync_rc() == fec.FEC_OK
        check_arena(dev.cpu().numpy(), model, "encode")
        return
    fill_damaged(arena, data, par, c, k, L)
    dev = torch.from_numpy(arena).cuda()
    p = dev.data_ptr()
    assert p % 16 == 0
    dm = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    model = arena.copy()
    lost_d, e_d, few = c["lost"][:, :k], c["e_d"], c["few"]
    if step == "reconstruct":
        rebuilt = lost_d & ~few[:, None]                       # erased data shards of recoverable blocks
        data.view(model, 0, L)[rebuilt] = c["rec"][:, :k][rebuilt]
        data.view(model, L, R)[rebuilt] = 0
        st_want = np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS, 0)
        rc = fec.lib.fec_rs_reconstruct_batch(h, k, m, L, B, p + data.off, data.bs, p + par.off, par.bs, data.ss,
                                              dm.data_ptr(), st.data_ptr(), fec.FEC_DEVICE)
        assert rc == fec.FEC_OK
        expect_sync(codec, fec, st_want)
        assert np.array_equal(st.cpu().numpy(), st_want)
        check_arena(dev.cpu().numpy(), model, "in-place reconstruct")
        return
    omodel = oarena.copy()
    st_want = recover_statuses(fec, e_d, few, slots)
    assert (st_want > 0).any()
    for b in np.flatnonzero(st_want > 0):
        for r, i in enumerate(np.flatnonzero(lost_d[b])):
            o = out.at(b, r)
            omodel[o:o + L] = c["rec"][b, i]
            omodel[o + L:o + R] = 0
    odev = torch.from_numpy(oarena).cuda()
    op = odev.data_ptr()
    assert op % 16 == 0
    rc = fec.lib.fec_rs_recover_batch(h, k, m, L, B, p + data.off, data.bs, p + par.off, par.bs, data.ss,
                                      dm.data_ptr(), op + out.off, out.bs, slots, st.data_ptr(), fec.FEC_DEVICE)
    assert rc == fec.FEC_OK
    expect_sync(codec, fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    check_arena(dev.cpu().numpy(), model, "recover, input arena")
    check_arena(odev.cpu().numpy(), omodel, "recover, out arena")


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("k,m,L", RS_CASES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rs_layout_writes_only_what_the_header_allows(codec, oracle, torch, fec, layout, k, m, L, step):
    run_rs_step(codec, fec, torch, rs_case(oracle, k, m, L), layout, k, m, L, step)


def xor_case(oracle, rng, k, L, B=B):
    """Host side of one XOR(k, 1) batch drawn from rng: shards [B, k + 1, L] with the oracle's parity,
    masks over four kinds (intact, parity lost, one data shard lost, two shards lost with a data shard
    among them), and the oracle's in-place reconstruct of the damaged batch."""
    n = k + 1
    sh = np.zeros((B, n, L), dtype=np.uint8)
    sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    oracle.xor_encode(k, sh)
    kind = np.array(([0, 1, 2, 3] * B)[:B])
    rng.shuffle(kind)
    masks = np.empty(B, dtype=np.uint32)
    for b in range(B):
        lost = {0: [], 1: [k], 2: [int(rng.integers(0, k))],
                3: [int(rng.integers(0, k))]}[int(kind[b])]
        if kind[b] == 3:
            lost.append(int(rng.choice([i for i in range(n) if i != lost[0]])))
        masks[b] = ((1 << n) - 1) & ~sum(1 << i for i in lost)
    lost = ((masks[:, None] >> np.arange(n)[None, :]) & 1) == 0
    dmg = sh.copy()
    dmg[lost] = ERASED
    rec = dmg.copy()
    st_ref = oracle.xor_reconstruct(k, rec, masks)
    fail = kind == 3
    assert np.array_equal(st_ref != 0, fail) and fail.any() and (kind == 2).any()
    rebuilt = lost[:, :k] & (kind == 2)[:, None]
    assert np.array_equal(rec[:, :k][rebuilt], sh[:, :k][rebuilt])
    return dict(sh=sh, masks=masks, lost=lost, dmg=dmg, rec=rec, kind=kind, fail=fail, rebuilt=rebuilt)


def run_xor(codec, fec, torch, c, layout, k, L):
    """XOR(k, 1) encode and in-place reconstruct of the case c on one layout, whole arena against the
    model, the statuses and the sticky code."""
    R, B = rup16(L), len(c["masks"])
    sh, masks, fail, rebuilt = c["sh"], c["masks"], c["fail"], c["rebuilt"]
    h = codec.handle
    arena, data, par, _, _ = make_layout(layout, k, 1, L, 1, B)
    data.view(arena, 0, L)[...] = sh[:, :k]
    model = arena.copy()
    par.view(model, 0, L)[...] = sh[:, k:]
    par.view(model, L, R)[...] = 0
    dev = torch.from_numpy(arena).cuda()
    p = dev.data_ptr()
    assert fec.lib.fec_xor_encode_batch(h, k, L, B, p + data.off, data.bs, p + par.off, par.bs, data.ss,
                                        fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(dev.cpu().numpy(), model, "xor encode")
    arena, data, par, _, _ = make_layout(layout, k, 1, L, 1, B)
    fill_damaged(arena, data, par, c, k, L)
    model = arena.copy()
    data.view(model, 0, L)[rebuilt] = c["rec"][:, :k][rebuilt]
    data.view(model, L, R)[rebuilt] = 0
    dev = torch.from_numpy(arena).cuda()
    p = dev.data_ptr()
    dm = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    assert fec.lib.fec_xor_reconstruct_batch(h, k, L, B, p + data.off, data.bs, p + par.off, par.bs, data.ss,
                                             dm.data_ptr(), st.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
    st_want = np.where(fail, fec.FEC_ERR_TOO_FEW_SHARDS, 0)
    expect_sync(codec, fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    check_arena(dev.cpu().numpy(), model, "xor reconstruct")


@pytest.mark.parametrize("L", [18, 1202])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_xor_layout_writes_only_what_the_header_allows(codec, oracle, torch, fec, layout, L):
    """XOR(3,1) encode and in-place reconstruct (L = 18: masks by per-lane loads, L = 1202: by the
    wave's scalar loads) on every layout, whole arena against the model."""
    k = 3
    rng = np.random.default_rng(31 * L + LAYOUTS.index(layout))
    run_xor(codec, fec, torch, xor_case(oracle, rng, k, L), layout, k, L)


@pytest.mark.parametrize("k,m", [(8, 4), (16, 8)])
def test_shard_stride_of_4gib_is_refused(codec, torch, fec, k, m):
    """The rebuild kernels take 32-bit shard strides: a reconstruct or recover with a shard stride
    of 2^32 is refused before anything is enqueued (no byte written, a clean sync). (The encode
    kernels take 64-bit strides and would run, so the call is not made on them.)"""
    L, nb = 1202, 4
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    dm = torch.full((nb,), (1 << (k + m)) - 1, dtype=torch.int32, device="cuda")   # nothing erased
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    p, ss = buf.data_ptr(), 1 << 32
    assert fec.lib.fec_rs_reconstruct_batch(codec.handle, k, m, L, nb, p, 16, p + 2048, 16, ss, dm.data_ptr(),
                                            st.data_ptr(), fec.FEC_DEVICE) == fec.FEC_ERR_INVALID_ARG
    for slots in (1, m):
        assert fec.lib.fec_rs_recover_batch(codec.handle, k, m, L, nb, p, 16, p + 2048, 16, ss, dm.data_ptr(),
                                            p + 1024, 16, slots, st.data_ptr(),
                                            fec.FEC_DEVICE) == fec.FEC_ERR_INVALID_ARG
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and (st.cpu().numpy() == 99).all()


@pytest.mark.parametrize("step", ["reconstruct", "recover_m", "recover_1"])
@pytest.mark.parametrize("k,m", [(8, 4), (16, 8)])
def test_stray_mask_bits_are_ignored(codec, oracle, torch, fec, k, m, step):
    """Masks with every bit >= k + m set give the statuses and bytes of the clean masks (the
    oracle gets the clean ones): the routed kernel and its classify pass on RS(8,12), sorted plans
    and the compile-time-k rebuild on RS(16,24), the direct kernels on single-slot recovers."""
    L = 1202
    c = rs_case(oracle, k, m, L)
    stray = (c["masks"] | np.uint32((0xFFFFFFFF << (k + m)) & 0xFFFFFFFF)).astype(np.uint32)
    assert (stray >> (k + m)).all() and np.array_equal(stray & np.uint32((1 << (k + m)) - 1), c["masks"])
    run_rs_step(codec, fec, torch, c, "interleaved_slack", k, m, L, step, masks=stray)
