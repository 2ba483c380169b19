"""fec_rs_reconstruct_some_batch (klauspost Reconstruct / ReconstructSome, in place) on the device, by
the guarded-arena method of test_gpu_layouts.py: every batch lives in one canary-filled arena with
guards at both ends, shard slots hold canary from L on, erased slots 0x5A over their whole first
round_up(L, 16) bytes, and after each call the WHOLE arena is compared with a numpy model: the image
before the call with only the wanted missing shards of recoverable blocks changed (bytes [0, L) = the
oracle's, [L, round_up(L, 16)) = 0).

The expected bytes of a full reconstruct are the oracle's ReconstructData followed by its Encode on
the result; of those the model takes only the shards the call was asked to rebuild.
"""
import numpy as np
import pytest

from arena import CANARY, canary_image, check_arena, codec, place, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

ERASED = 0x5A
B = 67          # waves straddle blocks, the last workgroup is ragged
TOO_FEW = -4

LENS = [1, 33, 1202]
# (10,22) and (1,31): blocks that miss 22 and 31 shards take a second row pass of 16
CODES = [(2, 1), (3, 2), (8, 4), (16, 8), (20, 10), (10, 22), (1, 31), (31, 1), (32, 0)]
LAYOUTS = ["interleaved_slack", "split_parity_first", "shard_major"]


def low_mask(n):
    return (1 << n) - 1


def make_masks(rng, k, m, B=B):
    """Present masks of B blocks cycling through the kinds the code can have: 0 intact, 1 parity-only
    loss, 2 one data shard, 3 mixed data and parity loss up to m, 4 exactly k present and all of them
    parity (m >= k), 5 k - 1 present."""
    n = k + m
    kinds = [0, 5] + ([1, 2] if m >= 1 else []) + ([3] if m >= 2 else []) + ([4] if m >= k else [])
    kind = np.array((sorted(kinds) * (B // len(kinds) + 1))[:B])
    rng.shuffle(kind)
    masks = np.empty(B, dtype=np.uint32)
    for b in range(B):
        kd = kind[b]
        if kd == 0:
            lost = []
        elif kd == 1:
            lost = list(k + rng.choice(m, size=int(rng.integers(1, m + 1)), replace=False))
        elif kd == 2:
            lost = [int(rng.integers(0, k))]
        elif kd == 3:
            e_d = int(rng.integers(1, min(k, m - 1) + 1))
            e_p = int(rng.integers(1, m - e_d + 1))
            if b % 2:
                e_p = m - e_d                      # every other one loses as many as the code bears
            lost = list(rng.choice(k, size=e_d, replace=False)) + list(k + rng.choice(m, size=e_p, replace=False))
        elif kd == 4:
            keep = set((k + rng.choice(m, size=k, replace=False)).tolist())
            lost = [i for i in range(n) if i not in keep]
        else:
            keep = set(rng.choice(n, size=k - 1, replace=False).tolist())
            lost = [i for i in range(n) if i not in keep]
        masks[b] = low_mask(n) & ~sum(1 << int(i) for i in lost)
    return masks, kind


def bits(words, n):
    return ((np.asarray(words, dtype=np.uint32)[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & 1) == 1


_cases = {}


def make_case(oracle, k, m, L, masks, seed):
    """Host side of one batch of len(masks) blocks: shards [B, n, L] with the oracle's parity, the
    damaged batch, and the oracle's full reconstruct of it (ReconstructData, then Encode on the result)."""
    n, B = k + m, len(masks)
    rng = np.random.default_rng(seed)
    sh = np.zeros((B, n, L), dtype=np.uint8)
    sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    if m:
        oracle.rs_encode(k, m, sh)
    lost = ~bits(masks, n)
    ok = (~lost).sum(axis=1) >= k
    dmg = sh.copy()
    dmg[lost] = ERASED
    full = dmg.copy()
    st_ref = oracle.rs_reconstruct(k, m, full, masks)
    if m:
        oracle.rs_encode(k, m, full)
    if m:   # (without parity the oracle has nothing to report: no block with a loss can be rebuilt)
        assert np.array_equal(st_ref == 0, ok | ~lost[:, :k].any(axis=1))
    assert np.array_equal(full[ok], sh[ok])     # each shard has one right value
    c = dict(sh=sh, masks=np.asarray(masks, dtype=np.uint32), lost=lost, ok=ok, dmg=dmg, full=full)
    for a in c.values():
        a.setflags(write=False)
    return c


def rs_case(oracle, k, m, L, B=B):
    key = (k, m, L, B)
    if key not in _cases:
        rng = np.random.default_rng(100000 * k + 1000 * m + L)
        masks, kind = make_masks(rng, k, m, B)
        c = make_case(oracle, k, m, L, masks, 7 * L + k)
        nmiss = c["lost"].sum(axis=1)
        assert (~c["ok"]).any() and (nmiss[c["ok"]] == 0).any()
        if m:
            assert nmiss[c["ok"]].max() == m, "some block loses as many shards as the code bears"
        if m >= k:
            assert (c["ok"] & c["lost"][:, :k].all(axis=1)).any(), "all data lost, rebuilt from parity alone"
        _cases[key] = c
    return _cases[key]


def fill_damaged(img, data, par, c, k, L):
    """The encoded batch with its erased shards overwritten (bytes [0, round_up(L, 16)))."""
    R = rup16(L)
    data.view(img, 0, L)[...] = c["dmg"][:, :k]
    par.view(img, 0, L)[...] = c["dmg"][:, k:]
    for reg, lost in ((data, c["lost"][:, :k]), (par, c["lost"][:, k:])):
        reg.view(img, L, R)[lost] = ERASED


def run_some(codec, fec, torch, c, layout, k, m, L, want=None, dev_masks=None, dev_want=None, mutate=None):
    """One call on one layout; checks the whole arena, the statuses and the sticky code against the
    model. want: uint32 [B] or None (every shard); dev_masks / dev_want: what the device is given
    instead (stray bits). The batch is as many blocks as the case c holds; its slots are reached through
    strided views of the arena. Returns (arena before the call, arena after, statuses, rebuilt [B, n])."""
    n, R, B = k + m, rup16(L), len(c["masks"])
    data, par = place(layout, k, m, L, B)
    img = canary_image([data, par])
    fill_damaged(img, data, par, c, k, L)
    if mutate:
        mutate(img, data, par)
    wanted = np.ones((B, n), dtype=bool) if want is None else bits(want, n)
    rset = c["lost"] & wanted
    few = rset.any(axis=1) & ~c["ok"]
    rebuilt = rset & ~few[:, None]
    model = img.copy()
    for reg, rb, ref in ((data, rebuilt[:, :k], c["full"][:, :k]), (par, rebuilt[:, k:], c["full"][:, k:])):
        reg.view(model, 0, L)[rb] = ref[rb]
        reg.view(model, L, R)[rb] = 0
    dev = torch.from_numpy(img).cuda()
    p = dev.data_ptr()
    assert p % 16 == 0
    dm = torch.from_numpy(np.asarray(c["masks"] if dev_masks is None else dev_masks, dtype=np.uint32)
                          .view(np.int32).copy()).cuda()
    dw = dev_want if dev_want is not None else want
    dwt = None if dw is None else torch.from_numpy(np.asarray(dw, dtype=np.uint32).view(np.int32).copy()).cuda()
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    rc = fec.lib.fec_rs_reconstruct_some_batch(codec.handle, k, m, L, B, p + data.off, data.bs,
                                               (p + par.off) if m else None, par.bs, data.ss, dm.data_ptr(),
                                               None if dwt is None else dwt.data_ptr(), st.data_ptr(),
                                               fec.FEC_DEVICE)
    assert rc == fec.FEC_OK
    rc = codec.lib_sync_rc()
    assert rc == (fec.FEC_ERR_TOO_FEW_SHARDS if few.any() else fec.FEC_OK)
    assert codec.lib_sync_rc() == fec.FEC_OK   # reported once, then cleared
    got_st = st.cpu().numpy()
    assert np.array_equal(got_st, np.where(few, TOO_FEW, 0))
    got = dev.cpu().numpy()
    check_arena(got, model, "reconstruct-some")
    return img, got, got_st, rebuilt, (data, par)


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_full_reconstruct_against_the_oracle(codec, oracle, torch, fec, layout, k, m, L):
    """want = NULL: every missing shard of every recoverable block, data and parity; too-few blocks
    untouched with status -4 and the sticky code reported once."""
    c = rs_case(oracle, k, m, L)
    _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, layout, k, m, L)
    assert (st == TOO_FEW).any()
    if m:
        assert rebuilt[:, k:].any() and rebuilt[:, :k].any()
    if (k, m) in ((10, 22), (1, 31)):
        assert rebuilt.sum(axis=1).max() == m > 16   # the second row pass


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
def test_data_only_want_mask_equals_reconstruct_data(codec, oracle, torch, fec, k, m, L):
    """A want mask of low_mask(k): byte for byte and status for status what fec_rs_reconstruct_batch
    gives on a copy of the arena."""
    c = rs_case(oracle, k, m, L)
    want = np.full(B, low_mask(k), dtype=np.uint32)
    img, got, st, _, (data, par) = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=want)
    dev = torch.from_numpy(img).cuda()
    p = dev.data_ptr()
    dm = torch.from_numpy(c["masks"].view(np.int32).copy()).cuda()
    st2 = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    assert fec.lib.fec_rs_reconstruct_batch(codec.handle, k, m, L, B, p + data.off, data.bs,
                                            (p + par.off) if m else None, par.bs, data.ss, dm.data_ptr(),
                                            st2.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
    codec.lib_sync_rc()
    assert np.array_equal(st2.cpu().numpy(), st)
    check_arena(got, dev.cpu().numpy(), "reconstruct-some against fec_rs_reconstruct_batch")


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", [km for km in CODES if km[1]])
def test_all_parity_lost_equals_encode(codec, oracle, torch, fec, k, m, L):
    """Data intact, every parity shard erased, want = NULL: byte for byte what fec_rs_encode_batch
    writes into a copy of the arena."""
    c = make_case(oracle, k, m, L, np.full(B, low_mask(k), dtype=np.uint32), 3 * L + m)
    img, got, st, rebuilt, (data, par) = run_some(codec, fec, torch, c, "split_parity_first", k, m, L)
    assert rebuilt[:, k:].all() and not rebuilt[:, :k].any()
    dev = torch.from_numpy(img).cuda()
    p = dev.data_ptr()
    assert fec.lib.fec_rs_encode_batch(codec.handle, k, m, L, B, p + data.off, data.bs, p + par.off, par.bs,
                                       data.ss, fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(got, dev.cpu().numpy(), "reconstruct-some against fec_rs_encode_batch")


def two_of_four_case(oracle, k, m, L, B=B):
    """(case, want masks): every block misses two data and two parity shards, and its want mask names
    one of each and some present shards."""
    rng = np.random.default_rng(17 * k + L)
    masks = np.empty(B, dtype=np.uint32)
    want = np.empty(B, dtype=np.uint32)
    for b in range(B):
        d = rng.choice(k, size=2, replace=False)
        q = k + rng.choice(m, size=2, replace=False)
        masks[b] = low_mask(k + m) & ~sum(1 << int(i) for i in list(d) + list(q))
        want[b] = (1 << int(d[1])) | (1 << int(q[0])) | (int(rng.integers(0, 1 << 32)) & int(masks[b]))
    return make_case(oracle, k, m, L, masks, 5 * L + k), want


@pytest.mark.parametrize("L", [33, 1202])
@pytest.mark.parametrize("k,m", [(8, 4), (16, 8), (20, 10), (10, 22)])
def test_want_mask_names_two_of_four_missing(codec, oracle, torch, fec, k, m, L):
    """Every block misses two data and two parity shards; the want mask names one of each (and some
    present shards): the other two missing slots keep 0x5A."""
    c, want = two_of_four_case(oracle, k, m, L)
    _, got, st, rebuilt, _ = run_some(codec, fec, torch, c, "shard_major", k, m, L, want=want)
    assert (rebuilt.sum(axis=1) == 2).all() and (rebuilt[:, :k].sum(axis=1) == 1).all() and (st == 0).all()


@pytest.mark.parametrize("k,m", [(3, 2), (8, 4), (10, 22), (32, 0)])
def test_want_mask_of_present_shards_touches_nothing(codec, oracle, torch, fec, k, m):
    """A want mask naming only present shards: the block is untouched with status 0, even with k - 1
    present, and nothing is reported."""
    L = 33
    c = rs_case(oracle, k, m, L)
    assert (~c["ok"]).any()
    img, got, st, rebuilt, _ = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=c["masks"])
    assert not rebuilt.any() and (st == 0).all() and np.array_equal(img, got)


@pytest.mark.parametrize("k,m", [(3, 2), (8, 4), (10, 22)])
def test_inputs_are_the_first_k_present(codec, oracle, torch, fec, k, m):
    """One data shard lost, all parity present: the inputs are the other data shards and parity 0.
    Garbage in the present parity shards after those does not reach the output."""
    L = 33
    rng = np.random.default_rng(k)
    masks = np.array([low_mask(k + m) & ~(1 << int(rng.integers(0, k))) for _ in range(B)], dtype=np.uint32)
    c = make_case(oracle, k, m, L, masks, 9 * k)

    def garbage(img, data, par):
        idx = par.index(0, L)[:, 1:]
        img[idx] = rng.integers(0, 256, idx.shape, dtype=np.uint8)

    _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, mutate=garbage)
    assert (rebuilt.sum(axis=1) == 1).all() and (st == 0).all()


@pytest.mark.parametrize("k,m", [(8, 4), (16, 8), (1, 31)])
def test_stray_mask_bits_are_ignored(codec, oracle, torch, fec, k, m):
    """Bits at and above k + m, set in both masks, change nothing ((1,31): no such bits exist, the
    want mask of all ones is the NULL one)."""
    L = 33
    n = k + m
    c = rs_case(oracle, k, m, L)
    stray = np.uint32((0xFFFFFFFF << n) & 0xFFFFFFFF)
    run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, dev_masks=c["masks"] | stray,
             dev_want=np.full(B, 0xFFFFFFFF, dtype=np.uint32))
    # and with a data-only want mask
    want = np.full(B, low_mask(k), dtype=np.uint32)
    run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=want, dev_masks=c["masks"] | stray,
             dev_want=want | stray)


def test_codec_methods(codec, torch, fec):
    """Codec.rs_reconstruct_some / _split on [B, n, S] tensors, shard_len below the slot size."""
    k, m, S, L, nb = 6, 3, 48, 41, 9
    sh = torch.randint(0, 256, (nb, k + m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode(k, m, sh, shard_len=L)
    ref = sh.clone()
    masks = torch.full((nb,), low_mask(k + m), dtype=torch.int32, device="cuda")
    masks[3] = low_mask(k + m) & ~((1 << 1) | (1 << (k + 2)))
    masks[5] = low_mask(k + m) & ~(1 << k)
    sh[3, 1] = ERASED
    sh[3, k + 2] = ERASED
    sh[5, k] = ERASED
    ref[3, 1, L:] = ERASED      # the slot's bytes past round_up(L, 16) are not written
    ref[3, 1, L:rup16(L)] = 0
    ref[3, k + 2, L:] = ERASED
    ref[3, k + 2, L:rup16(L)] = 0
    ref[5, k, L:] = ERASED
    ref[5, k, L:rup16(L)] = 0
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    work = sh.clone()
    assert codec.rs_reconstruct_some(k, m, work, masks, status=st, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert torch.equal(work, ref) and (st == 0).all()
    data, par = sh[:, :k].contiguous(), sh[:, k:].contiguous()
    want = torch.full((nb,), 1 << (k + 2), dtype=torch.int32, device="cuda")
    assert codec.rs_reconstruct_some_split(k, m, data, par, masks, want=want, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert torch.equal(par[3, 2], ref[3, k + 2]) and torch.equal(data, sh[:, :k]) and torch.equal(par[5], sh[5, k:])
    with pytest.raises(AssertionError):
        codec.rs_reconstruct_some(k, m, sh.cpu(), masks, shard_len=L)


def test_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx are those of fec_rs_reconstruct_batch, the want mask's alignment after
    them; a 2^32 shard stride is refused (the rebuild takes 32-bit shard strides)."""
    h, D = codec.handle, fec.FEC_DEVICE
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    w = torch.zeros((8,), dtype=torch.int32, device="cuda")   # masks: nothing present, want: nothing
    st = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    p, mk, s = buf.data_ptr(), w.data_ptr(), st.data_ptr()
    F = fec.lib.fec_rs_reconstruct_some_batch
    assert F(h, 2, 1, 16, 0, None, 0, None, 0, 16, None, None, None, D) == fec.FEC_OK
    assert F(h, 2, 1, 16, 2, None, 48, p + 32, 48, 16, mk, None, s, D) == fec.FEC_ERR_INVALID_ARG
    assert F(h, 2, 1, 16, 2, p, 48, None, 48, 16, mk, None, s, D) == fec.FEC_ERR_INVALID_ARG
    assert F(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, None, None, s, D) == fec.FEC_ERR_INVALID_ARG
    assert F(h, 2, 1, 16, 2, p + 8, 48, p + 32, 48, 16, mk, None, s, D) == fec.FEC_ERR_ALIGNMENT
    assert F(h, 2, 1, 17, 2, p, 48, p + 32, 48, 16, mk, None, s, D) == fec.FEC_ERR_INVALID_ARG
    assert F(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, mk + 2, None, s, D) == fec.FEC_ERR_ALIGNMENT
    assert F(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, mk, None, s + 2, D) == fec.FEC_ERR_ALIGNMENT
    assert F(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, mk, mk + 18, s, D) == fec.FEC_ERR_ALIGNMENT
    assert F(h, 2, 1, 16, 2, p, 16, p + 2048, 16, 1 << 32, mk, None, s, D) == fec.FEC_ERR_INVALID_ARG
    assert codec.lib_sync_rc() == fec.FEC_OK
    # nothing present, nothing wanted: untouched, status 0 (block_status is optional)
    assert F(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, mk, mk + 16, s, D) == fec.FEC_OK
    assert F(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, mk, mk + 16, None, D) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and st.cpu().tolist() == [0, 0, 99, 99]
