"""fec_rs_reconstruct_some_wide_batch (include/fec_hip_some_wide.h) on the device, by the guarded-arena
method of test_gpu_some.py: every batch lives in one canary-filled arena with guards at both ends,
shard slots hold canary from L on, erased slots 0x5A over their whole first round_up(L, 16) bytes, and
after each call the WHOLE arena is compared with a numpy model: the image before the call with only
the wanted missing shards of recoverable blocks changed (bytes [0, L) = the expected, [L, round_up(L,
16)) = 0).

The expected bytes are those of some_wide_cases.py: inverse-matrix rows from the oracle applied to the
first k present shards, equal to the oracle's encode; none of them comes from the library.
"""
import numpy as np
import pytest

import some_wide_cases as sw
from arena import CANARY, canary_image, check_arena, codec, place, rup16, torch  # noqa: F401
from some_wide_cases import B, ERASED, TOO_FEW

pytestmark = pytest.mark.gpu

CODES = sw.CODES
LAYOUTS = ["interleaved_slack", "split_parity_first", "shard_major"]
SHAPES = [(k, m, L) for k, m in CODES for L in (1, 33)] + [(20, 13, 1202), (64, 16, 1202)]


def words(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def fill_damaged(img, data, par, c, k, L):
    """The encoded batch with its erased shards overwritten (bytes [0, round_up(L, 16)))."""
    R = rup16(L)
    data.view(img, 0, L)[...] = c["dmg"][:, :k]
    par.view(img, 0, L)[...] = c["dmg"][:, k:]
    for reg, lost in ((data, c["lost"][:, :k]), (par, c["lost"][:, k:])):
        reg.view(img, L, R)[lost] = ERASED


def region_args(p, data, par, m, L, nb):
    """shard_len, nblocks, data, data_block_stride, parity, parity_block_stride, shard_stride."""
    return L, nb, p + data.off, data.bs, (p + par.off) if m else None, par.bs, data.ss


def run_some(codec, fec, torch, c, layout, k, m, L, want=None, dev_masks=None, dev_want=None, mutate=None, W=None):
    """One call on one layout; checks the whole arena, the statuses and the sticky code against the
    model. want: bool [B, n] or None (every shard); dev_masks / dev_want: the uint32 [B, W] words the
    device is given instead of wide_masks() of the case (stray bits, more words). Returns (arena before
    the call, arena after, statuses, rebuilt [B, n], (data, parity, masks given))."""
    n, R, nb = k + m, rup16(L), len(c["lost"])
    data, par = place(layout, k, m, L, nb)
    img = canary_image([data, par])
    fill_damaged(img, data, par, c, k, L)
    if mutate:
        mutate(img, data, par)
    wanted = np.ones((nb, n), dtype=bool) if want is None else want
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
    masks = fec.wide_masks(~c["lost"]) if dev_masks is None else dev_masks
    if W is not None and dev_masks is None:
        masks = np.concatenate([masks, np.zeros((nb, W - masks.shape[1]), dtype=np.uint32)], axis=1)
    Wm = masks.shape[1]
    dm = words(torch, masks)
    dw = dev_want if dev_want is not None else (None if want is None else fec.wide_masks(want))
    if dw is not None and dw.shape[1] < Wm:
        dw = np.concatenate([dw, np.zeros((nb, Wm - dw.shape[1]), dtype=np.uint32)], axis=1)
    assert dw is None or dw.shape == masks.shape
    dwt = None if dw is None else words(torch, dw)
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    rc = fec.lib.fec_rs_reconstruct_some_wide_batch(codec.handle, k, m, *region_args(p, data, par, m, L, nb),
                                                    dm.data_ptr(), None if dwt is None else dwt.data_ptr(), Wm,
                                                    st.data_ptr(), fec.FEC_DEVICE)
    assert rc == fec.FEC_OK
    rc = codec.lib_sync_rc()
    assert rc == (fec.FEC_ERR_TOO_FEW_SHARDS if few.any() else fec.FEC_OK)
    assert codec.lib_sync_rc() == fec.FEC_OK   # reported once, then cleared
    got_st = st.cpu().numpy()
    assert np.array_equal(got_st, np.where(few, TOO_FEW, 0))
    got = dev.cpu().numpy()
    check_arena(got, model, "wide reconstruct-some")
    return img, got, got_st, rebuilt, (data, par, masks)


@pytest.mark.parametrize("k,m,L", SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_full_reconstruct_against_the_oracle(codec, oracle, torch, fec, layout, k, m, L):
    """want = NULL: every missing shard of every recoverable block, data and parity; too-few blocks
    untouched with status -4 and the sticky code reported once."""
    c = sw.rs_case(oracle, k, m, L)
    _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, layout, k, m, L)
    assert (st == TOO_FEW).any()
    lost_ok = c["lost"] & c["ok"][:, None]
    assert np.array_equal(rebuilt, lost_ok)
    if m:
        assert rebuilt[:, k:].any() and rebuilt[:, :k].any()
    if (k, m) in ((16, 240), (1, 255)):
        assert rebuilt.sum(axis=1).max() == m    # 15 and 16 row passes


@pytest.mark.parametrize("k,m,L", SHAPES)
def test_data_only_want_mask_equals_wide_reconstruct(codec, oracle, torch, fec, k, m, L):
    """A want mask of the low k bits: byte for byte and status for status what
    fec_rs_reconstruct_wide_batch gives on a copy of the arena."""
    c = sw.rs_case(oracle, k, m, L)
    want = np.zeros((B, k + m), dtype=bool)
    want[:, :k] = True
    img, got, st, _, (data, par, masks) = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=want)
    dev = torch.from_numpy(img).cuda()
    dm = words(torch, masks)
    st2 = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    assert fec.lib.fec_rs_reconstruct_wide_batch(codec.handle, k, m, *region_args(dev.data_ptr(), data, par, m, L, B),
                                                 dm.data_ptr(), masks.shape[1], st2.data_ptr(),
                                                 fec.FEC_DEVICE) == fec.FEC_OK
    codec.lib_sync_rc()
    assert np.array_equal(st2.cpu().numpy(), st)
    check_arena(got, dev.cpu().numpy(), "wide reconstruct-some against fec_rs_reconstruct_wide_batch")


@pytest.mark.parametrize("k,m,L", [s for s in SHAPES if s[1]])
def test_all_parity_lost_equals_encode(codec, oracle, torch, fec, k, m, L):
    """Data intact, every parity shard erased, want = NULL: byte for byte what fec_rs_encode_batch
    writes into a copy of the arena."""
    lost = np.zeros((B, k + m), dtype=bool)
    lost[:, k:] = True
    c = sw.make_case(oracle, k, m, L, lost, 3 * L + m)
    img, got, st, rebuilt, (data, par, _) = run_some(codec, fec, torch, c, "split_parity_first", k, m, L)
    assert rebuilt[:, k:].all() and not rebuilt[:, :k].any()
    dev = torch.from_numpy(img).cuda()
    assert fec.lib.fec_rs_encode_batch(codec.handle, k, m, *region_args(dev.data_ptr(), data, par, m, L, B),
                                       fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(got, dev.cpu().numpy(), "wide reconstruct-some against fec_rs_encode_batch")


@pytest.mark.parametrize("W", [2, 1])
@pytest.mark.parametrize("k,m", [(8, 4), (10, 22)])
@pytest.mark.parametrize("L", [1, 33])
def test_narrow_codes_equal_reconstruct_some(codec, oracle, torch, fec, k, m, L, W):
    """Codes of at most 32 shards: with two mask words the wide plan kernel runs, with one the call
    forwards; either way bytes and statuses are those of fec_rs_reconstruct_some_batch on a copy of the
    arena, with a want mask too."""
    c = sw.rs_case(oracle, k, m, L)
    rng = np.random.default_rng(k + L)
    for want in (None, rng.integers(0, 2, (B, k + m)).astype(bool)):
        img, got, st, _, (data, par, masks) = run_some(codec, fec, torch, c, "shard_major", k, m, L, want=want, W=W)
        assert masks.shape == (B, W)
        dev = torch.from_numpy(img).cuda()
        dm = words(torch, masks[:, 0])
        dw = None if want is None else words(torch, fec.wide_masks(want)[:, 0])
        st2 = torch.full((B,), 99, dtype=torch.int32, device="cuda")
        assert fec.lib.fec_rs_reconstruct_some_batch(codec.handle, k, m,
                                                     *region_args(dev.data_ptr(), data, par, m, L, B), dm.data_ptr(),
                                                     None if dw is None else dw.data_ptr(), st2.data_ptr(),
                                                     fec.FEC_DEVICE) == fec.FEC_OK
        codec.lib_sync_rc()
        assert np.array_equal(st2.cpu().numpy(), st)
        check_arena(got, dev.cpu().numpy(), "wide reconstruct-some against fec_rs_reconstruct_some_batch")


def two_of_four_case(oracle, k, m, L, nb=B):
    """(case, want [B, n]): every block misses two data and two parity shards, and its want mask names
    one of each and some present shards."""
    rng = np.random.default_rng(17 * k + L)
    n = k + m
    lost = np.zeros((nb, n), dtype=bool)
    want = np.zeros((nb, n), dtype=bool)
    for b in range(nb):
        d = sw.pick(rng, range(k), 2, sw.BOUNDARY if b % 2 else ())
        q = sw.pick(rng, range(k, n), 2, sw.BOUNDARY if b % 2 else ())
        lost[b, d + q] = True
        want[b] = rng.integers(0, 2, n).astype(bool) & ~lost[b]
        want[b, [d[1], q[0]]] = True
    return sw.make_case(oracle, k, m, L, lost, 5 * L + k), want


@pytest.mark.parametrize("k,m", [(20, 13), (33, 32), (64, 16), (128, 128)])
def test_want_mask_names_two_of_four_missing(codec, oracle, torch, fec, k, m):
    """Every block misses two data and two parity shards; the want mask names one of each (and some
    present shards): the other two missing slots keep 0x5A."""
    L = 33
    c, want = two_of_four_case(oracle, k, m, L)
    _, got, st, rebuilt, _ = run_some(codec, fec, torch, c, "shard_major", k, m, L, want=want)
    assert (rebuilt.sum(axis=1) == 2).all() and (rebuilt[:, :k].sum(axis=1) == 1).all() and (st == 0).all()


@pytest.mark.parametrize("k,m", [(20, 13), (64, 16), (1, 255), (40, 0)])
def test_want_mask_of_present_shards_touches_nothing(codec, oracle, torch, fec, k, m):
    """A want mask naming only present shards: the block is untouched with status 0, even with k - 1
    present, and nothing is reported."""
    L = 33
    c = sw.rs_case(oracle, k, m, L)
    assert (~c["ok"]).any()
    img, got, st, rebuilt, _ = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=~c["lost"])
    assert not rebuilt.any() and (st == 0).all() and np.array_equal(img, got)


@pytest.mark.parametrize("k,m", [(20, 13), (64, 16), (128, 128)])
def test_inputs_are_the_first_k_present(codec, oracle, torch, fec, k, m):
    """One data shard lost, all parity present: the inputs are the other data shards and parity 0.
    Garbage in the present parity shards after those does not reach the output."""
    L = 33
    rng = np.random.default_rng(k)
    lost = np.zeros((B, k + m), dtype=bool)
    lost[np.arange(B), rng.integers(0, k, B)] = True
    c = sw.make_case(oracle, k, m, L, lost, 9 * k)

    def garbage(img, data, par):
        idx = par.index(0, L)[:, 1:]
        img[idx] = rng.integers(0, 256, idx.shape, dtype=np.uint8)

    _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, mutate=garbage)
    assert (rebuilt.sum(axis=1) == 1).all() and (st == 0).all()


@pytest.mark.parametrize("k,m", [(20, 13), (33, 32), (64, 16), (16, 240)])
def test_stray_mask_bits_are_ignored(codec, oracle, torch, fec, k, m):
    """Eight mask words; every bit at and above k + m set in both masks (and drawn): nothing changes."""
    L = 33
    n = k + m
    c = sw.rs_case(oracle, k, m, L)
    rng = np.random.default_rng(n)
    m8 = np.zeros((B, 8), dtype=np.uint32)
    m8[:, :fec.mask_words(n)] = fec.wide_masks(~c["lost"])
    ones = np.zeros((B, 8), dtype=np.uint32)
    ones[:, :fec.mask_words(n)] = fec.wide_masks(np.ones((B, n), dtype=bool))
    run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, dev_masks=sw.stray(m8, n),
             dev_want=sw.stray(ones, n))
    # and with a data-only want mask, the stray bits drawn
    want = np.zeros((B, n), dtype=bool)
    want[:, :k] = True
    w8 = np.zeros((B, 8), dtype=np.uint32)
    w8[:, :fec.mask_words(n)] = fec.wide_masks(want)
    run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=want, dev_masks=sw.stray(m8, n, rng),
             dev_want=sw.stray(w8, n, rng))


def test_long_shards(codec, oracle, torch, fec):
    """RS(33,32), L = 4098, five blocks: 257 chunks per shard, two chunk tiles and a 2-byte tail."""
    k, m, L, nb = 33, 32, 4098, 5
    lost = sw.far_lost(k, m)
    c = sw.make_case(oracle, k, m, L, lost, 41)
    for layout in ("interleaved_slack", "shard_major"):
        _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, layout, k, m, L)
        assert st.tolist() == [0, TOO_FEW, 0, 0, 0] and rebuilt[4].sum() == m


def test_batch_spans_launch_slices(fec, codec, torch):
    """RS(128,128), 17-byte shards, 20000 blocks: the plan records (about 16.5 KiB each) exceed the plan
    workspace bound, so the batch runs as two slices. Each block loses one data and one parity shard; the
    want mask names the parity shard on even blocks and the data shard on odd ones, so a want pointer
    that did not advance with the slice would rebuild the wrong shards in the second one."""
    k, m, L, S, nb = 128, 128, 17, 32, 20000
    n = k + m
    g = torch.Generator(device="cuda").manual_seed(11)
    sh = torch.zeros((nb, n, S), dtype=torch.uint8, device="cuda")
    sh[:, :k, :L] = torch.randint(0, 256, (nb, k, L), dtype=torch.uint8, device="cuda", generator=g)
    codec.rs_encode(k, m, sh, shard_len=L)
    codec.sync()
    rng = np.random.default_rng(11)
    ld, lp = rng.integers(0, k, nb), k + rng.integers(0, m, nb)
    ld[:4], lp[:4] = [0, 31, 32, 127], [k, k + 31, k + 32, n - 1]
    present = np.ones((nb, n), dtype=bool)
    present[np.arange(nb), ld] = False
    present[np.arange(nb), lp] = False
    even = np.arange(nb) % 2 == 0
    wanted = np.where(even, lp, ld)
    other = np.where(even, ld, lp)
    want = rng.integers(0, 2, (nb, n)).astype(bool) & present       # some present shards named too
    want[np.arange(nb), wanted] = True
    dmg = sh.clone()
    ar = torch.arange(nb, device="cuda")
    t_w, t_o = torch.from_numpy(wanted).cuda(), torch.from_numpy(other).cuda()
    dmg[ar, t_w] = ERASED
    dmg[ar, t_o] = ERASED
    before = dmg.clone()
    dm, dw = words(torch, fec.wide_masks(present)), words(torch, fec.wide_masks(want))
    ds = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    assert codec.rs_reconstruct_some_wide(k, m, dmg, dm, want=dw, status=ds, shard_len=L) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert not ds.any().item()
    # the rebuilt slots against the originals, the unwanted ones against 0x5A, nothing else changed
    assert torch.equal(dmg[ar, t_w], sh[ar, t_w])
    assert (dmg[ar, t_o] == ERASED).all().item()
    expect = before
    expect[ar, t_w] = sh[ar, t_w]
    assert torch.equal(dmg, expect)
    # the first and the last four blocks of each parity class, exactly, on the host
    edge = np.r_[0:8, nb - 8:nb]
    got, ref = dmg[edge].cpu().numpy(), sh[edge].cpu().numpy()
    for i, b in enumerate(edge):
        model = ref[i].copy()
        model[other[b]] = ERASED
        assert np.array_equal(got[i], model), b


def test_codec_methods(codec, torch, fec):
    """Codec.rs_reconstruct_some_wide / _split on [B, n, S] tensors, shard_len below the slot size."""
    k, m, S, L, nb = 40, 20, 48, 41, 9
    n = k + m
    sh = torch.randint(0, 256, (nb, n, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode(k, m, sh, shard_len=L)
    ref = sh.clone()
    present = np.ones((nb, n), dtype=bool)
    holes = [(3, 1), (3, k + 12), (5, k), (7, 32), (7, 31)]
    for b, i in holes:
        present[b, i] = False
        sh[b, i] = ERASED
        ref[b, i, L:] = ERASED      # the slot's bytes past round_up(L, 16) are not written
        ref[b, i, L:rup16(L)] = 0
    masks = words(torch, fec.wide_masks(present))
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    work = sh.clone()
    assert codec.rs_reconstruct_some_wide(k, m, work, masks, status=st, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert torch.equal(work, ref) and (st == 0).all()
    data, par = sh[:, :k].contiguous(), sh[:, k:].contiguous()
    w = np.zeros((nb, n), dtype=bool)
    w[:, k + 12] = True
    assert codec.rs_reconstruct_some_wide_split(k, m, data, par, masks, want=words(torch, fec.wide_masks(w)),
                                                shard_len=L) == fec.FEC_OK
    codec.sync()
    assert torch.equal(par[3, 12], ref[3, k + 12]) and torch.equal(data, sh[:, :k]) and torch.equal(par[5], sh[5, k:])
    with pytest.raises(AssertionError):
        codec.rs_reconstruct_some_wide(k, m, sh.cpu(), masks, shard_len=L)
    with pytest.raises(AssertionError):      # want has the masks' shape
        codec.rs_reconstruct_some_wide(k, m, work, masks, want=masks[:, :1].contiguous(), shard_len=L)


def test_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx: an empty batch, null pointers, the layouts, then the alignment of the
    present masks, the statuses and the want masks; a 2^32 shard stride is refused (the rebuild takes
    32-bit shard strides). RS(20,13) with two mask words: the wide path."""
    h, D = codec.handle, fec.FEC_DEVICE
    k, m, ss, bs = 20, 13, 16, 33 * 16
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    w = torch.zeros((16,), dtype=torch.int32, device="cuda")   # masks: nothing present, want: nothing
    st = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    p, mk, s = buf.data_ptr(), w.data_ptr(), st.data_ptr()
    pp = p + k * ss
    INV, ALN = fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_ALIGNMENT
    F = fec.lib.fec_rs_reconstruct_some_wide_batch
    assert F(h, k, m, 16, 0, None, 0, None, 0, 16, None, None, 2, None, D) == fec.FEC_OK
    assert F(h, k, m, 16, 2, None, bs, pp, bs, ss, mk, None, 2, s, D) == INV
    assert F(h, k, m, 16, 2, p, bs, None, bs, ss, mk, None, 2, s, D) == INV
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, None, None, 2, s, D) == INV
    assert F(h, k, m, 16, 2, p + 8, bs, pp, bs, ss, mk, None, 2, s, D) == ALN
    assert F(h, k, m, 17, 2, p, bs, pp, bs, ss, mk, None, 2, s, D) == INV
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, mk + 2, None, 2, s, D) == ALN
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, mk, None, 2, s + 2, D) == ALN
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, mk, mk + 34, 2, s, D) == ALN     # a misaligned want mask
    assert F(h, k, m, 17, 2, p, bs, pp, bs, ss, mk + 2, mk + 34, 2, s, D) == INV     # the layouts come first
    assert F(h, k, m, 16, 2, p, 16, p + 2048, 16, 1 << 32, mk, None, 2, s, D) == INV
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, mk, None, 1, s, D) == INV        # mask_words before them all
    assert codec.lib_sync_rc() == fec.FEC_OK
    # m == 0: the parity region may be NULL
    assert F(h, 40, 0, 16, 2, p, 40 * 16, None, 0, 16, mk, mk + 32, 2, s, D) == fec.FEC_OK
    # nothing present, nothing wanted: untouched, status 0 (block_status is optional)
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, mk, mk + 32, 2, s, D) == fec.FEC_OK
    assert F(h, k, m, 16, 2, p, bs, pp, bs, ss, mk, mk + 32, 2, None, D) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and st.cpu().tolist() == [0, 0, 99, 99]
