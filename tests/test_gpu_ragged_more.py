"""Ragged verify and ragged reconstruct-some on the GPU (include/fec_hip_ragged.h) against the batches
of ragged_more_cases.py: expected parity from the CPU oracle (or the matrix models of cauchy_model.py
and custom_model.py) run per block at the block's own length, expected statuses from the masks and
the lengths.

Every batch lives in one canary-filled device arena with guards at both ends and gaps between the
blocks; after each call the WHOLE arena is compared byte for byte with a numpy model. Verify writes
nothing: the arena must come back as it went, whatever garbage the slots hold from a block's length
on. Reconstruct-some writes bytes [0, len) of the shards it rebuilds and zeros to round_up(len, 16):
every other byte, of failed, zero-length and oversize blocks too, must stay. The knob rag_g forces
the blocks per tile, so that tile and wave edges fall on every kind of block.
"""
import numpy as np
import pytest

import ragged_more_cases as rc
from arena import CANARY, STALE, check_arena, codec, rup16, torch  # noqa: F401
from ragged_more_cases import B, ERASED, MAXL, RAG_G, S, SHARD_SIZE, SINGULAR, TOO_FEW

pytestmark = pytest.mark.gpu


def upload(torch, img):
    dev = torch.from_numpy(img).cuda()
    assert dev.data_ptr() % 16 == 0
    return dev


def words(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def stale(torch, n, value=STALE):
    return torch.full((n,), value, dtype=torch.int32, device="cuda")


def lay_args(dev, data, par, nb, maxl=MAXL):
    p = dev.data_ptr()
    return maxl, nb, p + data.off, data.bs, p + par.off, par.bs, data.ss


def run_verify(codec, fec, torch, c, layout, ss=S, maxl=MAXL, count=True):
    """One ragged verify of a batch: statuses, the count, a clean sync, the arena untouched."""
    nb = c["lens"].size
    img, data, par = rc.verify_image(c, layout, ss)
    dev = upload(torch, img)
    dl, st = words(torch, c["lens"]), stale(torch, nb)
    cnt = stale(torch, 1) if count else None
    rc_ = codec.rs_verify_ragged_raw(c["k"], c["m"], *lay_args(dev, data, par, nb, maxl), dl.data_ptr(), st.data_ptr(),
                                     cnt.data_ptr() if count else None)
    assert rc_ == fec.FEC_OK
    # a mismatch does not touch the sticky word; an oversize block does
    assert codec.lib_sync_rc() == (SHARD_SIZE if (c["status"] == SHARD_SIZE).any() else fec.FEC_OK)
    assert codec.lib_sync_rc() == fec.FEC_OK
    got = st.cpu().numpy()
    print("verify RS(%d,%d) %s: %d bad of %d, count %s" % (c["k"], c["m"], layout, (got == 0).sum(), nb,
                                                           cnt.cpu().numpy().tolist() if count else None))
    assert np.array_equal(got, c["status"])
    if count:
        assert cnt.cpu().numpy().tolist() == [c["count"]]
    check_arena(dev.cpu().numpy(), img, "ragged verify")


def run_some(codec, fec, torch, c, layout, which, ss=S, maxl=MAXL):
    """One ragged reconstruct-some of a batch, with its want masks (which = "want") or without."""
    nb = c["lens"].size
    img, model, data, par = rc.some_images(c, layout, which, ss)
    dev = upload(torch, img)
    dl, dm, st = words(torch, c["lens"]), words(torch, c["masks"]), stale(torch, nb)
    dw = words(torch, c["wants"]) if which == "want" else None
    rc_ = codec.rs_reconstruct_some_ragged_raw(c["k"], c["m"], *lay_args(dev, data, par, nb, maxl), dm.data_ptr(),
                                               dl.data_ptr(), dw.data_ptr() if dw is not None else None, st.data_ptr())
    assert rc_ == fec.FEC_OK
    assert codec.lib_sync_rc() == rc.sync_code(c["st_" + which], c["by_mask_" + which])
    assert codec.lib_sync_rc() == fec.FEC_OK   # reported once, then cleared
    assert np.array_equal(st.cpu().numpy(), c["st_" + which])
    check_arena(dev.cpu().numpy(), model, "ragged reconstruct-some (%s)" % which)


# ------------------------------------------------------------------ verify

@pytest.mark.parametrize("rag_g", RAG_G)
@pytest.mark.parametrize("layout", ["interleaved", "split"])
@pytest.mark.parametrize("k,m,nb", rc.VERIFY_SHAPES)
def test_ragged_verify(codec, oracle, torch, fec, tune, k, m, nb, layout, rag_g):
    """RS(10,22): two row passes, a corrupt data shard found by both and counted once, a parity row
    >= 16 seen by the second alone; RS(100,40): three passes, each of up to 1600 tables staged in LDS;
    RS(130,20): a first pass of 2080 tables, more than LDS keeps, read from global memory (the
    <MAXM, false> instance), then a pass of 4 rows from LDS."""
    tune(rag_g=rag_g)
    c = rc.verify_case(rc.oracle_encode(oracle), k, m, nb)
    run_verify(codec, fec, torch, c, layout)
    if rag_g == 0:
        run_verify(codec, fec, torch, c, layout, count=False)


@pytest.mark.parametrize("rag_g", [0, 16])
def test_ragged_verify_of_long_shards_counts_a_block_once(codec, oracle, torch, fec, tune, rag_g):
    """RS(4,2), max_shard_len 70 000, blocks of 70 000, 1 and 33 333 bytes: tiles of three windows and
    more. Block 0 has a corrupt byte in its first and in its last window, block 2 in its last chunk."""
    tune(rag_g=rag_g)
    k, m, L = 4, 2, 70000
    hits = {0: [(1, 100), (k + 1, L - 1)], 2: [(0, 33332)]}
    c = rc.verify_case(rc.oracle_encode(oracle), k, m, 3, lens=[70000, 1, 33333], key="long", ss=L, maxl=L, hits=hits)
    assert c["status"].tolist() == [0, 1, 0] and c["count"] == 2 and len(c["flips"]) == 3
    run_verify(codec, fec, torch, c, "split", ss=L, maxl=L)


# ------------------------------------------------------------------ reconstruct-some

@pytest.mark.parametrize("rag_g", RAG_G)
@pytest.mark.parametrize("layout", ["interleaved", "split"])
@pytest.mark.parametrize("k,m", rc.SOME_SHAPES)
def test_ragged_reconstruct_some(codec, oracle, torch, fec, tune, k, m, layout, rag_g):
    """RS(10,22) and RS(1,31): two row passes of up to 22 and 31 rows; RS(5,0): no parity region."""
    tune(rag_g=rag_g)
    c = rc.some_case(rc.oracle_encode(oracle), k, m)
    run_some(codec, fec, torch, c, layout, "want")
    run_some(codec, fec, torch, c, layout, "all")


@pytest.mark.parametrize("rag_g", [0, 16])
def test_ragged_reconstruct_some_of_long_shards(codec, oracle, torch, fec, tune, rag_g):
    tune(rag_g=rag_g)
    k, m, L = 4, 2, 70000
    lost = np.array([[0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0]], dtype=bool)
    c = rc.some_case(rc.oracle_encode(oracle), k, m, 3, lens=[70000, 1, 33333], key="long", ss=L, maxl=L, lost=lost,
                     want=np.ones((3, 6), dtype=bool))
    assert c["rebuilt_all"].sum() == 5
    run_some(codec, fec, torch, c, "split", "all", ss=L, maxl=L)


# ------------------------------------------------------------------ the uniform calls

@pytest.mark.parametrize("L", [17, 1200])
@pytest.mark.parametrize("k,m", [(8, 4), (20, 10)])
def test_ragged_calls_equal_uniform_calls_at_one_length(codec, oracle, torch, fec, k, m, L):
    """With every block_len = L both calls leave the arena, the statuses, the count and the sync code
    as fec_rs_verify_batch and fec_rs_reconstruct_some_batch with shard_len = L do."""
    nb = B
    lens = np.full(nb, L, dtype=np.uint32)
    dl = words(torch, lens)
    h, D = codec.handle, fec.FEC_DEVICE
    enc = rc.oracle_encode(oracle)
    v = rc.verify_case(enc, k, m, nb, lens=lens, key=("uniform", L))
    img, data, par = rc.verify_image(v, "interleaved")
    got = []
    for ragged in (False, True):
        dev = upload(torch, img)
        st, cnt = stale(torch, nb), stale(torch, 1)
        la = lay_args(dev, data, par, nb, L)
        rc_ = (codec.rs_verify_ragged_raw(k, m, *la, dl.data_ptr(), st.data_ptr(), cnt.data_ptr()) if ragged else
               fec.lib.fec_rs_verify_batch(h, k, m, *la, st.data_ptr(), cnt.data_ptr(), D))
        assert rc_ == fec.FEC_OK
        got.append((codec.lib_sync_rc(), st.cpu().numpy(), cnt.cpu().numpy().tolist(), dev.cpu().numpy()))
    assert got[0][0] == got[1][0] == fec.FEC_OK and got[0][2] == got[1][2] == [v["count"]] and v["count"] > 0
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[1][1], v["status"])
    check_arena(got[1][3], got[0][3], "ragged verify against the uniform call")
    s = rc.some_case(enc, k, m, nb, lens=lens, key=("uniform", L))
    dm, dw = words(torch, s["masks"]), words(torch, s["wants"])
    for which, want_ptr in (("want", dw.data_ptr()), ("all", None)):
        img, model, data, par = rc.some_images(s, "split", which)
        got = []
        for ragged in (False, True):
            dev = upload(torch, img)
            st = stale(torch, nb)
            la = lay_args(dev, data, par, nb, L)
            rc_ = (codec.rs_reconstruct_some_ragged_raw(k, m, *la, dm.data_ptr(), dl.data_ptr(), want_ptr,
                                                        st.data_ptr()) if ragged else
                   fec.lib.fec_rs_reconstruct_some_batch(h, k, m, *la, dm.data_ptr(), want_ptr, st.data_ptr(), D))
            assert rc_ == fec.FEC_OK
            got.append((codec.lib_sync_rc(), st.cpu().numpy(), dev.cpu().numpy()))
        assert got[0][0] == got[1][0] == rc.sync_code(s["st_" + which])
        assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[1][1], s["st_" + which])
        check_arena(got[1][2], got[0][2], "ragged reconstruct-some against the uniform call")
        check_arena(got[1][2], model, "ragged reconstruct-some at one length")
        assert not np.array_equal(got[1][2], img)   # the call did something


# ------------------------------------------------------------------ oversize blocks

def oversize_lens(nb):
    lens = rc.default_lens(nb).copy()
    lens[[5, 17]] = MAXL + 1
    lens[30] = 0xFFFFFFFF
    return lens


@pytest.mark.parametrize("rag_g", [0, 3])
def test_oversize_blocks_are_skipped_and_reported(codec, oracle, torch, fec, tune, rag_g):
    """Two blocks of length MAXL + 1 and one of 0xFFFFFFFF: untouched, status FEC_ERR_SHARD_SIZE, not
    counted, fec_sync FEC_ERR_SHARD_SIZE once; a too-few-shards block in the same call comes first."""
    tune(rag_g=rag_g)
    k, m, nb = 8, 4, 40
    enc = rc.oracle_encode(oracle)
    lens = oversize_lens(nb)
    v = rc.verify_case(enc, k, m, nb, lens=lens, key="oversize")
    assert (v["status"] == SHARD_SIZE).sum() == 3 and v["count"] == (v["status"] == 0).sum() > 0
    run_verify(codec, fec, torch, v, "interleaved")
    # every block loses one data shard and one parity shard: none fails by its mask
    n = k + m
    rng = np.random.default_rng(40)
    lost = np.zeros((nb, n), dtype=bool)
    lost[np.arange(nb), rng.integers(0, k, nb)] = True
    lost[np.arange(nb), k + rng.integers(0, m, nb)] = True
    s = rc.some_case(enc, k, m, nb, lens=lens, key="oversize", lost=lost, want=np.ones((nb, n), dtype=bool))
    assert (s["st_all"] == SHARD_SIZE).sum() == 3 and (s["st_all"] == 0).sum() == nb - 3
    assert rc.sync_code(s["st_all"], s["by_mask_all"]) == SHARD_SIZE
    run_some(codec, fec, torch, s, "split", "all")
    # the same with a too-few block of a valid length, and an oversize block whose mask has too few
    lost2 = lost.copy()
    lost2[[3, 17], :m + 1] = True
    s2 = rc.some_case(enc, k, m, nb, lens=lens, key="oversize_few", lost=lost2, want=np.ones((nb, n), dtype=bool))
    assert s2["st_all"][3] == TOO_FEW and s2["st_all"][17] == SHARD_SIZE and s2["by_mask_all"][17] == TOO_FEW
    assert rc.sync_code(s2["st_all"], s2["by_mask_all"]) == TOO_FEW
    run_some(codec, fec, torch, s2, "interleaved", "all")


def test_verify_of_a_code_without_parity_says_one_for_every_block(codec, oracle, torch, fec):
    """m == 0 comes before the oversize rule: nothing is launched, every status is 1, the oversize
    blocks' too, nothing is counted and fec_sync() returns FEC_OK."""
    k, m, nb = 5, 0, 40
    v = rc.verify_case(rc.oracle_encode(oracle), k, m, nb, lens=oversize_lens(nb), key="no parity")
    assert (v["lens"] > MAXL).sum() == 3 and (v["status"] == 1).all() and v["count"] == 0
    run_verify(codec, fec, torch, v, "split")


# ------------------------------------------------------------------ matrix kinds

@pytest.mark.parametrize("k,m", [(8, 4), (20, 10)])
def test_cauchy_codes(oracle, torch, fec, k, m):
    import cauchy_model as cm
    enc = rc.matrix_encode(cm.matrix(k, m))
    cdc = fec.Codec(0, matrix="cauchy").use_torch_stream()
    try:
        run_verify(cdc, fec, torch, rc.verify_case(enc, k, m, B, key="cauchy"), "split")
        s = rc.some_case(enc, k, m, B, key="cauchy")
        run_some(cdc, fec, torch, s, "interleaved", "want")
        run_some(cdc, fec, torch, s, "split", "all")
    finally:
        cdc.close()


@pytest.mark.parametrize("k,m,name", [(8, 4, "lrc"), (20, 10, "cauchy255")])
def test_custom_codes(oracle, torch, fec, k, m, name):
    """A custom matrix; the (8,4) one is not MDS: blocks whose first k present rows are dependent get
    FEC_ERR_SINGULAR and have nothing written."""
    import custom_model as cu
    n = k + m
    P = cu.rows(name, k, m)
    M = cu.matrix(P)
    enc = rc.matrix_encode(M)
    cdc = fec.Codec(0).use_torch_stream()
    try:
        # selected but not registered
        cdc.set_matrix("custom")
        one = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        w = stale(torch, 4)
        p = one.data_ptr()
        la = (16, 1, p, n * 16, p + k * 16, n * 16, 16)
        assert cdc.rs_verify_ragged_raw(k, m, *la, w.data_ptr(), w.data_ptr() + 4) == fec.FEC_ERR_NO_MATRIX
        assert cdc.rs_reconstruct_some_ragged_raw(k, m, *la, w.data_ptr(), w.data_ptr() + 4, None,
                                                  w.data_ptr() + 8) == fec.FEC_ERR_NO_MATRIX
        assert (w.cpu().numpy() == STALE).all() and cdc.lib_sync_rc() == fec.FEC_OK
        cdc.set_custom_matrix(k, m, P)
        run_verify(cdc, fec, torch, rc.verify_case(enc, k, m, B, key=name), "interleaved")
        # the default batch's losses, with blocks that lose data shard 4 alone among them
        base = rc.some_case(enc, k, m, B, key=(name, "base"))
        lost = base["lost"].copy()
        lost[10:300:29] = False
        lost[10:300:29, 4] = True
        singular = np.array([cu.decode(M, ~lost[b]) is cu.SINGULAR for b in range(B)])
        s = rc.some_case(enc, k, m, B, key=name, lost=lost, singular=singular)
        if name == "lrc":
            assert singular[10] and (s["st_all"] == SINGULAR).sum() >= 10 and (s["st_want"] == SINGULAR).any()
            assert not s["rebuilt_all"][s["st_all"] == SINGULAR].any()
        else:
            assert not singular.any()
        assert (s["st_all"] == 0).any() and s["rebuilt_all"].any()
        run_some(cdc, fec, torch, s, "split", "want")
        run_some(cdc, fec, torch, s, "interleaved", "all")
    finally:
        cdc.close()


# ------------------------------------------------------------------ arguments the device sees

def test_misaligned_block_len_is_refused_and_empty_batches_write_nothing(codec, oracle, torch, fec):
    k, m, nb = 8, 4, 16
    img, data, par = rc.make_arena("split", nb, k, m)
    dev = upload(torch, img)
    dl = torch.full((nb + 1,), MAXL, dtype=torch.int32, device="cuda")
    dm = torch.full((nb,), 0xFFE, dtype=torch.int32, device="cuda")   # data shard 0 lost: recoverable
    st, cnt = stale(torch, nb), stale(torch, 1)
    la = lay_args(dev, data, par, nb)
    for off in (1, 2, 3):
        assert codec.rs_verify_ragged_raw(k, m, *la, dl.data_ptr() + off, st.data_ptr(),
                                          cnt.data_ptr()) == fec.FEC_ERR_ALIGNMENT
        assert codec.rs_reconstruct_some_ragged_raw(k, m, *la, dm.data_ptr(), dl.data_ptr() + off, None,
                                                    st.data_ptr()) == fec.FEC_ERR_ALIGNMENT
    # no blocks: nothing at all, the statuses and the count included
    la0 = (MAXL, 0) + la[2:]
    assert codec.rs_verify_ragged_raw(k, m, *la0, dl.data_ptr(), st.data_ptr(), cnt.data_ptr()) == fec.FEC_OK
    assert codec.rs_reconstruct_some_ragged_raw(k, m, *la0, dm.data_ptr(), dl.data_ptr(), None,
                                                st.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (dev.cpu().numpy() == CANARY).all() and (st.cpu().numpy() == STALE).all()
    assert (cnt.cpu().numpy() == STALE).all()
    # every block of length 0: no shard byte is read or moves; verify says 1, the masks give 0
    dl[:] = 0
    assert codec.rs_verify_ragged_raw(k, m, *la, dl.data_ptr(), st.data_ptr(), cnt.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (st.cpu().numpy() == 1).all() and cnt.cpu().numpy().tolist() == [0]
    assert codec.rs_reconstruct_some_ragged_raw(k, m, *la, dm.data_ptr(), dl.data_ptr(), None,
                                                st.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK and (st.cpu().numpy() == 0).all()
    assert (dev.cpu().numpy() == CANARY).all()


# ------------------------------------------------------------------ the heal loop

@pytest.mark.parametrize("form", ["interleaved", "split"])
def test_heal_loop_queued_without_a_sync(codec, oracle, torch, fec, form):
    """Ragged encode, shards dropped and corrupted on the device, ragged verify (flags them), ragged
    reconstruct-some with the dropped shards' masks, ragged verify (all clean, count 0): five steps on
    one stream, one sync at the end. Through the tensor methods of Codec, on compact buffers."""
    k, m, nb = 8, 4, 70
    n = k + m
    lens = rc.default_lens(nb)
    ok = rc.usable(lens)
    rng = np.random.default_rng(8470)
    data = rng.integers(0, 256, (nb, k, S), dtype=np.uint8)
    sh = rc.encoded(rc.oracle_encode(oracle), k, m, data, ok)
    v = rc.span_mask(0 * ok, ok, S)
    host = np.full((nb, n, S), CANARY, dtype=np.uint8)
    host[:, :k] = np.where(v, sh[:, :k], CANARY)
    # every third block loses one or two shards, data and parity
    drop = np.zeros((nb, n), dtype=bool)
    for b in range(0, nb, 3):
        drop[b, rng.choice(n, size=1 + b % 2, replace=False)] = True
    masks = rc.pack(~drop)
    if form == "interleaved":
        dev = torch.from_numpy(host).cuda()
    else:
        dd, dp = torch.from_numpy(host[:, :k].copy()).cuda(), torch.from_numpy(host[:, k:].copy()).cuda()
    dl, dm = words(torch, lens), words(torch, masks)
    st0, st1, st2, st3 = (stale(torch, nb) for _ in range(4))
    c1, c2 = stale(torch, 1), stale(torch, 1)
    tdrop = torch.from_numpy(drop).cuda()
    if form == "interleaved":
        codec.rs_encode_ragged(k, m, dev, dl, status=st0)
        dev[tdrop] = ERASED
        codec.rs_verify_ragged(k, m, dev, dl, st1, c1)
        codec.rs_reconstruct_some_ragged(k, m, dev, dm, dl, status=st2)
        codec.rs_verify_ragged(k, m, dev, dl, st3, count=c2)
    else:
        codec.rs_encode_ragged_split(k, m, dd, dp, dl, status=st0)
        dd[tdrop[:, :k]] = ERASED
        dp[tdrop[:, k:]] = ERASED
        codec.rs_verify_ragged_split(k, m, dd, dp, dl, st1, c1)
        codec.rs_reconstruct_some_ragged_split(k, m, dd, dp, dm, dl, status=st2)
        codec.rs_verify_ragged_split(k, m, dd, dp, dl, st3, count=c2)
    assert codec.lib_sync_rc() == fec.FEC_OK
    # (a dropped shard shows only where its bytes below the block's length differ from the fill)
    flagged = (drop & (np.where(v, sh, ERASED) != ERASED).any(axis=2)).any(axis=1)
    assert flagged.sum() >= 15 and not flagged[ok == 0].any()
    assert (st0.cpu().numpy() == 0).all() and (st2.cpu().numpy() == 0).all()
    assert np.array_equal(st1.cpu().numpy(), np.where(flagged, 0, 1)) and c1.cpu().numpy().tolist() == [flagged.sum()]
    assert (st3.cpu().numpy() == 1).all() and c2.cpu().numpy().tolist() == [0]
    # the image: the encoded batch, the dropped shards healed (zeros to round_up(len, 16), the rest of
    # their slots as the drop left it)
    want = np.where(v, sh, CANARY).astype(np.uint8)
    want[:, k:] = np.where(rc.span_mask(ok, rup16(ok), S), 0, want[:, k:])
    healed = np.where(v, sh, np.where(rc.span_mask(ok, rup16(ok), S), 0, ERASED)).astype(np.uint8)
    healed[ok == 0] = ERASED
    want = np.where(drop[:, :, None], healed, want)
    got = dev.cpu().numpy() if form == "interleaved" else np.concatenate([dd.cpu().numpy(), dp.cpu().numpy()], axis=1)
    check_arena(got.reshape(-1), want.reshape(-1), "heal loop")
