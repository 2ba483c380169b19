"""Ragged batches on the GPU: fec_rs_encode_ragged_batch, fec_rs_reconstruct_ragged_batch and
fec_rs_recover_ragged_batch against the CPU oracle run per block at the block's own length.

Every batch (data, parity, out) lives in one device arena pre-filled with a canary, with guards at
both ends and gaps between the regions; after each call the WHOLE arena is compared byte for byte
with a numpy model: the image before the call with only the bytes the header lets the call write
changed (bytes [0, len_b) of an output shard = the oracle's, [len_b, round_up(len_b, 16)) = 0). Input
slots hold canary bytes from len_b on, so a kernel that reads a neighbour's length, lets the tail of
a partial chunk leak, touches a block of length 0, an oversize block, a failed block, a slot's slack
or a guard fails here. The knob rag_g forces the blocks per tile, so the tile edges fall on every
kind of block.
"""
import numpy as np
import pytest

from arena import CANARY, GUARD, Region, canary_image, check_arena, codec, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

ERASED = 0x5A
GAP = 208
S = 1216
MAXL = 1202
B = 301
PATTERN = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1200, 1201, 1202]
RAG_G = [0, 1, 3, 16]

# RS(10,22): two row passes of the encode (m = 12 is one pass; 22 parity rows make two), RS(100,40):
# three passes with 100 inputs; RS(140,20): a 16-row pass of 2240 tables, past the 2048 kept in LDS
ENC_SHAPES = [(8, 4, B), (20, 10, B), (2, 1, B), (1, 1, B), (31, 1, B), (10, 22, B), (100, 40, 20), (140, 20, 20)]
# rebuild instances by the rows a block can need: RS(2,1) 1, RS(8,4) 4, RS(20,10) and RS(10,22) 10
# (the 12-row instance), RS(16,16) 16; single-slot recovers take the 1-row instance of every code
DEC_SHAPES = [(8, 4), (20, 10), (2, 1), (10, 22), (16, 16)]

KIND_COMPLETE, KIND_ONE, KIND_MAX, KIND_FEW, KIND_FIRSTK = range(5)


def default_lens(nb):
    lens = np.array([PATTERN[b % 14] for b in range(nb)], dtype=np.uint32)
    if nb >= 216:
        lens[100:120] = 0
        lens[200:216] = MAXL
    return lens


def span_mask(lo, hi, width):
    """bool [len(lo), 1, width]: byte x of block b lies in [lo[b], hi[b])."""
    x = np.arange(width)[None, None, :]
    return (x >= np.asarray(lo)[:, None, None]) & (x < np.asarray(hi)[:, None, None])


def make_arena(layout, nb, k, m, slots, ss=S):
    """(image, data, parity, out): one canary-filled arena holding the three regions."""
    n = k + m
    if layout == "interleaved":
        data = Region(GUARD, n * ss, ss, k, nb)
        par = Region(GUARD + k * ss, n * ss, ss, m, nb)
        top = GUARD + nb * n * ss
    else:   # split: the parity region below the data region
        par = Region(GUARD, m * ss, ss, m, nb)
        data = Region(par.end() + GAP, k * ss, ss, k, nb)
        top = data.end()
    out = Region(top + GAP, max(slots, 1) * ss, ss, max(slots, 1), nb)
    return canary_image([data, par, out]), data, par, out


def make_masks(rng, k, m, nb):
    """Present masks over the kinds the code can have, kind (b // 14 + b % 14) % kinds so that every
    residue of the length pattern meets every kind. Returns masks, kinds and, per block, the index
    of a present parity shard that is not among the first k present (or -1)."""
    n = k + m
    emax = min(k, m)
    kinds = [KIND_COMPLETE, KIND_ONE, KIND_FEW] + ([KIND_MAX] if emax >= 2 else []) + ([KIND_FIRSTK] if m >= 2 else [])
    kind = np.array([kinds[(b // 14 + b % 14) % len(kinds)] for b in range(nb)])
    masks = np.empty(nb, dtype=np.uint32)
    extra = np.full(nb, -1)
    for b in range(nb):
        kd = kind[b]
        if kd == KIND_COMPLETE:
            lost = []
        elif kd == KIND_ONE:
            lost = [int(rng.integers(0, k))] + list(k + rng.choice(m, size=int(rng.integers(0, m)), replace=False))
        elif kd == KIND_MAX:
            lost = list(rng.choice(k, size=emax, replace=False)) + \
                list(k + rng.choice(m, size=int(rng.integers(0, m - emax + 1)), replace=False))
        elif kd == KIND_FEW:
            d0 = int(rng.integers(0, k))
            rest = [i for i in range(n) if i != d0]
            lost = [d0] + list(rng.choice(rest, size=m, replace=False))
        else:   # every parity present, fewer data shards lost than parities: the last parity is spare
            lost = list(rng.choice(k, size=int(rng.integers(1, min(k, m - 1) + 1)), replace=False))
            extra[b] = n - 1
        masks[b] = ((1 << n) - 1) & ~sum(1 << int(i) for i in lost)
    return masks, kind, extra


_enc_cases = {}
_dec_cases = {}


def enc_case(oracle, k, m, nb, lens=None, key=None):
    """Data [nb, k, S] (random over the whole slot) and the oracle's parity of each block's data
    zero-padded to S; computed once per shape and left unchanged."""
    ck = (k, m, nb, key)
    if ck not in _enc_cases:
        rng = np.random.default_rng(1000003 * k + 1009 * m + nb)
        lens = default_lens(nb) if lens is None else np.asarray(lens, dtype=np.uint32)
        ok = np.where(lens <= MAXL, lens, 0)
        data = rng.integers(0, 256, (nb, k, S), dtype=np.uint8)
        sh = np.zeros((nb, k + m, S), dtype=np.uint8)
        sh[:, :k] = np.where(span_mask(0 * ok, ok, S), data, 0)
        oracle.rs_encode(k, m, sh)
        for a in (lens, ok, data, sh):
            a.setflags(write=False)
        _enc_cases[ck] = dict(lens=lens, ok=ok, data=data, sh=sh)
    return _enc_cases[ck]


def dec_case(oracle, k, m, nb=B, lens=None, key=None, all_ok=False):
    """Encoded batch, masks of every kind, the damaged input and the oracle's reconstruct of each
    block at its own length. The case itself asserts that it holds every kind of block, and every
    kind at a length of 0, of 1 and of MAXL."""
    ck = (k, m, nb, key)
    if ck in _dec_cases:
        return _dec_cases[ck]
    n = k + m
    pattern = lens is None   # the default lengths: every kind must meet lengths 0, 1 and MAXL
    e = enc_case(oracle, k, m, nb, lens, key)
    lens, ok, sh = e["lens"], e["ok"], e["sh"]
    rng = np.random.default_rng(7919 * k + 31 * m + nb)
    masks, kind, extra = make_masks(rng, k, m, nb)
    if all_ok:   # every block recoverable with one erasure (the oversize tests' batches)
        masks = (((1 << n) - 1) & ~(1 << rng.integers(0, k, nb))).astype(np.uint32)
        kind, extra = np.full(nb, KIND_ONE), np.full(nb, -1)
    lost = ((masks[:, None] >> np.arange(n)[None, :]) & 1) == 0
    e_d = lost[:, :k].sum(axis=1)
    few = (e_d > 0) & ((n - lost.sum(axis=1)) < k)
    if not all_ok:
        emax = min(k, m)
        want = {KIND_COMPLETE: (e_d == 0), KIND_ONE: (e_d == 1) & ~few, KIND_MAX: (e_d == emax) & ~few,
                KIND_FEW: few}
        if m >= 2:
            # a present parity past the first k present shards, holding garbage below
            pres_before = np.array([int((~lost[b, :extra[b]]).sum()) if extra[b] >= 0 else 0 for b in range(nb)])
            want[KIND_FIRSTK] = (extra >= 0) & (pres_before >= k) & (e_d >= 1) & ~few
            assert all(not lost[b, extra[b]] for b in range(nb) if extra[b] >= 0)
        for name, sel in want.items():
            assert sel.any(), "the batch holds no block of kind %d" % name
            if pattern and nb == B:
                for length in (0, 1, MAXL):
                    assert (sel & (lens == length)).any(), "kind %d does not occur at length %d" % (name, length)
    dmg = sh.copy()
    dmg[lost] = ERASED
    for b in np.flatnonzero(extra >= 0):
        dmg[b, extra[b]] = rng.integers(0, 256, S, dtype=np.uint8)
    rec = dmg.copy()
    for length in np.unique(ok):
        if length == 0:
            continue
        idx = np.flatnonzero(ok == length)
        sub = np.ascontiguousarray(dmg[idx][:, :, :length])
        st = oracle.rs_reconstruct(k, m, sub, masks[idx])
        assert np.array_equal(st != 0, few[idx])
        rec[idx, :, :length] = sub
    # the oracle gives the original data back wherever it can, garbage spare parity or not
    v = span_mask(0 * ok, ok, S)
    good = ~few
    assert np.array_equal(np.where(v, rec[:, :k], 0)[good], sh[:, :k][good])
    for a in (masks, lost, e_d, few, dmg, rec):
        a.setflags(write=False)
    _dec_cases[ck] = dict(e, masks=masks, lost=lost, e_d=e_d, few=few, dmg=dmg, rec=rec)
    return _dec_cases[ck]


def upload(torch, img):
    dev = torch.from_numpy(img).cuda()
    assert dev.data_ptr() % 16 == 0
    return dev


def dev_words(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def shards_of(dev, reg, rows=None):
    """The [nb, rows, S] tensor view of a compact region of the device arena."""
    rows = reg.rows if rows is None else rows
    assert reg.bs == rows * reg.ss
    return dev[reg.off:reg.off + reg.B * reg.bs].view(reg.B, rows, reg.ss)


def expect_sync(codec, fec, st_want):
    rc = codec.lib_sync_rc()
    want = (fec.FEC_ERR_TOO_FEW_SHARDS if (st_want == fec.FEC_ERR_TOO_FEW_SHARDS).any() else
            fec.FEC_ERR_INVALID_ARG if (st_want == fec.FEC_ERR_INVALID_ARG).any() else
            fec.FEC_ERR_SHARD_SIZE if (st_want == fec.FEC_ERR_SHARD_SIZE).any() else fec.FEC_OK)
    assert rc == want
    assert codec.lib_sync_rc() == fec.FEC_OK   # reported once, then cleared


# ------------------------------------------------------------------ the three steps, model and call

def fill_inputs(img, data, par, c, k, src):
    """Shards `src` [nb, n, S] into the data and parity slots, bytes [0, len_b); canary from len_b on."""
    v = span_mask(0 * c["ok"], c["ok"], data.ss)
    dv, pv = data.view(img), par.view(img)
    dv[...] = np.where(v, src[:, :k, :data.ss], CANARY)
    pv[...] = np.where(v, src[:, k:, :data.ss], CANARY)


def write_outputs(model_view, sel, values, ok):
    """Into the [nb, rows, ss] view: rows `sel` [nb, rows] receive values[..., :len_b] and zeros up
    to round_up(len_b, 16), for blocks of length ok[b] > 0."""
    ss = model_view.shape[2]
    body = span_mask(0 * ok, ok, ss) & sel[:, :, None]
    pad = span_mask(ok, rup16(ok.astype(np.int64)), ss) & sel[:, :, None]
    model_view[body] = values[body]
    model_view[pad] = 0


def run_encode(codec, fec, torch, c, k, m, layout, oversize_status=False):
    nb = c["lens"].size
    img, data, par, out = make_arena(layout, nb, k, m, 0)
    data.view(img)[...] = np.where(span_mask(0 * c["ok"], c["ok"], S), c["data"], CANARY)
    model = img.copy()
    write_outputs(par.view(model), np.ones((nb, m), dtype=bool), c["sh"][:, k:], c["ok"])
    dev = upload(torch, img)
    dl = dev_words(torch, c["lens"])
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    if layout == "interleaved":
        codec.rs_encode_ragged(k, m, shards_of(dev, Region(data.off, data.bs, S, k + m, nb), k + m), dl, status=st,
                               max_shard_len=MAXL)
    else:
        codec.rs_encode_ragged_split(k, m, shards_of(dev, data), shards_of(dev, par), dl, status=st,
                                     max_shard_len=MAXL)
    st_want = np.where(c["lens"] > MAXL, fec.FEC_ERR_SHARD_SIZE, 0)
    expect_sync(codec, fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    check_arena(dev.cpu().numpy(), model, "ragged encode")


def decode_statuses(fec, c, slots):
    """Statuses by the masks alone (slots 0: the in-place form), oversize lengths on top."""
    e_d, few = c["e_d"], c["few"]
    if slots == 0:
        st = np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS, 0)
    else:
        st = np.where(e_d == 0, 0, np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS,
                                            np.where(e_d > slots, fec.FEC_ERR_INVALID_ARG, e_d)))
    by_mask = st.copy()
    return np.where(c["lens"] > MAXL, fec.FEC_ERR_SHARD_SIZE, st), by_mask


def run_decode(codec, fec, torch, c, k, m, layout, slots):
    """slots 0: in-place reconstruct; else recover into `slots` out slots per block."""
    nb = c["lens"].size
    img, data, par, out = make_arena(layout, nb, k, m, slots)
    fill_inputs(img, data, par, c, k, c["dmg"])
    model = img.copy()
    lost_d, ok = c["lost"][:, :k], c["ok"]
    st_want, by_mask = decode_statuses(fec, c, slots)
    if slots == 0:
        write_outputs(data.view(model), lost_d & (by_mask == 0)[:, None], c["rec"][:, :k], ok)
    else:
        done = by_mask > 0
        assert (done & (ok > 0)).any()
        vals = np.zeros((nb, slots, S), dtype=np.uint8)
        sel = np.zeros((nb, slots), dtype=bool)
        for b in np.flatnonzero(done):
            idx = np.flatnonzero(lost_d[b])
            vals[b, :idx.size] = c["rec"][b, idx]
            sel[b, :idx.size] = True
        write_outputs(out.view(model), sel, vals, ok)
    dev = upload(torch, img)
    dl, dm = dev_words(torch, c["lens"]), dev_words(torch, c["masks"])
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    p = dev.data_ptr()
    if slots == 0 and layout == "interleaved":
        codec.rs_reconstruct_ragged(k, m, shards_of(dev, Region(data.off, data.bs, S, k + m, nb), k + m), dm, dl,
                                    status=st, max_shard_len=MAXL)
    elif slots == 0:
        codec.rs_reconstruct_ragged_split(k, m, shards_of(dev, data), shards_of(dev, par), dm, dl, status=st,
                                          max_shard_len=MAXL)
    elif layout == "split":
        codec.rs_recover_ragged_split(k, m, shards_of(dev, data), shards_of(dev, par), dm, dl, shards_of(dev, out),
                                      status=st, max_shard_len=MAXL)
    else:
        rc = codec.rs_recover_ragged_raw(k, m, MAXL, nb, p + data.off, data.bs, p + par.off, par.bs, S,
                                         dm.data_ptr(), dl.data_ptr(), p + out.off, out.bs, slots, st.data_ptr())
        assert rc == fec.FEC_OK
    expect_sync(codec, fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    check_arena(dev.cpu().numpy(), model, "ragged %s" % ("reconstruct" if slots == 0 else "recover"))


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("rag_g", RAG_G)
@pytest.mark.parametrize("layout", ["interleaved", "split"])
@pytest.mark.parametrize("k,m,nb", ENC_SHAPES)
def test_ragged_encode(codec, oracle, torch, fec, tune, k, m, nb, layout, rag_g):
    tune(rag_g=rag_g)
    run_encode(codec, fec, torch, enc_case(oracle, k, m, nb), k, m, layout)


@pytest.mark.parametrize("rag_g", RAG_G)
@pytest.mark.parametrize("layout", ["interleaved", "split"])
@pytest.mark.parametrize("k,m", DEC_SHAPES)
def test_ragged_reconstruct_in_place(codec, oracle, torch, fec, tune, k, m, layout, rag_g):
    tune(rag_g=rag_g)
    run_decode(codec, fec, torch, dec_case(oracle, k, m), k, m, layout, 0)


@pytest.mark.parametrize("rag_g", RAG_G)
@pytest.mark.parametrize("slots", ["1", "m"])
@pytest.mark.parametrize("k,m", DEC_SHAPES)
def test_ragged_recover(codec, oracle, torch, fec, tune, k, m, slots, rag_g):
    tune(rag_g=rag_g)
    c = dec_case(oracle, k, m)
    ns = 1 if slots == "1" else m
    if ns < min(k, m):
        # blocks with more erasures than slots, at every length of interest
        over = (c["e_d"] > ns) & ~c["few"]
        for length in (0, 1, MAXL):
            assert (over & (c["lens"] == length)).any()
    run_decode(codec, fec, torch, c, k, m, "split" if slots == "m" else "interleaved", ns)


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10)])
def test_ragged_calls_equal_uniform_calls_at_one_length(codec, oracle, torch, fec, k, m):
    """With every block_len = MAXL the ragged calls leave the arena, byte for byte, and the statuses
    as the uniform calls do."""
    nb, n = B, k + m
    lens = np.full(nb, MAXL, dtype=np.uint32)
    c = dec_case(oracle, k, m, nb, lens=lens, key="uniform")
    dl, dm = dev_words(torch, lens), dev_words(torch, c["masks"])
    h = codec.handle
    for step, slots in [("encode", 0), ("reconstruct", 0), ("recover", 1), ("recover", m)]:
        img, data, par, out = make_arena("split", nb, k, m, slots)
        fill_inputs(img, data, par, c, k, c["dmg"])
        if step == "encode":
            data.view(img)[...] = np.where(span_mask(0 * c["ok"], c["ok"], S), c["data"], CANARY)
        got = []
        for ragged in (False, True):
            dev = upload(torch, img)
            p = dev.data_ptr()
            st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
            lay = (p + data.off, data.bs, p + par.off, par.bs, S)
            if step == "encode":
                rc = (codec.rs_encode_ragged_raw(k, m, MAXL, nb, *lay, dl.data_ptr(), st.data_ptr()) if ragged else
                      fec.lib.fec_rs_encode_batch(h, k, m, MAXL, nb, *lay, fec.FEC_DEVICE))
                if not ragged:
                    st[:] = 0   # the uniform encode has no status
            elif step == "reconstruct":
                rc = (codec.rs_reconstruct_ragged_raw(k, m, MAXL, nb, *lay, dm.data_ptr(), dl.data_ptr(),
                                                      st.data_ptr()) if ragged else
                      fec.lib.fec_rs_reconstruct_batch(h, k, m, MAXL, nb, *lay, dm.data_ptr(), st.data_ptr(),
                                                       fec.FEC_DEVICE))
            else:
                rc = (codec.rs_recover_ragged_raw(k, m, MAXL, nb, *lay, dm.data_ptr(), dl.data_ptr(), p + out.off,
                                                  out.bs, slots, st.data_ptr()) if ragged else
                      fec.lib.fec_rs_recover_batch(h, k, m, MAXL, nb, *lay, dm.data_ptr(), p + out.off, out.bs,
                                                   slots, st.data_ptr(), fec.FEC_DEVICE))
            assert rc == fec.FEC_OK
            got.append((codec.lib_sync_rc(), st.cpu().numpy(), dev.cpu().numpy()))
        assert got[0][0] == got[1][0], step
        assert np.array_equal(got[0][1], got[1][1]), step
        check_arena(got[1][2], got[0][2], "ragged %s against the uniform call" % step)
        assert not np.array_equal(got[0][2], img)   # the call did something


@pytest.mark.parametrize("rag_g", [0, 3])
def test_oversize_blocks_are_skipped_and_reported(codec, oracle, torch, fec, tune, rag_g):
    """Two blocks of length MAXL + 1 and one of 0xFFFFFFFF: untouched, status FEC_ERR_SHARD_SIZE,
    fec_sync FEC_ERR_SHARD_SIZE once; a too-few-shards block in the batch comes first."""
    tune(rag_g=rag_g)
    k, m, nb = 8, 4, 40
    lens = default_lens(nb)
    lens[[5, 17]] = MAXL + 1
    lens[30] = 0xFFFFFFFF
    run_encode(codec, fec, torch, enc_case(oracle, k, m, nb, lens=lens, key="oversize"), k, m, "split")
    c = dec_case(oracle, k, m, nb, lens=lens, key="oversize", all_ok=True)
    assert not c["few"].any() and (c["e_d"] == 1).all()
    for slots in (0, 1):
        st_want, _ = decode_statuses(fec, c, slots)
        assert (st_want == fec.FEC_ERR_SHARD_SIZE).sum() == 3 and (st_want >= 0).sum() == nb - 3
        run_decode(codec, fec, torch, c, k, m, "interleaved", slots)   # sync: SHARD_SIZE once, then OK
    # the same batch with a too-few-shards block (a valid length) and an oversize block whose own
    # mask has too few shards: statuses -4 and -5, and fec_sync reports the too-few code
    masks = c["masks"].copy()
    masks[[3, 17]] = 0x3F
    lost = ((masks[:, None] >> np.arange(k + m)[None, :]) & 1) == 0
    e_d = lost[:, :k].sum(axis=1)
    few = e_d > m - lost[:, k:].sum(axis=1)
    assert few[3] and few[17] and few.sum() == 2
    dmg = c["dmg"].copy()
    dmg[lost] = ERASED
    c2 = dict(c, masks=masks, lost=lost, e_d=e_d, few=few, dmg=dmg)
    for slots in (0, 1):
        st_want, _ = decode_statuses(fec, c2, slots)
        assert st_want[3] == fec.FEC_ERR_TOO_FEW_SHARDS and st_want[17] == fec.FEC_ERR_SHARD_SIZE
        run_decode(codec, fec, torch, c2, k, m, "split", slots)


@pytest.mark.parametrize("rag_g", [0, 16])
def test_long_shards_are_cut_into_windows(codec, oracle, torch, fec, tune, rag_g):
    """RS(4,2), max_shard_len 70 000, blocks of 70 000, 1 and 33 333 bytes: tiles of several windows."""
    tune(rag_g=rag_g)
    k, m, L = 4, 2, 70000
    n = k + m
    lens = np.array([70000, 1, 33333], dtype=np.uint32)
    nb = lens.size
    rng = np.random.default_rng(70000)
    v = span_mask(0 * lens, lens, L)
    sh = np.zeros((nb, n, L), dtype=np.uint8)
    sh[:, :k] = np.where(v, rng.integers(0, 256, (nb, k, L), dtype=np.uint8), 0)
    oracle.rs_encode(k, m, sh)
    masks = np.array([0b111010, 0b110110, 0b011110], dtype=np.uint32)   # e = 2, 2, 1 (and a parity)
    lost = ((masks[:, None] >> np.arange(n)[None, :]) & 1) == 0
    dl, dm = dev_words(torch, lens), dev_words(torch, masks)
    # encode
    img, data, par, out = make_arena("split", nb, k, m, m, ss=L)
    data.view(img)[...] = np.where(v, sh[:, :k], CANARY)
    model = img.copy()
    write_outputs(par.view(model), np.ones((nb, m), dtype=bool), sh[:, k:], lens)
    dev = upload(torch, img)
    p = dev.data_ptr()
    lay = (p + data.off, data.bs, p + par.off, par.bs, L)
    assert codec.rs_encode_ragged_raw(k, m, L, nb, *lay, dl.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(dev.cpu().numpy(), model, "long ragged encode")
    # in-place reconstruct and recover of the damaged batch
    dmg = sh.copy()
    dmg[lost] = ERASED
    for slots in (0, m):
        img, data, par, out = make_arena("split", nb, k, m, slots, ss=L)
        data.view(img)[...] = np.where(v, dmg[:, :k], CANARY)
        par.view(img)[...] = np.where(v, dmg[:, k:], CANARY)
        model = img.copy()
        if slots == 0:
            write_outputs(data.view(model), lost[:, :k], sh[:, :k], lens)
        else:
            vals = np.zeros((nb, slots, L), dtype=np.uint8)
            sel = np.zeros((nb, slots), dtype=bool)
            for b in range(nb):
                idx = np.flatnonzero(lost[b, :k])
                vals[b, :idx.size] = sh[b, idx]
                sel[b, :idx.size] = True
            write_outputs(out.view(model), sel, vals, lens)
        dev = upload(torch, img)
        p = dev.data_ptr()
        lay = (p + data.off, data.bs, p + par.off, par.bs, L)
        st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
        if slots == 0:
            rc = codec.rs_reconstruct_ragged_raw(k, m, L, nb, *lay, dm.data_ptr(), dl.data_ptr(), st.data_ptr())
            st_want = np.zeros(nb, dtype=np.int32)
        else:
            rc = codec.rs_recover_ragged_raw(k, m, L, nb, *lay, dm.data_ptr(), dl.data_ptr(), p + out.off, out.bs,
                                             slots, st.data_ptr())
            st_want = lost[:, :k].sum(axis=1).astype(np.int32)
        assert rc == fec.FEC_OK and codec.lib_sync_rc() == fec.FEC_OK
        assert np.array_equal(st.cpu().numpy(), st_want)
        check_arena(dev.cpu().numpy(), model, "long ragged decode, %d slots" % slots)


def _all_calls(codec, fec, k, m, nb, p, data, par, out, dm, dl_ptr, st):
    lay = (p + data.off, data.bs, p + par.off, par.bs, S)
    return [codec.rs_encode_ragged_raw(k, m, MAXL, nb, *lay, dl_ptr, st.data_ptr()),
            codec.rs_reconstruct_ragged_raw(k, m, MAXL, nb, *lay, dm.data_ptr(), dl_ptr, st.data_ptr()),
            codec.rs_recover_ragged_raw(k, m, MAXL, nb, *lay, dm.data_ptr(), dl_ptr, p + out.off, out.bs, m,
                                        st.data_ptr())]


def test_misaligned_block_len_is_refused(codec, torch, fec):
    k, m, nb = 8, 4, 16
    img, data, par, out = make_arena("split", nb, k, m, m)
    dev = upload(torch, img)
    dl = torch.full((nb + 1,), MAXL, dtype=torch.int32, device="cuda")
    dm = torch.full((nb,), 0xFFE, dtype=torch.int32, device="cuda")
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    for off in (1, 2, 3):
        rcs = _all_calls(codec, fec, k, m, nb, dev.data_ptr(), data, par, out, dm, dl.data_ptr() + off, st)
        assert rcs == [fec.FEC_ERR_ALIGNMENT] * 3
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (dev.cpu().numpy() == CANARY).all() and (st.cpu().numpy() == 99).all()


def test_empty_batches_write_nothing(codec, torch, fec):
    k, m, nb = 8, 4, 37
    img, data, par, out = make_arena("split", nb, k, m, m)
    dev = upload(torch, img)
    dl = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    dm = torch.full((nb,), 0xFFE, dtype=torch.int32, device="cuda")   # data shard 0 lost: recoverable
    st = torch.full((nb,), 99, dtype=torch.int32, device="cuda")
    p = dev.data_ptr()
    # no blocks: nothing at all, the statuses included
    assert _all_calls(codec, fec, k, m, 0, p, data, par, out, dm, dl.data_ptr(), st) == [fec.FEC_OK] * 3
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (dev.cpu().numpy() == CANARY).all() and (st.cpu().numpy() == 99).all()
    # every block of length 0: no shard byte moves; the statuses are what the masks give
    lay = (p + data.off, data.bs, p + par.off, par.bs, S)
    assert codec.rs_encode_ragged_raw(k, m, MAXL, nb, *lay, dl.data_ptr(), st.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK and (st.cpu().numpy() == 0).all()
    st[:] = 99
    assert codec.rs_reconstruct_ragged_raw(k, m, MAXL, nb, *lay, dm.data_ptr(), dl.data_ptr(),
                                           st.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK and (st.cpu().numpy() == 0).all()
    assert codec.rs_recover_ragged_raw(k, m, MAXL, nb, *lay, dm.data_ptr(), dl.data_ptr(), p + out.off, out.bs, m,
                                       st.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK and (st.cpu().numpy() == 1).all()
    assert (dev.cpu().numpy() == CANARY).all()
