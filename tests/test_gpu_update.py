"""fec_rs_update_batch and fec_rs_encode_idx_batch (klauspost Update, EncodeIdx) on the device, by the
guarded-arena method of test_gpu_verify.py: every batch lives in one canary-filled arena with guards
at both ends; old data, new data and parity slots have slack and the block strides gaps; parity
slots start as random bytes P0 over [0, L) and canary from L on; every old and new slot, masked or
not, holds independent random bytes over [0, L) and canary from L on, so a column folded by mistake,
or a pad byte folded in, changes the result.

The model: for a block with a non-empty mask, bytes [0, L) of the parity slots become
P0 ^ oracle.rs_encode(k, m, D), where D holds old ^ new (update) or data (encode-idx) in the masked
columns and zeros elsewhere, and bytes [L, round_up(L, 16)) become zeros; every other byte of the
arena is unchanged. After each call the WHOLE arena is compared with the model and fec_sync() must
return FEC_OK.

67 blocks of short shards put many blocks with different masks into one wave (masks by per-lane
loads); shards of 497 bytes and more put at most 3 blocks into a wave (masks by scalar loads).
"""
import numpy as np
import pytest

from arena import CANARY, Region, canary_image, check_arena, codec, folded_parity, place, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 17, 33, 1202]
# (33,20): two parity row passes and two mask words; (32,0): nothing to write
CODES = [(2, 1), (8, 4), (20, 10), (31, 1), (33, 20), (32, 0)]
LAYOUTS = ["interleaved", "split"]


def make_layout(name, k, m, L, B):
    """(arena image, old data region, new data region, parity region): the old data and the parity as
    the layout places data and parity, the new data apart, above both."""
    old, par = place(name, k, m, L, B)
    ss = old.ss
    if name == "interleaved":   # old data and parity in one [B][k+m] region
        new = Region(max(old.end(), par.end()) + 96, k * ss + 16, ss, k, B)
    else:                       # three regions, parity lowest
        new = Region(old.end() + 32, k * ss + 32, ss, k, B)
    return canary_image([old, new, par]), old, new, par


def pack_masks(fec, cols, W, stray=False):
    """bool [B, k] -> uint32 [B, W]; stray: every bit at and above k set as well."""
    B, k = cols.shape
    bits = np.zeros((B, 32 * W), dtype=bool)
    bits[:, :k] = cols
    if stray:
        bits[:, k:] = True
    out = fec.wide_masks(bits)
    assert out.shape == (B, W)
    return out


class Batch:
    """Old data, new data and parity of B blocks in an arena: the image on the host (img, read-only)
    and on the device (dev), and the two calls on a fresh device copy with the whole-arena check."""

    def __init__(self, codec, fec, torch, oracle, layout, k, m, L, B, seed, zero_parity=False):
        self.codec, self.fec, self.torch, self.oracle = codec, fec, torch, oracle
        self.k, self.m, self.L, self.B = k, m, L, B
        img, self.old, self.new, self.par = make_layout(layout, k, m, L, B)
        rng = np.random.default_rng(seed)
        self.old.view(img, 0, L)[...] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        self.new.view(img, 0, L)[...] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        if zero_parity:
            self.par.view(img, 0, rup16(L))[...] = 0
        else:
            self.par.view(img, 0, L)[...] = rng.integers(0, 256, (B, m, L), dtype=np.uint8)
        img.setflags(write=False)
        self.img = img
        self.dev = torch.from_numpy(img.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def model(self, cols, has_old, img=None):
        """The arena after a call with column sets cols (bool [B, k])."""
        k, m, L, B = self.k, self.m, self.L, self.B
        out = (self.img if img is None else img).copy()
        if m == 0:
            return out
        d = self.new.view(out, 0, L) ^ self.old.view(out, 0, L) if has_old else self.old.view(out, 0, L)
        p = self.par.view(out, 0, L)
        p[...] = folded_parity(self.oracle, k, m, d, cols, p)
        pad = self.par.view(out, L, rup16(L))
        pad[cols.any(axis=1)] = 0
        return out

    def run(self, dev, call, words):
        """One call in place on the device arena `dev`; encode-idx folds the old region's slots."""
        fec, p = self.fec, dev.data_ptr()
        mk = self.torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()
        par = (p + self.par.off) if self.m else None
        W = words.shape[1]
        if call == "update":
            rc = fec.lib.fec_rs_update_batch(self.codec.handle, self.k, self.m, self.L, self.B, p + self.old.off,
                                             self.old.bs, p + self.new.off, self.new.bs, par, self.par.bs,
                                             self.old.ss, mk.data_ptr(), W, fec.FEC_DEVICE)
        else:
            rc = fec.lib.fec_rs_encode_idx_batch(self.codec.handle, self.k, self.m, self.L, self.B, p + self.old.off,
                                                 self.old.bs, par, self.par.bs, self.old.ss, mk.data_ptr(), W,
                                                 fec.FEC_DEVICE)
        assert rc == fec.FEC_OK, (call, rc)
        assert self.codec.lib_sync_rc() == fec.FEC_OK, call

    def check(self, call, cols, W, stray=False, what=""):
        dev = self.dev.clone()
        self.run(dev, call, pack_masks(self.fec, cols, W, stray))
        check_arena(dev.cpu().numpy(), self.model(cols, call == "update"), "%s, %s, %d mask words" % (what, call, W))


def mask_kinds(k, B, seed):
    """(name, bool [B, k], stray bits) for one batch."""
    rng = np.random.default_rng(seed)
    empty = np.zeros((B, k), dtype=bool)
    ends = empty.copy()
    ends[0::2, 0] = True
    ends[1::2, k - 1] = True
    rnd = rng.integers(0, 2, (B, k)).astype(bool)
    # popcounts 0, k, 1, 0, k, 1 ...: lanes of one wave with different trip counts, and empty blocks
    # between full ones
    steps = empty.copy()
    steps[1::3] = True
    ones = np.arange(2, B, 3)
    steps[ones, (ones * 5) % k] = True
    return [("all empty", empty, False), ("first / last column", ends, False), ("all k", ~empty, False),
            ("random", rnd, False), ("random, stray bits at and above k", rng.integers(0, 2, (B, k)).astype(bool), True),
            ("popcounts 0, k, 1 ...", steps, False)]


def run_cases(bt):
    Wmin = bt.fec.mask_words(bt.k)
    for name, cols, stray in mask_kinds(bt.k, bt.B, bt.k * 131 + bt.L):
        bt.check("encode_idx", cols, Wmin, stray, name)
        bt.check("update", cols, Wmin, stray, name)
        bt.check("update", cols, 8, stray, name)


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_update_and_encode_idx(codec, torch, fec, oracle, layout, k, m, L):
    run_cases(Batch(codec, fec, torch, oracle, layout, k, m, L, 67, 1000 * k + 10 * m + L))


@pytest.mark.parametrize("L", [496, 497, 520])
@pytest.mark.parametrize("k,m", [(8, 4), (33, 4)])
def test_mask_load_regimes(codec, torch, fec, oracle, k, m, L):
    """31 chunks per shard: the masks come by per-lane loads; 32: by scalar loads, two blocks per wave;
    33: by scalar loads, up to three blocks per wave."""
    run_cases(Batch(codec, fec, torch, oracle, "split", k, m, L, 7, k + L))


@pytest.mark.parametrize("k,m,L", [(2, 1, 1), (8, 4, 1202), (20, 10, 33), (33, 20, 17)])
def test_full_mask_on_zeroed_parity_is_the_encode(codec, torch, fec, oracle, k, m, L):
    bt = Batch(codec, fec, torch, oracle, "interleaved", k, m, L, 67, 3 * k + L, zero_parity=True)
    enc, idx = bt.dev.clone(), bt.dev.clone()
    p = enc.data_ptr()
    assert fec.lib.fec_rs_encode_batch(codec.handle, k, m, L, bt.B, p + bt.old.off, bt.old.bs, p + bt.par.off,
                                       bt.par.bs, bt.old.ss, fec.FEC_DEVICE) == fec.FEC_OK
    bt.run(idx, "encode_idx", pack_masks(fec, np.ones((bt.B, k), dtype=bool), fec.mask_words(k)))
    assert codec.lib_sync_rc() == fec.FEC_OK
    got = idx.cpu().numpy()
    check_arena(got, enc.cpu().numpy(), "encode-idx of every column against the encode")
    assert not np.array_equal(got, bt.img)


@pytest.mark.parametrize("call", ["update", "encode_idx"])
@pytest.mark.parametrize("k,m,L", [(8, 4, 33), (33, 20, 1202)])
def test_two_calls_with_complementary_masks_equal_one(codec, torch, fec, oracle, call, k, m, L):
    bt = Batch(codec, fec, torch, oracle, "split", k, m, L, 67, 7 * k + L)
    rng = np.random.default_rng(k)
    union = rng.integers(0, 4, (bt.B, k)) > 0
    part = union & rng.integers(0, 2, (bt.B, k)).astype(bool)
    W = fec.mask_words(k)
    one, two = bt.dev.clone(), bt.dev.clone()
    bt.run(one, call, pack_masks(fec, union, W))
    bt.run(two, call, pack_masks(fec, part, W))
    bt.run(two, call, pack_masks(fec, union & ~part, W))
    got = two.cpu().numpy()
    check_arena(got, one.cpu().numpy(), "two calls against one")
    check_arena(got, bt.model(union, call == "update"), "two calls against the model")


@pytest.mark.parametrize("k,m,L", [(8, 4, 1202), (20, 10, 17), (33, 20, 33)])
def test_update_is_the_encode_of_the_merged_data(codec, torch, fec, oracle, k, m, L):
    """Parity encoded from the old data on the device, updated for the changed columns, against the
    device encode of the merged data (new in the changed columns, old elsewhere)."""
    bt = Batch(codec, fec, torch, oracle, "split", k, m, L, 67, 11 * k + L)
    h, D, B = codec.handle, fec.FEC_DEVICE, bt.B
    cols = np.random.default_rng(L).integers(0, 3, (B, k)) == 0
    upd = bt.dev.clone()
    p = upd.data_ptr()
    assert fec.lib.fec_rs_encode_batch(h, k, m, L, B, p + bt.old.off, bt.old.bs, p + bt.par.off, bt.par.bs,
                                       bt.old.ss, D) == fec.FEC_OK
    bt.run(upd, "update", pack_masks(fec, cols, fec.mask_words(k)))
    merged = bt.img.copy()
    o, n = bt.old.view(merged, 0, L), bt.new.view(merged, 0, L)
    o[...] = np.where(cols[:, :, None], n, o)
    ref = torch.from_numpy(merged).cuda()
    p = ref.data_ptr()
    assert fec.lib.fec_rs_encode_batch(h, k, m, L, B, p + bt.old.off, bt.old.bs, p + bt.par.off, bt.par.bs,
                                       bt.old.ss, D) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    got, want = upd.cpu().numpy(), ref.cpu().numpy()
    R = rup16(L)
    assert np.array_equal(bt.par.view(got, 0, R), bt.par.view(want, 0, R))
    # and nothing but the parity changed: the update did not copy new over old
    bt.par.view(got, 0, R)[...] = bt.par.view(bt.img, 0, R)
    check_arena(got, bt.img, "outside the parity slots")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_widest_code(codec, torch, fec, oracle, layout):
    """RS(100,156): ten parity row passes, tables of a pass in LDS, masks of 4 words; 5 blocks of 33 bytes."""
    bt = Batch(codec, fec, torch, oracle, layout, 100, 156, 33, 5, 7)
    assert fec.mask_words(bt.k) == 4
    run_cases(bt)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tables_from_memory_and_a_bit_in_the_fifth_word(codec, torch, fec, oracle, layout):
    """RS(130,20): the tables of a row pass do not fit LDS; masks of 5 words; 3 blocks of 33 bytes."""
    bt = Batch(codec, fec, torch, oracle, layout, 130, 20, 33, 3, 9)
    assert fec.mask_words(bt.k) == 5
    run_cases(bt)
    cols = np.zeros((3, 130), dtype=bool)
    cols[0, 129] = cols[2, 128] = cols[2, 3] = True
    for call in ("update", "encode_idx"):
        bt.check(call, cols, 5, what="columns 128 and 129")


@pytest.mark.parametrize("k,m", [(8, 4), (130, 20)])
def test_block_spanning_workgroups(codec, torch, fec, oracle, k, m):
    """3 blocks of 70 000-byte shards (4375 chunks: a block spans 18 workgroups, the masks may go by
    scalar loads); block 1's mask is empty."""
    bt = Batch(codec, fec, torch, oracle, "interleaved", k, m, 70000, 3, 11)
    cols = np.random.default_rng(k).integers(0, 2, (3, k)).astype(bool)
    cols[0, k - 1] = cols[2, 0] = True
    cols[1] = False
    W = fec.mask_words(k)
    bt.check("update", cols, W, what="long shards")
    bt.check("encode_idx", cols, W, stray=True, what="long shards")


def test_codec_methods(codec, torch, fec, oracle):
    """Codec.rs_update / rs_encode_idx and their split forms on [B, n, S] tensors, shard_len below S."""
    k, m, S, L, B = 6, 3, 48, 41, 9
    rng = np.random.default_rng(2)
    sh = rng.integers(0, 256, (B, k + m, S), dtype=np.uint8)
    new = rng.integers(0, 256, (B, k, S), dtype=np.uint8)
    cols = rng.integers(0, 2, (B, k)).astype(bool)
    cols[3] = False

    def want(delta):
        D = np.zeros((B, k + m, L), dtype=np.uint8)
        D[:, :k] = delta[:, :, :L] * cols[:, :, None]
        oracle.rs_encode(k, m, D)
        out = sh.copy()
        hit = cols.any(axis=1)
        out[hit, k:, :L] ^= D[hit, k:]
        out[hit, k:, L:rup16(L)] = 0
        return out

    masks = torch.from_numpy(pack_masks(fec, cols, 1).view(np.int32)).cuda()
    new_d = torch.from_numpy(new).cuda()
    for name, delta in (("update", sh[:, :k] ^ new), ("encode_idx", sh[:, :k])):
        a, b = torch.from_numpy(sh).cuda(), torch.from_numpy(sh).cuda()
        data, par = b[:, :k].contiguous(), b[:, k:].contiguous()
        if name == "update":
            assert codec.rs_update(k, m, a, new_d, masks, shard_len=L) == fec.FEC_OK
            assert codec.rs_update_split(k, m, data, new_d, par, masks, shard_len=L) == fec.FEC_OK
        else:
            assert codec.rs_encode_idx(k, m, a, masks, shard_len=L) == fec.FEC_OK
            assert codec.rs_encode_idx_split(k, m, data, par, masks, shard_len=L) == fec.FEC_OK
        codec.sync()
        w = want(delta)
        assert np.array_equal(a.cpu().numpy(), w), name
        assert np.array_equal(par.cpu().numpy(), w[:, k:]), name + " split"
        assert np.array_equal(data.cpu().numpy(), sh[:, :k]) and np.array_equal(new_d.cpu().numpy(), new)
    with pytest.raises(AssertionError):
        codec.rs_encode_idx(k, m, torch.from_numpy(sh), masks, shard_len=L)
    with pytest.raises(AssertionError):
        codec.rs_update(k, m, torch.from_numpy(sh).cuda(), new_d, masks.cpu(), shard_len=L)


def test_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx, in order: nblocks == 0 and m == 0 touch nothing, then pointers, layouts,
    the mask's alignment."""
    h, D = codec.handle, fec.FEC_DEVICE
    INV, ALIGN, OK = fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_ALIGNMENT, fec.FEC_OK
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    mk = torch.full((4,), 3, dtype=torch.int32, device="cuda")
    p, s = buf.data_ptr(), mk.data_ptr()
    old, new, par = p, p + 1024, p + 2048
    U = fec.lib.fec_rs_update_batch
    E = fec.lib.fec_rs_encode_idx_batch

    def u(nb=2, m=1, L=16, o=old, obs=32, n=new, nbs=32, q=par, pbs=16, ss=16, mask=s, W=1):
        return U(h, 2, m, L, nb, o, obs, n, nbs, q, pbs, ss, mask, W, D)

    def e(nb=2, m=1, L=16, d=old, dbs=32, q=par, pbs=16, ss=16, mask=s, W=1):
        return E(h, 2, m, L, nb, d, dbs, q, pbs, ss, mask, W, D)

    assert U(h, 2, 1, 16, 0, None, 0, None, 0, None, 0, 16, None, 1, D) == OK
    assert E(h, 2, 1, 16, 0, None, 0, None, 0, 16, None, 1, D) == OK
    for call in (u, e):
        assert call(mask=None) == INV
        assert call(q=None) == INV
        assert call(q=par + 8) == ALIGN
        assert call(pbs=24) == ALIGN
        assert call(ss=24) == ALIGN
        assert call(L=17) == INV                      # stride < length
        assert call(mask=s + 2) == ALIGN
        # a pointer error comes before a layout error, a layout error before the mask's alignment
        assert call(mask=None, q=par + 8) == INV
        assert call(L=17, mask=s + 2) == INV
        assert call(m=0, q=None) == OK                # m = 0: no parity
        assert call(m=0, q=None, mask=None) == OK     # and nothing else is looked at
    assert u(o=None) == INV and u(n=None) == INV and e(d=None) == INV
    assert u(o=old + 8) == ALIGN and u(n=new + 8) == ALIGN and e(d=old + 8) == ALIGN
    assert u(obs=40) == ALIGN and u(nbs=40) == ALIGN and e(dbs=40) == ALIGN
    assert u(o=None, n=new + 8) == INV
    assert codec.lib_sync_rc() == OK
    assert (buf.cpu().numpy() == CANARY).all() and mk.cpu().tolist() == [3, 3, 3, 3]
