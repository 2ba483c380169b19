"""fec_rs_verify_batch (klauspost Encoder.Verify, batched) on the device, by the guarded-arena method
of test_gpu_layouts.py: every batch lives in one canary-filled arena with guards at both ends, shard
slots hold canary from L on, parity is made by fec_rs_encode_batch (its zero pad put back to canary),
single bits are flipped, and after each call the statuses and the count are compared with what the
flips must give and the WHOLE arena with its image before the call: verify writes nothing but the
status words and the count.

The statuses are reduced per block, not per wave or workgroup: 67 blocks of short shards put several
blocks into one wave, 70 000-byte shards spread one block over 18 workgroups, and the batch cut into
two launches puts one block alone into the second.
"""
import functools
import os
import re

import numpy as np
import pytest

from arena import CANARY, GUARD, STALE, check_arena, codec, encoded_arena, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENS = [1, 15, 16, 17, 33, 1202]
# (33,20): two parity row passes, (1,40): three; (32,0): nothing to compare
CODES = [(2, 1), (8, 4), (16, 8), (20, 10), (31, 1), (32, 0), (33, 20), (1, 40)]
LAYOUTS = ["interleaved", "split"]


class Batch:
    """An encoded batch in an arena on the host (img) with the calls to verify a flipped copy of it.
    build(layout, k, m, L, B, rng) makes the arena: encoded_arena by default, arena.oracle_arena for
    test_gpu_row_sweep.py."""

    def __init__(self, codec, fec, torch, layout, k, m, L, B, seed, build=None):
        self.codec, self.fec, self.torch = codec, fec, torch
        self.k, self.m, self.L, self.B = k, m, L, B
        build = build or functools.partial(encoded_arena, codec, fec, torch)
        img, self.data, self.par = build(layout, k, m, L, B, np.random.default_rng(seed))
        img.setflags(write=False)
        self.img = img

    def verify(self, flips, want_bad, count=True, what=""):
        """flips: (region 'd' / 'p', block, row, byte) whose bit 4 is flipped; want_bad: the blocks that
        must get status 0."""
        fec, torch = self.fec, self.torch
        img = self.img.copy()
        for reg, b, r, byte in flips:
            img[(self.data if reg == "d" else self.par).at(b, r) + byte] ^= 0x10
        dev = torch.from_numpy(img).cuda()
        p = dev.data_ptr()
        assert p % 16 == 0
        st = torch.full((self.B,), 99, dtype=torch.int32, device="cuda")
        cnt = torch.full((1,), STALE, dtype=torch.int32, device="cuda")   # a stale count is overwritten
        rc = fec.lib.fec_rs_verify_batch(self.codec.handle, self.k, self.m, self.L, self.B, p + self.data.off,
                                         self.data.bs, (p + self.par.off) if self.m else None, self.par.bs,
                                         self.data.ss, st.data_ptr(), cnt.data_ptr() if count else None,
                                         fec.FEC_DEVICE)
        assert rc == fec.FEC_OK, what
        assert self.codec.lib_sync_rc() == fec.FEC_OK, what     # a mismatch is a result, not an error
        want = np.ones(self.B, dtype=np.int32)
        want[sorted(want_bad)] = 0
        got = st.cpu().numpy()
        assert np.array_equal(got, want), "%s: statuses differ at blocks %s" % (what, np.flatnonzero(got != want))
        assert int(cnt.cpu().numpy()[0]) == (len(set(want_bad)) if count else STALE), what
        check_arena(dev.cpu().numpy(), img, what)


def run_cases(bt):
    k, m, L, B = bt.k, bt.m, bt.L, bt.B
    cps = (L + 15) // 16
    mid = min(L - 1, (cps // 2) * 16 + 3)
    bt.verify([], [], what="untouched")
    bt.verify([], [], count=False, what="untouched, no count")
    if m == 0:
        # no parity: nothing can mismatch
        bt.verify([("d", 3 % B, k - 1, 0)], [], what="m = 0, data flip")
        return
    b1, b2, b3 = 5 % B, (B - 1), 31 % B
    bt.verify([("d", b1, k - 1, 0)], [b1], what="byte 0 of a data shard")
    bt.verify([("p", b2, m - 1, L - 1)], [b2], what="byte L-1 of the last parity shard")
    bt.verify([("p", b3, 0, mid)], [b3], what="a middle chunk of parity row 0")
    bt.verify([("p", b3, 0, mid)], [b3], count=False, what="a mismatch, no count")
    if L % 16:
        bt.verify([("d", b1, 0, L), ("p", b1, m - 1, L), ("d", b2, k - 1, rup16(L) - 1), ("p", b3, 0, rup16(L) - 1)],
                  [], what="pad bytes of data and parity slots")
    if cps > 64:
        # the same lane of two waves of one block
        bt.verify([("p", b1, 0, 2 * 16 + 1), ("p", b1, 0, 66 * 16 + 1)], [b1], what="two flips 64 lanes apart")
    else:
        bt.verify([("p", b1, 0, 0), ("d", b1, 0, L - 1), ("p", b1, m - 1, mid)], [b1], what="three flips in one block")
    if B >= 67:
        # 0, 1, 65, 66 and every third block between: each neighbour of a bad block stays 1
        bad = sorted({0, 1, B - 2, B - 1} | set(range(4, B - 3, 3)))
        flips = [("p", b, (b * 7) % m, (b * 13) % L) if b % 2 else ("d", b, (b * 5) % k, (b * 11) % L) for b in bad]
        bt.verify(flips, bad, what="many bad blocks")


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_verify_statuses_and_count(codec, torch, fec, layout, k, m, L):
    run_cases(Batch(codec, fec, torch, layout, k, m, L, 67, 1000 * k + 10 * m + L))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_verify_widest_code(codec, torch, fec, layout):
    """RS(100,156): ten parity row passes, tables of a pass in LDS; 5 blocks of 33 bytes."""
    run_cases(Batch(codec, fec, torch, layout, 100, 156, 33, 5, 7))


@pytest.mark.parametrize("k,m", [(8, 4), (130, 20)])
def test_verify_block_spanning_workgroups(codec, torch, fec, k, m):
    """3 blocks of 70 000-byte shards (4375 chunks: a block spans 18 workgroups), a flip in the first
    chunk of one block and in the last chunk of another. (130,20): the tables of a row pass do not
    fit LDS and are read from memory."""
    bt = Batch(codec, fec, torch, "interleaved", k, m, 70000, 3, 11)
    bt.verify([], [], what="untouched")
    bt.verify([("d", 0, 1 % k, 5), ("p", 2, m - 1, 69999)], [0, 2], what="first chunk of block 0, last of block 2")
    bt.verify([("p", 1, 0, 16 * 300), ("p", 1, 0, 16 * 3000), ("d", 1, 0, 16 * 4000)], [1], what="one block, thrice")


def test_verify_batch_cut_into_two_launches(codec, torch, fec):
    """The smallest batch the encode's launch limit (fec_ctx.hpp kMaxItems chunks per launch) cuts in
    two: 2^31 / 4375 + 1 blocks of 70 000-byte shards, the last block alone in the second launch.
    Verify only reads its shards, so the blocks may overlap: RS(1,2) with both block strides 16 makes
    block b the window [16 b, 16 b + 70 000) of one data and one parity stream of 7.9 MB, and the
    parity stream is the encode of the data stream as one long shard. Chunk t of a stream then belongs
    to blocks t - 4374 .. t: a flip in the first chunk makes block 0 bad alone, in the last chunk the
    last block alone, and in chunk t = the second launch's first block, 4375 blocks across the cut,
    which the count must add up over both launches."""
    src = open(os.path.join(ROOT, "0xfec_amd", "csrc", "fec_ctx.hpp")).read()
    lim = re.search(r"kMaxItems\s*=\s*uint64_t\(1\)\s*<<\s*(\d+)\s*;", src)
    assert lim, "the encode's launch limit"
    max_items = 1 << int(lim.group(1))
    L = 70000
    cps = L // 16
    per_launch = max_items // cps
    B = per_launch + 1
    nchunks = B + cps - 1
    T = nchunks * 16
    h = codec.handle
    rng = np.random.default_rng(5)
    img = np.full(GUARD + T + GUARD + T + GUARD, CANARY, dtype=np.uint8)
    d_off, p_off = GUARD, GUARD + T + GUARD
    img[d_off:d_off + T] = rng.integers(0, 256, T, dtype=np.uint8)
    dev = torch.from_numpy(img).cuda()
    p = dev.data_ptr()
    assert fec.lib.fec_rs_encode_batch(h, 1, 1, T, 1, p + d_off, T, p + p_off, T, T, fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    img = dev.cpu().numpy()
    st = torch.empty((B,), dtype=torch.int32, device="cuda")
    cnt = torch.empty((1,), dtype=torch.int32, device="cuda")
    for what, chunks, bad_lo, bad_hi in [("clean", [], 0, 0), ("first and last chunk", [0, nchunks - 1], None, None),
                                         ("across the cut", [per_launch], per_launch - cps + 1, per_launch + 1)]:
        cur = img.copy()
        for t in chunks:
            cur[p_off + 16 * t + 7] ^= 0x10
        dev = torch.from_numpy(cur).cuda()
        p = dev.data_ptr()
        st.fill_(99)
        cnt.fill_(STALE)
        assert fec.lib.fec_rs_verify_batch(h, 1, 1, L, B, p + d_off, 16, p + p_off, 16, L, st.data_ptr(),
                                           cnt.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
        assert codec.lib_sync_rc() == fec.FEC_OK
        want = np.ones(B, dtype=np.int32)
        if bad_lo is None:
            want[0] = want[B - 1] = 0
        else:
            want[bad_lo:bad_hi] = 0
        got = st.cpu().numpy()
        assert np.array_equal(got, want), "%s: statuses differ at blocks %s" % (what, np.flatnonzero(got != want)[:8])
        assert int(cnt.cpu().numpy()[0]) == int((want == 0).sum()), what
        check_arena(dev.cpu().numpy(), cur, what)


def test_verify_codec_methods(codec, torch, fec):
    """Codec.rs_verify / rs_verify_split on [B, n, S] tensors, shard_len below the slot size."""
    k, m, S, L, B = 6, 3, 48, 41, 9
    sh = torch.randint(0, 256, (B, k + m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode(k, m, sh, shard_len=L)
    sh[4, k + 1, L - 1] ^= 1
    sh[2, 0, L] ^= 1          # pad byte of a data slot
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), STALE, dtype=torch.int32, device="cuda")
    assert codec.rs_verify(k, m, sh, st, cnt, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert st.cpu().tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1] and int(cnt.cpu()[0]) == 1
    data, par = sh[:, :k].contiguous(), sh[:, k:].contiguous()
    st.fill_(99)
    assert codec.rs_verify_split(k, m, data, par, st, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert st.cpu().tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    with pytest.raises(AssertionError):
        codec.rs_verify(k, m, sh.cpu(), st, shard_len=L)


def test_verify_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx, in order: nblocks == 0 touches nothing, then pointers, layouts, word
    alignment."""
    h, D = codec.handle, fec.FEC_DEVICE
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    st = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    p, s = buf.data_ptr(), st.data_ptr()
    V = fec.lib.fec_rs_verify_batch
    assert V(h, 2, 1, 16, 0, None, 0, None, 0, 16, None, None, D) == fec.FEC_OK
    assert V(h, 2, 1, 16, 2, None, 48, p + 32, 48, 16, s, None, D) == fec.FEC_ERR_INVALID_ARG
    assert V(h, 2, 1, 16, 2, p, 48, None, 48, 16, s, None, D) == fec.FEC_ERR_INVALID_ARG
    assert V(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, None, None, D) == fec.FEC_ERR_INVALID_ARG
    assert V(h, 2, 1, 16, 2, p + 8, 48, p + 32, 48, 16, s, None, D) == fec.FEC_ERR_ALIGNMENT
    assert V(h, 2, 1, 16, 2, p, 48, p + 32, 40, 16, s, None, D) == fec.FEC_ERR_ALIGNMENT
    assert V(h, 2, 1, 17, 2, p, 48, p + 32, 48, 16, s, None, D) == fec.FEC_ERR_INVALID_ARG   # stride < length
    assert V(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, s + 2, None, D) == fec.FEC_ERR_ALIGNMENT
    assert V(h, 2, 1, 16, 2, p, 48, p + 32, 48, 16, s, s + 6, D) == fec.FEC_ERR_ALIGNMENT
    # a pointer error comes before a layout error, a layout error before the word alignment
    assert V(h, 2, 1, 16, 2, p + 8, 48, p + 32, 48, 16, None, None, D) == fec.FEC_ERR_INVALID_ARG
    assert V(h, 2, 1, 17, 2, p, 48, p + 32, 48, 16, s + 2, None, D) == fec.FEC_ERR_INVALID_ARG
    assert V(h, 2, 0, 16, 2, p, 32, None, 0, 16, s, None, D) == fec.FEC_OK                     # m = 0: no parity
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and st.cpu().tolist() == [1, 1, 99, 99]
