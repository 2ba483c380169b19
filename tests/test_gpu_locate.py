"""fec_rs_locate_batch (which shard of a block that fails verify is the corrupt one) on the device, by
the guarded-arena method of test_gpu_verify.py: every batch lives in one canary-filled arena with
guards at both ends, shard slots hold canary from L on, parity is made by fec_rs_encode_batch (its
zero pad put back to canary), shards are corrupted in thirteen patterns spread over the blocks so
that neighbouring blocks carry different verdicts, the three outputs are pre-filled with a stale
value, and after each call the WHOLE arena is compared with its image before the call: locate writes
nothing but its outputs.

The expected verdicts come from a model of the definition written here in numpy: the syndromes are
the stored parity xor the ORACLE's encode of the stored data, products are the oracle's gf_mul, and a
block is clean if every syndrome is zero, else (m >= 2) it names the one shard s such that some
replacement of s alone explains every syndrome, else it is unknown. Every block is compared. Two
consequences are asserted without the model: one corrupt shard with m >= 2 is located, and t corrupt
shards with 2 <= t < m give unknown.
"""
import functools

import numpy as np
import pytest

from arena import CANARY, STALE, check_arena, codec, encoded_arena, gf, shards, torch  # noqa: F401

pytestmark = pytest.mark.gpu

CLEAN, UNKNOWN = -1, -2

LENS = [1, 15, 16, 17, 33, 1202]
# (31,1): every bad block unknown; (32,0): every block clean; (33,20): two passes; (1,40): three;
# (100,156): eleven passes, mask_words 8; (130,20): the tables of a pass do not fit LDS
CODES = [(1, 2), (2, 2), (8, 4), (20, 10), (31, 1), (32, 0), (33, 20), (1, 40), (100, 156), (254, 2), (130, 20)]
LAYOUTS = ["interleaved", "split"]
NPATTERNS = 13


def model_verdicts(oracle, gf, k, m, shards, L):
    """The definition, per block of shards [B, k + m, S] (bytes [0, L) count): the syndromes against
    the oracle's encode, then every shard that could explain them alone."""
    mul, inv = gf
    B = shards.shape[0]
    out = np.full(B, CLEAN, dtype=np.int32)
    if m == 0:
        return out
    want = np.ascontiguousarray(shards[:, :, :L]).copy()
    oracle.rs_encode(k, m, want)
    S = shards[:, k:, :L] ^ want[:, k:, :]                     # [B, m, L]
    P = oracle.build_matrix(k, k + m)[k:]                      # [m, k]
    for b in np.flatnonzero(S.reshape(B, -1).any(axis=1)):
        s = S[b]
        out[b] = UNKNOWN
        if m < 2:
            continue
        found = []
        rows = np.flatnonzero(s.any(axis=1))
        if rows.size == 1:
            found.append(k + int(rows[0]))
        # a data shard j explains the block iff S_r[x] == M[k+r][j] * e[x] with e = S_0 / M[k][j] in
        # every row and byte column; one nonzero column sieves the columns, the survivors get all of it
        x = int(np.flatnonzero(s.any(axis=0))[0])
        e = mul[inv[P[0]], s[0, x]]                            # [k]
        for j in np.flatnonzero((mul[P, e[None, :]] == s[:, x][:, None]).all(axis=0)):
            ej = mul[inv[P[0, j]], s[0]]                       # [L]
            if np.array_equal(mul[P[:, j][:, None], ej[None, :]], s):
                found.append(int(j))
        assert len(found) <= 1, "the code has distance m + 1 >= 3: at most one shard explains a block"
        if found:
            out[b] = found[0]
    return out


class Batch:
    """An encoded batch in an arena, corrupted per block by pattern, with the calls that locate it.
    build(layout, k, m, L, B, rng) makes the encoded arena: encoded_arena by default, arena.oracle_arena for
    test_gpu_row_sweep.py."""

    def __init__(self, codec, fec, torch, oracle, gf, layout, k, m, L, B, seed, patterns=None, build=None):
        self.codec, self.fec, self.torch, self.oracle, self.gf = codec, fec, torch, oracle, gf
        self.k, self.m, self.n, self.L, self.B = k, m, k + m, L, B
        self.rng = rng = np.random.default_rng(seed)
        build = build or functools.partial(encoded_arena, codec, fec, torch)
        img, self.data, self.par = build(layout, k, m, L, B, rng)
        self.clean = img.copy()
        self.clean.setflags(write=False)
        self.P = oracle.build_matrix(k, k + m)[k:] if m else None
        self.hit = [set() for _ in range(B)]      # the shards of each block with a changed byte in [0, L)
        self.img = img
        pats = patterns or [(b * 5 + 3) % NPATTERNS for b in range(B)]   # neighbours differ; each pattern >= 5 times
        for b, pat in enumerate(pats):
            self.corrupt(b, pat)
        self.img.setflags(write=False)
        self.want = model_verdicts(oracle, gf, k, m, self.shards(self.img), L)
        # what must hold without a model
        for b in range(B):
            t = len(self.hit[b])
            if m == 0 or t == 0:
                assert self.want[b] == CLEAN, (b, pats[b])
            elif t == 1 and m >= 2:
                assert self.want[b] == next(iter(self.hit[b])), (b, pats[b])
            elif (m == 1 and t == 1) or 2 <= t < m:
                assert self.want[b] == UNKNOWN, (b, pats[b])

    def shards(self, img):
        """[B, n, S] copy of the arena's slots."""
        return shards(img, self.data, self.par)

    def flip(self, b, s, x, v=None):
        """shard s of block b, byte x ^= v (nonzero); a parity shard the code does not have: nothing."""
        if s >= self.n:
            return
        v = int(self.rng.integers(1, 256)) if v is None else v
        assert v
        self.img[(self.data.at(b, s) if s < self.k else self.par.at(b, s - self.k)) + x] ^= v
        if x < self.L:
            self.hit[b].add(s)

    def corrupt(self, b, pat):
        k, m, n, L, rng = self.k, self.m, self.n, self.L, self.rng
        cps = (L + 15) // 16
        j1 = int(rng.integers(k))
        j2 = (j1 + 1 + int(rng.integers(k - 1))) % k if k > 1 else k     # (k = 1: parity shard 0)
        ca = int(rng.integers(cps))
        cb = (ca + 1 + int(rng.integers(cps - 1))) % cps if cps > 1 else ca

        def byte_in(c):   # a byte of chunk c below L
            return 16 * c + int(rng.integers(min(16, L - 16 * c)))
        xa, xb = byte_in(ca), byte_in(cb)
        late = k + (16 + int(rng.integers(m - 16)) if m > 16 else max(m - 1, 0))   # a parity row of a later pass
        if pat == 0:                                   # none
            pass
        elif pat == 1:                                 # one data shard, one bit
            self.flip(b, j1, xa, 1 << int(rng.integers(8)))
        elif pat == 2:                                 # one data shard, bytes in different chunks
            for x in {0, xa, xb, L - 1, (cps // 2) * 16}:
                self.flip(b, j1, x)
        elif pat == 3:                                 # one data shard, every byte
            for x in range(L) if L <= 1202 else range(0, L, 7):
                self.flip(b, j1, x)
        elif pat == 4:                                 # parity shard 0
            for x in {xa, xb}:
                self.flip(b, k, x)
        elif pat == 5:                                 # a parity shard of pass 0
            self.flip(b, k + int(rng.integers(min(m, 16))) if m else n, xa)
        elif pat == 6:                                 # a parity shard of a later pass only
            for x in {xa, L - 1}:
                self.flip(b, late, x)
        elif pat == 7:                                 # two shards, different columns of one chunk
            xc = 16 * ca + (xa - 16 * ca + 1) % min(16, L - 16 * ca)
            self.flip(b, j1, xa), self.flip(b, j2, xc)
        elif pat == 8:                                 # two shards, each chunk alone a single-shard error
            self.flip(b, j1, xa), self.flip(b, j2, xb)
        elif pat == 9:                                 # a data shard in one chunk, a parity shard in another
            self.flip(b, j1, xa), self.flip(b, k + int(rng.integers(m)) if m else n, xb)
        elif pat == 10:                                # every pass agrees on column j1, not on the error
            e, d = int(rng.integers(1, 256)), int(rng.integers(1, 256))
            self.flip(b, j1, xa, e)
            for i in range(16, m):                     # rows 16 ..: as if the error were e ^ d
                self.flip(b, k + i, xa, int(self.gf[0][self.P[i, j1], d]))
        elif pat == 11:                                # bytes at and past L only: clean
            for s in (j1, k, n - 1):
                self.flip(b, s, L), self.flip(b, s, self.data.ss - 1)
        elif pat == 12:                                # t shards, 2 <= t < m where the code has room
            t = int(rng.integers(2, m)) if m >= 3 else 2
            for s in rng.choice(n, size=min(t, n), replace=False):
                self.flip(b, int(s), xa if rng.integers(2) else xb)
        else:
            raise ValueError(pat)

    def upload(self, img=None):
        dev = self.torch.from_numpy(np.array(self.img if img is None else img)).cuda()   # (a writable copy)
        assert dev.data_ptr() % 16 == 0
        return dev

    def call(self, dev, bad, present, W, counts):
        fec, p = self.fec, dev.data_ptr()
        return fec.lib.fec_rs_locate_batch(self.codec.handle, self.k, self.m, self.L, self.B, p + self.data.off,
                                           self.data.bs, (p + self.par.off) if self.m else None, self.par.bs,
                                           self.data.ss, bad.data_ptr(), None if present is None else present.data_ptr(),
                                           W, None if counts is None else counts.data_ptr(), fec.FEC_DEVICE)

    def want_present(self, verdicts, W):
        bits = np.zeros((self.B, 32 * W), dtype=np.uint8)
        bits[:, :self.n] = 1
        loc = np.flatnonzero(verdicts >= 0)
        bits[loc, verdicts[loc]] = 0
        return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(self.B, W)

    def locate(self, dev, W, present=True, counts=True, want=None, what=""):
        """One call on the arena dev: verdicts, masks and counts against `want` (default: the model's),
        the arena against its image before the call. Returns (verdicts, present_out tensor)."""
        fec, torch = self.fec, self.torch
        want = self.want if want is None else want
        before = dev.cpu().numpy()
        bad = torch.full((self.B,), 99, dtype=torch.int32, device="cuda")
        pm = torch.full((self.B, W), STALE, dtype=torch.int32, device="cuda") if present else None
        cnt = torch.full((2,), STALE, dtype=torch.int32, device="cuda") if counts else None
        assert self.call(dev, bad, pm, W, cnt) == fec.FEC_OK, what
        assert self.codec.lib_sync_rc() == fec.FEC_OK, what          # a corrupt block is a result, not an error
        got = bad.cpu().numpy()
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, "%s: verdicts differ at blocks %s: got %s, want %s" % (what, diff[:8], got[diff[:8]],
                                                                                     want[diff[:8]])
        if counts:
            assert cnt.cpu().numpy().tolist() == [int((got >= 0).sum()), int((got == UNKNOWN).sum())], what
        if present:
            assert np.array_equal(pm.cpu().numpy().view(np.uint32), self.want_present(want, W)), what
        check_arena(dev.cpu().numpy(), before, what)
        return got, pm

    def run(self):
        fec = self.fec
        Wmin = fec.mask_words(self.n)
        dev = self.upload()
        self.locate(dev, Wmin, what="minimum mask words")
        self.locate(dev, 8, counts=False, what="8 mask words, no counts")
        self.locate(dev, Wmin, present=False, what="no masks")
        self.locate(dev, Wmin, present=False, counts=False, what="verdicts alone")
        clean = self.upload(self.clean)
        self.locate(clean, Wmin, want=np.full(self.B, CLEAN, dtype=np.int32), what="clean batch")
        if self.n <= 32:
            self.heal(dev)

    def heal(self, dev):
        """locate -> reconstruct-some with present_out as its masks: every located block with one corrupt
        shard holds its original bytes again (with as many corrupt shards as parity rows or more, the
        shard named may be a wrong one), and a second locate calls every located block clean and leaves
        the unknown ones unknown."""
        fec, p = self.fec, dev.data_ptr()
        got, pm = self.locate(dev, 1, what="heal: locate")
        rc = fec.lib.fec_rs_reconstruct_some_batch(self.codec.handle, self.k, self.m, self.L, self.B,
                                                   p + self.data.off, self.data.bs,
                                                   (p + self.par.off) if self.m else None, self.par.bs, self.data.ss,
                                                   pm.data_ptr(), None, None, fec.FEC_DEVICE)
        assert rc == fec.FEC_OK and self.codec.lib_sync_rc() == fec.FEC_OK
        healed = self.shards(dev.cpu().numpy())[:, :, :self.L]
        orig = self.shards(self.clean)[:, :, :self.L]
        loc = got >= 0
        one = loc & (np.array([len(h) for h in self.hit]) == 1)
        assert one.any() or self.m < 2
        assert np.array_equal(healed[one], orig[one]), "located blocks hold their original bytes"
        assert np.array_equal(healed[~loc], self.shards(self.img)[:, :, :self.L][~loc]), "the others are untouched"
        self.locate(dev, 1, want=np.where(loc, CLEAN, got).astype(np.int32), what="heal: second locate")


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_locate_verdicts_masks_and_counts(codec, torch, fec, oracle, gf, layout, k, m, L):
    Batch(codec, fec, torch, oracle, gf, layout, k, m, L, 67, 1000 * k + 10 * m + L).run()


@pytest.mark.parametrize("k,m,B", [(8, 4, 13), (130, 20, 3)])
def test_locate_block_spanning_workgroups(codec, torch, fec, oracle, gf, k, m, B):
    """70 000-byte shards (4375 chunks: a block spans 18 workgroups), so the proposals of one block
    meet in its word from many workgroups. (130,20): two passes, neither's tables fit LDS."""
    pats = list(range(NPATTERNS)) if B == 13 else [2, 8, 10]
    Batch(codec, fec, torch, oracle, gf, "interleaved", k, m, 70000, B, 17 + k, patterns=pats).run()


def test_locate_codec_methods_and_heal_loop(codec, torch, fec):
    """Codec.rs_locate / rs_locate_split on [B, n, S] tensors, shard_len below the slot size, then
    Codec.rs_reconstruct_some with the masks locate wrote."""
    k, m, S, L, B = 6, 3, 48, 41, 9
    sh = torch.randint(0, 256, (B, k + m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode(k, m, sh, shard_len=L)
    truth = sh.clone()
    sh[4, k + 1, L - 1] ^= 1          # a parity shard
    sh[6, 2, 0] ^= 0x80               # a data shard
    sh[6, 2, 40] ^= 0x01
    sh[7, 0, 5] ^= 3                  # two data shards: 2 <= t < m
    sh[7, 5, 20] ^= 9
    sh[2, 0, L] ^= 1                  # pad byte of a data slot
    want = [CLEAN, CLEAN, CLEAN, CLEAN, k + 1, CLEAN, 2, UNKNOWN, CLEAN]
    bad = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    pm = torch.full((B, 1), STALE, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), STALE, dtype=torch.int32, device="cuda")
    assert codec.rs_locate(k, m, sh, bad, pm, cnt, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == want and cnt.cpu().tolist() == [2, 1]
    full = (1 << (k + m)) - 1
    assert pm.cpu().flatten().tolist() == [full & ~(1 << v) if v >= 0 else full for v in want]
    data, par = sh[:, :k].contiguous(), sh[:, k:].contiguous()
    bad.fill_(99)
    assert codec.rs_locate_split(k, m, data, par, bad, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == want
    codec.rs_reconstruct_some(k, m, sh, pm.flatten(), shard_len=L)
    codec.sync()
    ok = [b for b in range(B) if want[b] != UNKNOWN]
    assert torch.equal(sh[ok][:, :, :L], truth[ok][:, :, :L])
    assert codec.rs_locate(k, m, sh, bad, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == [CLEAN if v != UNKNOWN else UNKNOWN for v in want]
    with pytest.raises(AssertionError):
        codec.rs_locate(k, m, sh.cpu(), bad, shard_len=L)


def test_locate_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx, in order: nblocks == 0 touches nothing, then pointers, layouts, the
    alignment of the three word arrays; None for either optional output works."""
    h, D = codec.handle, fec.FEC_DEVICE
    INV, ALIGN = fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_ALIGNMENT
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 99, dtype=torch.int32, device="cuda")
    p, s = buf.data_ptr(), out.data_ptr()
    pm, cn = s + 16, s + 32

    def F(k, m, L, B, data, dbs, par, pbs, ss, bad, present=None, W=1, counts=None):
        return fec.lib.fec_rs_locate_batch(h, k, m, L, B, data, dbs, par, pbs, ss, bad, present, W, counts, D)
    assert F(2, 2, 16, 0, None, 0, None, 0, 16, None) == fec.FEC_OK
    assert F(2, 2, 16, 2, None, 64, p + 32, 64, 16, s) == INV
    assert F(2, 2, 16, 2, p, 64, None, 64, 16, s) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, None) == INV
    assert F(2, 2, 16, 2, p + 8, 64, p + 32, 64, 16, s) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 56, 16, s) == ALIGN
    assert F(2, 2, 17, 2, p, 64, p + 32, 64, 16, s) == INV          # stride < length
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s + 2) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, pm + 1) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, pm, 1, cn + 2) == ALIGN
    # mask_words is checked with no present_out, before the ctx's work
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, None, 0) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, None, 9) == INV
    # a pointer error comes before a layout error, a layout error before the word alignment
    assert F(2, 2, 16, 2, p + 8, 64, p + 32, 64, 16, None) == INV
    assert F(2, 2, 17, 2, p, 64, p + 32, 64, 16, s + 2) == INV
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and (out.cpu().numpy() == 99).all()
    # m = 0: no parity, every block clean; both optional outputs
    assert F(2, 0, 16, 2, p, 32, None, 0, 16, s, pm, 2, cn) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    got = out.cpu().numpy()
    assert got[:2].tolist() == [CLEAN, CLEAN] and got[4:8].tolist() == [3, 0, 3, 0] and got[8:10].tolist() == [0, 0]
    assert (got[[2, 3, 10, 11]] == 99).all() and (buf.cpu().numpy() == CANARY).all()
