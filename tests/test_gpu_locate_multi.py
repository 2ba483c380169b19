"""fec_rs_locate_multi_batch (up to m/2 corrupt shards of a block that fails verify) on the device, by
the guarded-arena method of test_gpu_locate.py: every batch lives in one canary-filled arena with
guards at both ends, shard slots hold canary from L on, parity is made by fec_rs_encode_batch (its
zero pad put back to canary), shards are corrupted in fourteen patterns spread over the blocks so
that neighbouring blocks differ, the three outputs are pre-filled with a stale value, and after each
call the WHOLE arena is compared with its image before the call: the call writes nothing but its
outputs.

The expected results come from a model written here in numpy with the ORACLE's gf_mul and
build_matrix. With T = min(max_bad, m // 2):
  - codes of n = k + m <= 12: the definition by brute force. The syndromes are the stored parity xor
    the oracle's encode of the stored data; every set of at most T shards is tried in ascending size,
    and a set explains the block if every syndrome column lies in the span of its columns of [P | I]
    (tested with a basis of the left null space of those columns). The patterns reach any number of
    corrupt shards up to n.
  - larger codes: the patterns keep the number t of corrupt shards at or below m - T, so the theorem
    gives the expectation: exactly the corrupt shards for t <= T, unknown above.
Every block is compared; the theorem's two consequences are asserted for the small codes as well.
"""
import functools
import itertools

import numpy as np
import pytest

from arena import CANARY, STALE, check_arena, codec, encoded_arena, gf, shards, torch  # noqa: F401

pytestmark = pytest.mark.gpu

UNKNOWN = -2
MAX_BAD = 8

LENS = [1, 15, 16, 17, 33, 1202]
# (31,1): every bad block unknown; (32,0): every block 0; (4,16): 16 rows, T = 8; (240,16): 8 mask words,
# the tables do not fit LDS
CODES = [(1, 2), (2, 2), (6, 3), (8, 4), (20, 10), (4, 16), (240, 16), (31, 1), (32, 0)]
LAYOUTS = ["interleaved", "split"]
NPATTERNS = 14
BRUTE_N = 12


_NULL = {}


def left_null(gf, H, key):
    """A basis N (rows) of {y : y H = 0} for the m x v matrix H over the field, by reducing [H | I]."""
    if key in _NULL:
        return _NULL[key]
    mul, inv = gf
    m, v = H.shape
    G = np.concatenate([H, np.eye(m, dtype=np.uint8)], axis=1)
    row = 0
    for j in range(v):
        p = next((i for i in range(row, m) if G[i, j]), None)
        if p is None:
            continue
        G[[row, p]] = G[[p, row]]
        G[row] = mul[inv[G[row, j]], G[row]]
        for i in range(m):
            if i != row and G[i, j]:
                G[i] ^= mul[G[i, j], G[row]]
        row += 1
    N = G[row:, v:].copy()
    assert not np.bitwise_xor.reduce(mul[N[:, :, None], H[None, :, :]], axis=1).any()
    _NULL[key] = N
    return N


def model_brute(oracle, gf, k, m, T, shards, L):
    """The definition, per block of shards [B, n, S]: (counts [B], sets [B] of frozensets)."""
    mul, _ = gf
    B, n = shards.shape[0], k + m
    counts = np.zeros(B, dtype=np.int32)
    sets = [frozenset()] * B
    if m == 0:
        return counts, sets
    want = np.ascontiguousarray(shards[:, :, :L]).copy()
    oracle.rs_encode(k, m, want)
    S = shards[:, k:, :L] ^ want[:, k:, :]                     # [B, m, L]
    P = oracle.build_matrix(k, k + m)[k:]                      # [m, k]
    H = np.concatenate([P, np.eye(m, dtype=np.uint8)], axis=1)  # [m, n]
    code = P.tobytes()                                         # the cache of null spaces is per matrix
    for b in np.flatnonzero(S.reshape(B, -1).any(axis=1)):
        cols = np.unique(S[b][:, S[b].any(axis=0)], axis=1)    # the distinct nonzero syndrome columns
        counts[b] = UNKNOWN
        for v in range(1, T + 1):
            found = []
            for E in itertools.combinations(range(n), v):
                N = left_null(gf, H[:, list(E)], (k, m, E, code))
                if not np.bitwise_xor.reduce(mul[N[:, :, None], cols[None, :, :]], axis=1).any():
                    found.append(E)
            assert len(found) <= 1, "distance m + 1 > 2 T: at most one smallest set explains a block"
            if found:
                counts[b], sets[b] = v, frozenset(found[0])
                break
    return counts, sets


class Batch:
    """An encoded batch in an arena, corrupted per block by pattern, with the calls that locate it.
    build(layout, k, m, L, B, rng) makes the encoded arena: encoded_arena by default, arena.oracle_arena for
    test_gpu_row_sweep.py."""

    def __init__(self, codec, fec, torch, oracle, gf, layout, k, m, L, B, seed, max_bad=MAX_BAD, patterns=None,
                 build=None):
        self.codec, self.fec, self.torch, self.oracle, self.gf = codec, fec, torch, oracle, gf
        self.k, self.m, self.n, self.L, self.B = k, m, k + m, L, B
        self.max_bad = max_bad
        self.T = T = min(max_bad, m // 2)
        self.brute = self.n <= BRUTE_N
        # larger codes: at most m - T corrupt shards per block (m = 0: nothing can be inconsistent)
        self.cap = self.n if self.brute or m == 0 else m - T
        self.rng = rng = np.random.default_rng(seed)
        build = build or functools.partial(encoded_arena, codec, fec, torch)
        img, self.data, self.par = build(layout, k, m, L, B, rng)
        self.clean = img.copy()
        self.clean.setflags(write=False)
        self.hit = [set() for _ in range(B)]      # the shards of each block with a changed byte in [0, L)
        self.flipped = set()
        self.img = img
        pats = patterns or [(b * 5 + 3) % NPATTERNS for b in range(B)]   # neighbours differ; each pattern >= 4 times
        for b, pat in enumerate(pats):
            self.corrupt(b, pat)
        self.img.setflags(write=False)
        # the expectation
        t = np.array([len(h) for h in self.hit])
        if self.brute:
            self.want, self.sets = model_brute(oracle, gf, k, m, T, self.shards(self.img), L)
        else:
            assert (t <= self.cap).all()
            self.want = np.where(t <= T, t, UNKNOWN).astype(np.int32) if m else np.zeros(B, dtype=np.int32)
            self.sets = [frozenset(h) if len(h) <= T else frozenset() for h in self.hit]
        # what must hold whatever the model
        for b in range(B):
            if m == 0 or t[b] == 0:
                assert self.want[b] == 0, (b, pats[b])
            elif t[b] <= T:
                assert self.want[b] == t[b] and self.sets[b] == self.hit[b], (b, pats[b])
            elif t[b] <= m - T:
                assert self.want[b] == UNKNOWN, (b, pats[b])

    def shards(self, img):
        """[B, n, S] copy of the arena's slots."""
        return shards(img, self.data, self.par)

    def flip(self, b, s, x, v=None):
        """shard s of block b, byte x ^= v (nonzero). Nothing for a byte already changed, and nothing
        below L for a shard that would take the block past its cap of corrupt shards."""
        if (b, s, x) in self.flipped:
            return
        if x < self.L and s not in self.hit[b] and len(self.hit[b]) >= self.cap:
            return
        v = int(self.rng.integers(1, 256)) if v is None else v
        assert v
        self.flipped.add((b, s, x))
        self.img[(self.data.at(b, s) if s < self.k else self.par.at(b, s - self.k)) + x] ^= v
        if x < self.L:
            self.hit[b].add(s)

    def corrupt(self, b, pat):
        k, m, n, L, T, rng = self.k, self.m, self.n, self.L, self.T, self.rng
        cps = (L + 15) // 16
        perm = [int(s) for s in rng.permutation(n)]          # distinct random shards
        ca = int(rng.integers(cps))
        cb = (ca + 1 + int(rng.integers(cps - 1))) % cps if cps > 1 else ca

        def byte_in(c):   # a byte of chunk c below L
            return 16 * c + int(rng.integers(min(16, L - 16 * c)))
        xa, xb = byte_in(ca), byte_in(cb)
        if pat == 0:                                   # none
            pass
        elif pat == 1:                                 # one shard, one bit
            self.flip(b, perm[0], xa, 1 << int(rng.integers(8)))
        elif pat == 2:                                 # T shards in one byte column
            for s in perm[:T]:
                self.flip(b, s, xa)
        elif pat == 3:                                 # T shards, each in another chunk (while there are chunks)
            for i, s in enumerate(perm[:T]):
                self.flip(b, s, byte_in((ca + i) % cps))
        elif pat == 4:                                 # supports {a, b} and {b, c} in two chunks
            self.flip(b, perm[0], xa), self.flip(b, perm[1 % n], xa)
            self.flip(b, perm[1 % n], xb), self.flip(b, perm[2 % n], xb)
        elif pat == 5:                                 # shard 0 among the corrupt
            self.flip(b, 0, xb)
            for s in [s for s in perm if s][:max(T - 1, 0)]:
                self.flip(b, s, xb)
        elif pat == 6:                                 # parity shards only
            for s in [s for s in perm if s >= k][:max(T, 1)]:
                self.flip(b, s, xa if rng.integers(2) else xb)
        elif pat == 7:                                 # a data and a parity shard
            self.flip(b, int(rng.integers(k)), xa)
            if m:
                self.flip(b, k + int(rng.integers(m)), xb)
        elif pat == 8:                                 # one shard, every byte
            for x in range(L):
                self.flip(b, perm[0], x)
        elif pat == 9:                                 # T + 1 shards in one byte column
            for s in perm[:T + 1]:
                self.flip(b, s, xa)
        elif pat == 10:                                # T + 1 shards, no chunk holding more than T (while there are chunks)
            for i, s in enumerate(perm[:T + 1]):
                self.flip(b, s, byte_in((ca + i) % cps))
        elif pat == 11:                                # bytes at and past L only: clean
            for s in (perm[0], k if m else 0, n - 1):
                self.flip(b, s, L), self.flip(b, s, self.data.ss - 1)
        elif pat == 12:                                # the tail chunk: the last byte below L
            for s in perm[:max(min(T, 1 + int(rng.integers(max(T, 1)))), 1)]:
                self.flip(b, s, L - 1)
        elif pat == 13:                                # t random shards at random bytes, 0 <= t <= n
            for s in perm[:int(rng.integers(n + 1))]:
                self.flip(b, s, int(rng.integers(L)))
        else:
            raise ValueError(pat)

    def upload(self, img=None):
        dev = self.torch.from_numpy(np.array(self.img if img is None else img)).cuda()   # (a writable copy)
        assert dev.data_ptr() % 16 == 0
        return dev

    def call(self, dev, bad, present, W, counts, max_bad=None):
        fec, p = self.fec, dev.data_ptr()
        return fec.lib.fec_rs_locate_multi_batch(
            self.codec.handle, self.k, self.m, self.L, self.B, p + self.data.off, self.data.bs,
            (p + self.par.off) if self.m else None, self.par.bs, self.data.ss,
            self.max_bad if max_bad is None else max_bad, bad.data_ptr(),
            None if present is None else present.data_ptr(), W, None if counts is None else counts.data_ptr(),
            fec.FEC_DEVICE)

    def want_present(self, counts, sets, W):
        bits = np.zeros((self.B, 32 * W), dtype=np.uint8)
        bits[:, :self.n] = 1
        for b in np.flatnonzero(counts > 0):
            bits[b, sorted(sets[b])] = 0
        return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(self.B, W)

    def locate(self, dev, W, present=True, counts=True, want=None, sets=None, what=""):
        """One call on the arena dev: results, masks and counts against (want, sets) (default: the
        model's), the arena against its image before the call. Returns (results, present_out tensor)."""
        fec, torch = self.fec, self.torch
        want = self.want if want is None else want
        sets = self.sets if sets is None else sets
        before = dev.cpu().numpy()
        bad = torch.full((self.B,), 99, dtype=torch.int32, device="cuda")
        pm = torch.full((self.B, W), STALE, dtype=torch.int32, device="cuda") if present else None
        cnt = torch.full((2,), STALE, dtype=torch.int32, device="cuda") if counts else None
        assert self.call(dev, bad, pm, W, cnt) == fec.FEC_OK, what
        assert self.codec.lib_sync_rc() == fec.FEC_OK, what          # a corrupt block is a result, not an error
        got = bad.cpu().numpy()
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, "%s: results differ at blocks %s: got %s, want %s" % (what, diff[:8], got[diff[:8]],
                                                                                    want[diff[:8]])
        if counts:
            assert cnt.cpu().numpy().tolist() == [int((got > 0).sum()), int((got == UNKNOWN).sum())], what
        if present:
            gotpm = pm.cpu().numpy().view(np.uint32)
            wantpm = self.want_present(want, sets, W)
            rows = np.flatnonzero((gotpm != wantpm).any(axis=1))
            assert rows.size == 0, "%s: masks differ at blocks %s: got %s, want %s" % (what, rows[:4], gotpm[rows[:4]],
                                                                                      wantpm[rows[:4]])
        check_arena(dev.cpu().numpy(), before, what)
        return got, pm

    def run(self):
        fec = self.fec
        Wmin = fec.mask_words(self.n)
        dev = self.upload()
        self.locate(dev, Wmin, what="minimum mask words")
        self.locate(dev, 8, counts=False, what="8 mask words, no counts")
        self.locate(dev, Wmin, present=False, what="no masks")
        self.locate(dev, Wmin, present=False, counts=False, what="results alone")
        clean = self.upload(self.clean)
        self.locate(clean, Wmin, want=np.zeros(self.B, dtype=np.int32), what="clean batch")
        self.heal(dev)

    def heal(self, dev):
        """locate-multi -> reconstruct with present_out as its masks: reconstruct-some for n <= 32, which
        rebuilds data and parity; the wide reconstruct otherwise, which rebuilds data shards and leaves a
        located parity shard to a later encode. Every block with t <= T corrupt shards holds its original
        bytes again (past the radius the set named may be a wrong one); the others are untouched; a
        second call reports 0 for the located blocks (the wide path: the corrupt parity shards that are
        still there, and 0 after an encode) and leaves the unknown ones unknown."""
        fec, p, k, n, L = self.fec, dev.data_ptr(), self.k, self.n, self.L
        narrow = n <= 32
        W = 1 if narrow else fec.mask_words(n)
        got, pm = self.locate(dev, W, what="heal: locate")
        args = (self.codec.handle, k, self.m, L, self.B, p + self.data.off, self.data.bs,
                (p + self.par.off) if self.m else None, self.par.bs, self.data.ss, pm.data_ptr())
        if narrow:
            rc = fec.lib.fec_rs_reconstruct_some_batch(*args, None, None, fec.FEC_DEVICE)
        else:
            rc = fec.lib.fec_rs_reconstruct_wide_batch(*args, W, None, fec.FEC_DEVICE)
        assert rc == fec.FEC_OK and self.codec.lib_sync_rc() == fec.FEC_OK
        healed = self.shards(dev.cpu().numpy())[:, :, :L]
        orig = self.shards(self.clean)[:, :, :L]
        loc = got > 0
        within = loc & (np.array([len(h) for h in self.hit]) <= self.T)
        assert within.any() or self.T == 0
        rebuilt = n if narrow else k
        assert np.array_equal(healed[within][:, :rebuilt], orig[within][:, :rebuilt]), "blocks within the radius hold their original bytes"
        assert np.array_equal(healed[~loc], self.shards(self.img)[:, :, :L][~loc]), "the others are untouched"
        if narrow:
            want2, sets2 = np.where(loc, 0, got).astype(np.int32), self.sets
        else:   # the located parity shards are still corrupt
            sets2 = [frozenset(s for s in self.sets[b] if s >= k) if loc[b] else self.sets[b] for b in range(self.B)]
            want2 = np.array([len(sets2[b]) if loc[b] else got[b] for b in range(self.B)], dtype=np.int32)
        self.locate(dev, W, want=want2, sets=sets2, what="heal: second locate")
        if not narrow and not (got == UNKNOWN).any():
            assert fec.lib.fec_rs_encode_batch(self.codec.handle, k, self.m, L, self.B, p + self.data.off, self.data.bs,
                                               p + self.par.off, self.par.bs, self.data.ss, fec.FEC_DEVICE) == fec.FEC_OK
            assert self.codec.lib_sync_rc() == fec.FEC_OK
            assert np.array_equal(self.shards(dev.cpu().numpy())[:, :, :L][within], orig[within])
            self.locate(dev, W, want=np.zeros(self.B, dtype=np.int32), what="heal: locate after the encode")


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_locate_multi_counts_masks_and_heal(codec, torch, fec, oracle, gf, layout, k, m, L):
    Batch(codec, fec, torch, oracle, gf, layout, k, m, L, 67, 1000 * k + 10 * m + L).run()


def test_locate_multi_max_bad_below_the_radius(codec, torch, fec, oracle, gf):
    """(20,10) with max_bad 2: T = 2, so three corrupt shards (<= m - T = 8) give unknown although the
    code could name them; up to eight corrupt shards stay unknown."""
    b = Batch(codec, fec, torch, oracle, gf, "interleaved", 20, 10, 33, 67, 77, max_bad=2)
    assert b.T == 2 and b.cap == 8
    dev = b.upload()
    three = [i for i in range(b.B) if len(b.hit[i]) == 3]
    assert three and all(b.want[i] == UNKNOWN for i in three)
    b.locate(dev, 1, what="max_bad 2")


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (240, 16), (31, 1)])
def test_locate_multi_max_bad_one_equals_locate(codec, torch, fec, oracle, gf, k, m):
    """max_bad = 1 against fec_rs_locate_batch on the same arena, block for block: clean with 0, shard s
    with count 1 and bit s cleared, unknown with unknown."""
    b = Batch(codec, fec, torch, oracle, gf, "split", k, m, 33, 67, 5 + k, max_bad=1)
    dev = b.upload()
    W = fec.mask_words(b.n)
    got, pm = b.locate(dev, W, what="max_bad 1")
    p = dev.data_ptr()
    old = torch.full((b.B,), 99, dtype=torch.int32, device="cuda")
    opm = torch.full((b.B, W), STALE, dtype=torch.int32, device="cuda")
    assert fec.lib.fec_rs_locate_batch(codec.handle, k, m, b.L, b.B, p + b.data.off, b.data.bs, p + b.par.off, b.par.bs,
                                       b.data.ss, old.data_ptr(), opm.data_ptr(), W, None, fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    old = old.cpu().numpy()
    assert np.array_equal(got, np.where(old == fec.FEC_LOCATE_CLEAN, 0, np.where(old >= 0, 1, UNKNOWN)))
    assert (old >= 0).any() or m < 2
    assert (old == fec.FEC_LOCATE_UNKNOWN).any()
    assert torch.equal(pm, opm)


@pytest.mark.parametrize("k,m,B", [(8, 4, 13)])
def test_locate_multi_block_spanning_workgroups(codec, torch, fec, oracle, gf, k, m, B):
    """70 000-byte shards (4375 chunks: a block spans 18 workgroups and 69 bitmap words), so the
    supports of one block meet in its words from many waves of the solve. One block per pattern, the
    random one left to the other tests."""
    Batch(codec, fec, torch, oracle, gf, "interleaved", k, m, 70000, B, 17 + k, patterns=list(range(B))).run()


def test_locate_multi_codec_methods_and_heal_loop(codec, torch, fec):
    """Codec.rs_locate_multi / rs_locate_multi_split on [B, n, S] tensors, shard_len below the slot
    size, then Codec.rs_reconstruct_some with the masks the call wrote."""
    k, m, S, L, B = 6, 4, 48, 41, 9
    sh = torch.randint(0, 256, (B, k + m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode(k, m, sh, shard_len=L)
    truth = sh.clone()
    sh[4, k + 1, L - 1] ^= 1          # a parity shard
    sh[6, 2, 0] ^= 0x80               # two data shards in different chunks
    sh[6, 0, 40] ^= 0x01
    sh[7, 0, 5] ^= 3                  # shard 0
    sh[3, 1, 20] ^= 9                 # a data and a parity shard in one column
    sh[3, k + 3, 20] ^= 0xFF
    sh[2, 0, L] ^= 1                  # pad byte of a data slot
    want = [0, 0, 0, 2, 1, 0, 2, 1, 0]
    sets = {3: [1, k + 3], 4: [k + 1], 6: [0, 2], 7: [0]}
    bad = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    pm = torch.full((B, 1), STALE, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), STALE, dtype=torch.int32, device="cuda")
    assert codec.rs_locate_multi(k, m, sh, bad, present_out=pm, counts=cnt, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == want and cnt.cpu().tolist() == [4, 0]
    full = (1 << (k + m)) - 1
    assert pm.cpu().flatten().tolist() == [full & ~sum(1 << s for s in sets.get(b, [])) for b in range(B)]
    # max_bad = 1: the blocks of two corrupt shards are unknown (2 <= m - 1)
    assert codec.rs_locate_multi(k, m, sh, bad, 1, counts=cnt, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == [0, 0, 0, UNKNOWN, 1, 0, UNKNOWN, 1, 0] and cnt.cpu().tolist() == [2, 2]
    data, par = sh[:, :k].contiguous(), sh[:, k:].contiguous()
    bad.fill_(99)
    assert codec.rs_locate_multi_split(k, m, data, par, bad, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == want
    codec.rs_reconstruct_some(k, m, sh, pm.flatten(), shard_len=L)
    codec.sync()
    assert torch.equal(sh[:, :, :L], truth[:, :, :L])
    assert codec.rs_locate_multi(k, m, sh, bad, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == [0] * B
    with pytest.raises(AssertionError):
        codec.rs_locate_multi(k, m, sh.cpu(), bad, shard_len=L)


def test_locate_multi_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx, in order: nblocks == 0 touches nothing, then pointers, layouts, the
    alignment of the three word arrays; None for either optional output works."""
    h, D = codec.handle, fec.FEC_DEVICE
    INV, ALIGN = fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_ALIGNMENT
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 99, dtype=torch.int32, device="cuda")
    p, s = buf.data_ptr(), out.data_ptr()
    pm, cn = s + 16, s + 32

    def F(k, m, L, B, data, dbs, par, pbs, ss, bad, present=None, W=1, counts=None, max_bad=2):
        return fec.lib.fec_rs_locate_multi_batch(h, k, m, L, B, data, dbs, par, pbs, ss, max_bad, bad, present, W,
                                                 counts, D)
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
    # m > 16, max_bad and mask_words are checked before the ctx's work, with valid buffers too
    assert F(2, 17, 16, 2, p, 64, p + 32, 64, 16, s) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, max_bad=0) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, max_bad=9) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, None, 0) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, s, None, 9) == INV
    # a pointer error comes before a layout error, a layout error before the word alignment
    assert F(2, 2, 16, 2, p + 8, 64, p + 32, 64, 16, None) == INV
    assert F(2, 2, 17, 2, p, 64, p + 32, 64, 16, s + 2) == INV
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and (out.cpu().numpy() == 99).all()
    # m = 0: no parity, every block 0; both optional outputs
    assert F(2, 0, 16, 2, p, 32, None, 0, 16, s, pm, 2, cn) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    got = out.cpu().numpy()
    assert got[:2].tolist() == [0, 0] and got[4:8].tolist() == [3, 0, 3, 0] and got[8:10].tolist() == [0, 0]
    assert (got[[2, 3, 10, 11]] == 99).all() and (buf.cpu().numpy() == CANARY).all()
