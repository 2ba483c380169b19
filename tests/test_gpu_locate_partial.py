"""fec_rs_locate_partial_batch (corrupt shards of blocks that also have missing shards) on the device,
by the guarded-arena method of test_gpu_locate_multi.py, whose batch, corruption patterns and arena
check this module reuses: the whole arena is compared with its image before each call, the outputs are
pre-filled with a stale value, and every missing shard's slot is filled with garbage over its whole
stride (a batch is run twice with different garbage: the outputs must not change).

Every block gets an erasure kind, chosen so that neighbours differ and a wave spans blocks of
different e: none missing; e = m (vacuous); e = m + 1 (too few; for n > 32 a whole mask word clear);
e = m - 1 (detect only); shard 0 missing; data shards only; parity shards only; a random few. The
corruption patterns are the sibling's, applied to present shards (a flip of a missing shard is
dropped). Some blocks' masks carry stray bits at and above n.

The expected results come from a model written here in numpy with the ORACLE's gf_mul and
build_matrix. With e_b missing shards and T_b = min(max_bad, (m - e_b) // 2):
  - codes of n <= 12: the definition by brute force against the punctured generator. Every set E of
    at most T_b present shards is tried in ascending size; E explains the block if every byte column
    of the present shards outside E lies in the column space of the generator's rows of those shards
    (tested with a basis of the left null space of those rows). Any number of corrupt shards.
  - larger codes: at most (m - e_b) - T_b corrupt present shards, so the theorem gives the
    expectation: exactly the corrupt shards for t <= T_b, unknown above.
Every block is compared, for bad_count, present_out and the three counts.
"""
import functools
import itertools

import numpy as np
import pytest

from arena import CANARY, STALE, check_arena, codec, encoded_arena, gf, torch  # noqa: F401
from test_gpu_locate_multi import BRUTE_N, NPATTERNS, Batch, left_null

pytestmark = pytest.mark.gpu

UNKNOWN, TOO_FEW = -2, -3
MAX_BAD = 8
LENS = [1, 15, 16, 17, 33, 1202]
CODES = [(1, 2), (2, 2), (6, 3), (8, 4), (20, 10), (4, 16), (240, 16), (31, 1), (32, 0)]
LAYOUTS = ["interleaved", "split"]
NKINDS = 8


def model_brute(oracle, gf, k, m, T, present, y, L):
    """One block by the definition: present (sorted shard indices), y [n, S]. (count, frozenset)."""
    mul, _ = gf
    M = oracle.build_matrix(k, k + m)
    code = M[k:].tobytes()                                # the cache of null spaces is per matrix

    def residue(rows, Y):
        """N Y for a basis N of the left null space of the generator's rows `rows`: zero columns are the
        columns of Y (one byte per row) that lie in the column space of those rows."""
        N = left_null(gf, M[list(rows)], ("punctured", k, m, tuple(rows), code))
        return np.bitwise_xor.reduce(mul[N[:, :, None], Y[None, :, :]], axis=1)
    if len(present) <= k:
        return 0, frozenset()                             # any k rows of the generator are independent
    # a byte column that fits all present shards fits every subset of them: only the others are tried
    Y = y[:, :L]
    Y = np.unique(Y[:, residue(present, Y[present]).any(axis=0)], axis=1)
    if Y.shape[1] == 0:
        return 0, frozenset()
    for v in range(1, T + 1):
        found = []
        for E in itertools.combinations(present, v):
            rows = [r for r in present if r not in E]
            if len(rows) <= k or not residue(rows, Y[rows]).any():
                found.append(E)
        assert len(found) <= 1, "distance m - e + 1 > 2 T: at most one smallest set explains a block"
        if found:
            return v, frozenset(found[0])
    return UNKNOWN, frozenset()


class PBatch(Batch):
    """An encoded batch with missing shards per block by kind and corrupt present shards by pattern.
    build(layout, k, m, L, B, rng) makes the encoded arena: encoded_arena by default, arena.oracle_arena for
    test_gpu_row_sweep.py."""

    def __init__(self, codec, fec, torch, oracle, gf, layout, k, m, L, B, seed, patterns=None, kinds=None,
                 build=None):
        self.codec, self.fec, self.torch, self.oracle, self.gf = codec, fec, torch, oracle, gf
        self.k, self.m, self.n, self.L, self.B = k, m, k + m, L, B
        self.max_bad = MAX_BAD
        self.brute = self.n <= BRUTE_N
        self.rng = rng = np.random.default_rng(seed)
        build = build or functools.partial(encoded_arena, codec, fec, torch)
        img, self.data, self.par = build(layout, k, m, L, B, rng)
        self.clean = img.copy()
        self.clean.setflags(write=False)
        self.kinds = kinds or [(b * 3 + 1) % NKINDS for b in range(B)]           # neighbours differ
        self.miss = [self.erase(kd) for kd in self.kinds]
        self.e = np.array([len(x) for x in self.miss])
        self.few = self.e > m
        self.Tb = np.where(self.few, 0, np.minimum(MAX_BAD, (m - np.minimum(self.e, m)) // 2))
        # larger codes: at most (m - e) - T corrupt present shards (too few: the bytes do not matter)
        self.capb = [self.n if self.brute or self.few[b] else int(m - self.e[b] - self.Tb[b]) for b in range(B)]
        self.hit = [set() for _ in range(B)]
        self.flipped = set()
        self.img = img
        pats = patterns or [(b * 5 + 3) % NPATTERNS for b in range(B)]
        for b, pat in enumerate(pats):
            self.T = int(self.Tb[b])          # the sibling's patterns size themselves by the radius
            self.corrupt(b, pat)
        self.garbage(rng)
        self.img.setflags(write=False)
        bits = np.zeros((B, 256), dtype=np.uint8)
        bits[:, :self.n] = 1
        for b in range(B):
            bits[b, sorted(self.miss[b])] = 0
            if b % 3 == 0:
                bits[b, self.n:] = rng.integers(0, 2, 256 - self.n)   # stray bits at and above n: ignored
        self.bits = bits
        self._expect = {}
        assert (self.e == 0).any() and self.few.any()
        if m:
            assert (self.e == m).any() and (self.e == m - 1).any()

    def erase(self, kind):
        k, m, n, rng = self.k, self.m, self.n, self.rng
        perm = [int(s) for s in rng.permutation(n)]
        if kind == 0 or (m == 0 and kind != 2):
            return set()
        if kind == 1:
            return set(perm[:m])
        if kind == 2:                                      # too few
            return set(range(32, 64)) if n > 64 else set(perm[:m + 1])
        if kind == 3:
            return set(perm[:m - 1])
        if kind == 4:
            return {0}
        if kind == 5:
            return set([s for s in perm if s < k][:max(1, m // 2)])
        if kind == 6:
            return set([s for s in perm if s >= k][:max(1, m // 2)])
        return set(perm[:int(rng.integers(0, m // 2 + 1))])

    def flip(self, b, s, x, v=None):
        """The sibling's flip, on present shards only and with the block's own cap."""
        if s in self.miss[b]:
            return
        self.cap = self.capb[b]
        Batch.flip(self, b, s, x, v)

    def garbage(self, rng, img=None):
        """Random bytes over the whole slot of every missing shard."""
        img = self.img if img is None else img
        for b in range(self.B):
            for s in self.miss[b]:
                at = self.data.at(b, s) if s < self.k else self.par.at(b, s - self.k)
                img[at:at + self.data.ss] = rng.integers(0, 256, self.data.ss, dtype=np.uint8)

    def masks(self, W):
        return np.packbits(self.bits[:, :32 * W], axis=1, bitorder="little").view("<u4").reshape(self.B, W).copy()

    def expect(self, max_bad):
        """(results [B], sets [B]) at this max_bad."""
        if max_bad in self._expect:
            return self._expect[max_bad]
        k, m, n = self.k, self.m, self.n
        want = np.zeros(self.B, dtype=np.int32)
        sets = [frozenset()] * self.B
        sh = self.shards(self.img) if self.brute else None
        for b in range(self.B):
            if self.few[b]:
                want[b] = TOO_FEW
                continue
            sums = m - int(self.e[b])
            T, t = min(max_bad, sums // 2), len(self.hit[b])
            if self.brute:
                present = [r for r in range(n) if r not in self.miss[b]]
                want[b], sets[b] = model_brute(self.oracle, self.gf, k, m, T, present, sh[b], self.L)
            else:
                assert t <= sums - T
                want[b], sets[b] = (t, frozenset(self.hit[b])) if t <= T else (UNKNOWN, frozenset())
            # what must hold whatever the model
            if t == 0:
                assert want[b] == 0, (b, self.kinds[b])
            elif t <= T:
                assert want[b] == t and sets[b] == self.hit[b], (b, self.kinds[b])
            elif t <= sums - T:
                assert want[b] == UNKNOWN, (b, self.kinds[b])
        self._expect[max_bad] = (want, sets)
        return want, sets

    def want_present(self, want, sets, W):
        bits = self.bits[:, :32 * W].copy()
        bits[:, self.n:] = 0
        for b in np.flatnonzero(want > 0):
            bits[b, sorted(sets[b])] = 0
        return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(self.B, W)

    def call(self, dev, masks, W, max_bad, bad, present, counts):
        fec, p = self.fec, dev.data_ptr()
        return fec.lib.fec_rs_locate_partial_batch(
            self.codec.handle, self.k, self.m, self.L, self.B, p + self.data.off, self.data.bs,
            (p + self.par.off) if self.m else None, self.par.bs, self.data.ss, masks.data_ptr(), W, max_bad,
            bad.data_ptr(), None if present is None else present.data_ptr(),
            None if counts is None else counts.data_ptr(), fec.FEC_DEVICE)

    def locate(self, dev, W, present=True, counts=True, alias=False, max_bad=MAX_BAD, what=""):
        """One call on the arena dev: results, masks and counts against the model at max_bad, the arena
        against its image before the call, the masks read unchanged unless aliased.
        Returns (results, present_out tensor, the three counts or None)."""
        fec, torch = self.fec, self.torch
        want, sets = self.expect(max_bad)
        before = dev.cpu().numpy()
        mk = torch.from_numpy(self.masks(W).view(np.int32)).cuda()
        mk0 = mk.cpu().numpy().view(np.uint32)
        bad = torch.full((self.B,), 99, dtype=torch.int32, device="cuda")
        pm = mk if alias else torch.full((self.B, W), STALE, dtype=torch.int32, device="cuda") if present else None
        cnt = torch.full((3,), STALE, dtype=torch.int32, device="cuda") if counts else None
        assert self.call(dev, mk, W, max_bad, bad, pm, cnt) == fec.FEC_OK, what
        assert self.codec.lib_sync_rc() == fec.FEC_OK, what          # no result is an error
        got = bad.cpu().numpy()
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, "%s: results differ at blocks %s: got %s, want %s, kinds %s" % (
            what, diff[:8], got[diff[:8]], want[diff[:8]], [self.kinds[b] for b in diff[:8]])
        three = None
        if counts:
            three = cnt.cpu().numpy().tolist()
            assert three == [int((got > 0).sum()), int((got == UNKNOWN).sum()), int((got == TOO_FEW).sum())], what
        if pm is not None:
            gotpm = pm.cpu().numpy().view(np.uint32)
            wantpm = self.want_present(want, sets, W)
            rows = np.flatnonzero((gotpm != wantpm).any(axis=1))
            assert rows.size == 0, "%s: masks differ at blocks %s: got %s, want %s" % (what, rows[:4], gotpm[rows[:4]],
                                                                                      wantpm[rows[:4]])
        if not alias:
            assert np.array_equal(mk.cpu().numpy().view(np.uint32), mk0), what + ": present_mask is only read"
        check_arena(dev.cpu().numpy(), before, what)
        return got, pm, three

    def run(self):
        fec = self.fec
        Wmin = fec.mask_words(self.n)
        dev = self.upload()
        got, pm, three = self.locate(dev, Wmin, what="minimum mask words")
        self.locate(dev, 8, counts=False, what="8 mask words, no counts")
        self.locate(dev, Wmin, present=False, what="no masks written")
        self.locate(dev, Wmin, present=False, counts=False, what="results alone")
        self.locate(dev, Wmin, alias=True, what="present_out is present_mask")
        self.locate(dev, Wmin, max_bad=0, what="max_bad 0: verify under the masks")
        if self.m >= 4:
            self.locate(dev, Wmin, max_bad=1, what="max_bad below the radius")
        # other garbage in the missing slots: the same outputs
        img2 = np.array(self.img)
        self.garbage(np.random.default_rng(12345), img2)
        assert not np.array_equal(img2, self.img) or not any(self.miss)
        got2, pm2, three2 = self.locate(self.upload(img2), Wmin, what="other garbage")
        assert np.array_equal(got, got2) and self.torch.equal(pm, pm2) and three == three2


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("k,m", CODES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_locate_partial_results_masks_and_counts(codec, torch, fec, oracle, gf, layout, k, m, L):
    PBatch(codec, fec, torch, oracle, gf, layout, k, m, L, 67, 2000 * k + 10 * m + L).run()


def test_locate_partial_max_bad_below_the_radius(codec, torch, fec, oracle, gf):
    """(20,10) with max_bad 2: a block with e missing shards and three corrupt ones (<= (m - e) - 2) is
    unknown although the punctured code could name them; max_bad 0 names nothing."""
    b = PBatch(codec, fec, torch, oracle, gf, "interleaved", 20, 10, 33, 67, 78)
    dev = b.upload()
    want2, _ = b.expect(2)
    three = [i for i in range(b.B) if len(b.hit[i]) == 3 and not b.few[i]]
    assert three and all(want2[i] == UNKNOWN for i in three)
    assert any(b.expect(8)[0][i] == 3 for i in three)
    b.locate(dev, 1, max_bad=2, what="max_bad 2")
    want0, _ = b.expect(0)
    assert set(want0.tolist()) == {0, UNKNOWN, TOO_FEW}
    b.locate(dev, 1, max_bad=0, what="max_bad 0")


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (240, 16), (31, 1)])
def test_locate_partial_full_masks_equal_locate_multi(codec, torch, fec, oracle, gf, k, m):
    """Every mask full: results, masks and counts[0..1] of fec_rs_locate_multi_batch on the same arena,
    block for block, and counts[2] == 0."""
    old = Batch(codec, fec, torch, oracle, gf, "split", k, m, 33, 67, 5 + k)
    dev = old.upload()
    W = fec.mask_words(old.n)
    got, pm = old.locate(dev, W, what="locate-multi")
    cnt_old = torch.full((2,), STALE, dtype=torch.int32, device="cuda")
    bad_old = torch.full((old.B,), 99, dtype=torch.int32, device="cuda")
    assert old.call(dev, bad_old, None, W, cnt_old) == fec.FEC_OK
    full = np.packbits(np.arange(32 * W) < old.n, bitorder="little").view("<u4")
    mk = torch.from_numpy(np.tile(full, (old.B, 1)).view(np.int32)).cuda()
    bad = torch.full((old.B,), 99, dtype=torch.int32, device="cuda")
    pm2 = torch.full((old.B, W), STALE, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), STALE, dtype=torch.int32, device="cuda")
    p = dev.data_ptr()
    before = dev.cpu().numpy()
    assert fec.lib.fec_rs_locate_partial_batch(codec.handle, k, m, old.L, old.B, p + old.data.off, old.data.bs,
                                               p + old.par.off, old.par.bs, old.data.ss, mk.data_ptr(), W, MAX_BAD,
                                               bad.data_ptr(), pm2.data_ptr(), cnt.data_ptr(),
                                               fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert np.array_equal(bad.cpu().numpy(), got) and torch.equal(pm2, pm)
    assert cnt.cpu().tolist() == cnt_old.cpu().tolist() + [0]
    assert (got > 0).any() or m < 2
    assert (got != 0).any()
    check_arena(dev.cpu().numpy(), before, "full masks")


def test_locate_partial_block_spanning_workgroups(codec, torch, fec, oracle, gf):
    """70 000-byte shards (4375 chunks: a block spans 18 workgroups and 69 bitmap words), RS(8,12), one
    corruption pattern per block, the erasure kinds cycling."""
    B = 13
    b = PBatch(codec, fec, torch, oracle, gf, "interleaved", 8, 4, 70000, B, 25, patterns=list(range(B)),
               kinds=[(b * 3 + 1) % NKINDS for b in range(8)] + [0, 4, 5, 6, 7])
    dev = b.upload()
    b.locate(dev, 1, what="70 000-byte shards")
    b.locate(dev, 8, counts=False, alias=True, what="70 000-byte shards, masks in place")


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (40, 16)])
def test_locate_partial_heal_loop_without_a_sync(codec, torch, fec, oracle, gf, k, m):
    """Queued back to back with no sync between them: locate-partial, the reconstruct with the masks it
    wrote (reconstruct-some for n <= 32; the wide reconstruct, which rebuilds data shards, for n > 32),
    locate-partial again with those masks. Blocks within their radius hold their original bytes in every
    shard the reconstruct rebuilds and report 0 the second time; unknown and too-few blocks are
    unchanged and report what they reported."""
    b = PBatch(codec, fec, torch, oracle, gf, "interleaved", k, m, 33, 67, 91 + k)
    n, L, B = b.n, b.L, b.B
    narrow = n <= 32
    W = fec.mask_words(n)
    want, sets = b.expect(MAX_BAD)
    dev = b.upload()
    p = dev.data_ptr()
    mk = torch.from_numpy(b.masks(W).view(np.int32)).cuda()
    pm = torch.full((B, W), STALE, dtype=torch.int32, device="cuda")
    bad1 = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    bad2 = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    cnt2 = torch.full((3,), STALE, dtype=torch.int32, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    assert b.call(dev, mk, W, MAX_BAD, bad1, pm, None) == fec.FEC_OK
    args = (codec.handle, k, m, L, B, p + b.data.off, b.data.bs, p + b.par.off, b.par.bs, b.data.ss, pm.data_ptr())
    if narrow:
        assert fec.lib.fec_rs_reconstruct_some_batch(*args, None, st.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
    else:
        assert fec.lib.fec_rs_reconstruct_wide_batch(*args, W, st.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
    assert b.call(dev, pm, W, MAX_BAD, bad2, None, cnt2) == fec.FEC_OK
    # the reconstruct reports the too-few blocks as it always does; the locate calls add nothing
    assert codec.lib_sync_rc() == (fec.FEC_ERR_TOO_FEW_SHARDS if b.few.any() else fec.FEC_OK)
    assert np.array_equal(bad1.cpu().numpy(), want)
    assert np.array_equal(pm.cpu().numpy().view(np.uint32), b.want_present(want, sets, W))
    healed = b.shards(dev.cpu().numpy())[:, :, :L]
    orig, was = b.shards(b.clean)[:, :, :L], b.shards(b.img)[:, :, :L]
    t = np.array([len(h) for h in b.hit])
    within = ~b.few & (t <= b.Tb)
    assert (within & (want > 0)).any() and (want == UNKNOWN).any()
    rebuilt = n if narrow else k
    for i in np.flatnonzero(within):
        redo = sorted(s for s in (b.miss[i] | set(sets[i])) if s < rebuilt)
        keep = sorted(set(range(n)) - set(redo))
        assert np.array_equal(healed[i, redo], orig[i, redo]), i
        assert np.array_equal(healed[i, keep], was[i, keep]), i
    # an unknown block keeps its mask, so the reconstruct fills its missing slots and touches no present
    # shard; a too-few block is left alone altogether
    status = st.cpu().numpy()
    for i in np.flatnonzero(want == UNKNOWN):
        has = sorted(set(range(n)) - b.miss[i])
        assert np.array_equal(healed[i, has], was[i, has]), i
    assert np.array_equal(healed[b.few], was[b.few])
    assert (status[b.few] == fec.FEC_ERR_TOO_FEW_SHARDS).all() and (status[~b.few] == 0).all()
    got2 = bad2.cpu().numpy()
    assert (got2[within] == 0).all()
    assert (got2[b.few] == TOO_FEW).all() and (got2[want == UNKNOWN] == UNKNOWN).all()
    assert cnt2.cpu().tolist()[2] == int(b.few.sum())


def test_locate_partial_codec_methods(codec, torch, fec):
    """Codec.rs_locate_partial / rs_locate_partial_split on [B, n, S] tensors, shard_len below the slot
    size, masks updated in place, then Codec.rs_reconstruct_some with them."""
    k, m, S, L, B = 6, 4, 48, 41, 8
    n = k + m
    sh = torch.randint(0, 256, (B, n, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode(k, m, sh, shard_len=L)
    truth = sh.clone()
    full = (1 << n) - 1
    miss = {1: [2], 2: [0, k + 1], 3: [1], 4: [3, 4, 5, k], 5: [0, 1, 2, 3, 4], 6: [k + 3], 7: [5]}
    for b, ss in miss.items():
        for s in ss:
            sh[b, s] = torch.randint(0, 256, (S,), dtype=torch.uint8, device="cuda")
    sh[1, 4, 7] ^= 0x10               # one missing, one corrupt: T = 1
    sh[2, 3, 40] ^= 1                 # two missing, one corrupt: T = 1
    sh[3, 0, 0] ^= 5                  # one missing, two corrupt: T = 1, 2 <= 3 - 1: unknown
    sh[3, k, 0] ^= 7
    sh[6, 2, L] ^= 1                  # a pad byte: clean
    sh[7, 0, 3] ^= 9                  # one missing, one corrupt, max_bad 0 below: unknown
    masks = torch.tensor([[full & ~sum(1 << s for s in miss.get(b, []))] for b in range(B)], dtype=torch.int32,
                         device="cuda")
    want = [0, 1, 1, -2, 0, -3, 0, 1]
    bad = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    pm = torch.full((B, 1), STALE, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), STALE, dtype=torch.int32, device="cuda")
    assert codec.rs_locate_partial(k, m, sh, masks, bad, present_out=pm, counts=cnt, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == want and cnt.cpu().tolist() == [3, 1, 1]
    located = {1: [4], 2: [3], 7: [0]}
    assert pm.cpu().flatten().tolist() == [int(masks[b, 0]) & ~sum(1 << s for s in located.get(b, [])) for b in range(B)]
    assert codec.rs_locate_partial(k, m, sh, masks, bad, 0, counts=cnt, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == [0, -2, -2, -2, 0, -3, 0, -2] and cnt.cpu().tolist() == [0, 4, 1]
    data, par = sh[:, :k].contiguous(), sh[:, k:].contiguous()
    inplace = masks.clone()
    assert codec.rs_locate_partial_split(k, m, data, par, inplace, bad, present_out=inplace, shard_len=L) == fec.FEC_OK
    codec.sync()
    assert bad.cpu().tolist() == want and torch.equal(inplace, pm)
    ok = [b for b in range(B) if want[b] >= 0]
    pm[5] = full                       # the too-few block: nothing to rebuild, no error
    pm[3] = full                       # the unknown block is left as it is
    codec.rs_reconstruct_some(k, m, sh, pm.flatten(), shard_len=L)
    codec.sync()
    assert torch.equal(sh[ok][:, :, :L], truth[ok][:, :, :L])
    with pytest.raises(AssertionError):
        codec.rs_locate_partial(k, m, sh.cpu(), masks, bad, shard_len=L)


def test_locate_partial_argument_errors_on_the_device(codec, torch, fec):
    """The checks past the ctx, in order: nblocks == 0 touches nothing, then pointers, layouts, the
    alignment of the four word arrays; max_bad 0 runs; None for either optional output works."""
    h, D = codec.handle, fec.FEC_DEVICE
    INV, ALIGN = fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_ALIGNMENT
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    out = torch.full((20,), 99, dtype=torch.int32, device="cuda")
    mk = torch.tensor([15, 15, 15, 15], dtype=torch.int32, device="cuda")
    p, s, q = buf.data_ptr(), out.data_ptr(), mk.data_ptr()
    pm, cn = s + 16, s + 32

    def F(k, m, L, B, data, dbs, par, pbs, ss, masks, bad, present=None, W=1, counts=None, max_bad=2):
        return fec.lib.fec_rs_locate_partial_batch(h, k, m, L, B, data, dbs, par, pbs, ss, masks, W, max_bad, bad,
                                                   present, counts, D)
    assert F(2, 2, 16, 0, None, 0, None, 0, 16, None, None) == fec.FEC_OK
    assert F(2, 2, 16, 0, None, 0, None, 0, 16, None, None, max_bad=0) == fec.FEC_OK     # 0 is accepted,
    assert F(2, 2, 16, 0, None, 0, None, 0, 16, None, None, max_bad=9) == INV            # 9 and -1 are not
    assert F(2, 2, 16, 0, None, 0, None, 0, 16, None, None, max_bad=-1) == INV
    assert F(2, 2, 16, 2, None, 64, p + 32, 64, 16, q, s) == INV
    assert F(2, 2, 16, 2, p, 64, None, 64, 16, q, s) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, None) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, None, s) == INV          # the masks are required
    assert F(2, 2, 16, 2, p + 8, 64, p + 32, 64, 16, q, s) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 56, 16, q, s) == ALIGN
    assert F(2, 2, 17, 2, p, 64, p + 32, 64, 16, q, s) == INV             # stride < length
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, s + 2) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q + 2, s) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, s, pm + 1) == ALIGN
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, s, pm, 1, cn + 2) == ALIGN
    # m > 16, max_bad and mask_words are checked before the ctx's work, with valid buffers too
    assert F(2, 17, 16, 2, p, 64, p + 32, 64, 16, q, s) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, s, max_bad=9) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, s, None, 0) == INV
    assert F(2, 2, 16, 2, p, 64, p + 32, 64, 16, q, s, None, 9) == INV
    # a pointer error comes before a layout error, a layout error before the word alignment
    assert F(2, 2, 16, 2, p + 8, 64, p + 32, 64, 16, q, None) == INV
    assert F(2, 2, 17, 2, p, 64, p + 32, 64, 16, q + 2, s) == INV
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (buf.cpu().numpy() == CANARY).all() and (out.cpu().numpy() == 99).all()
    # m = 0: no parity; a full mask gives 0, a missing shard too few; two mask words; max_bad 0
    two = torch.tensor([3, 0, 1, 0], dtype=torch.int32, device="cuda")
    assert F(2, 0, 16, 2, p, 32, None, 0, 16, two.data_ptr(), s, pm, 2, cn, max_bad=0) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    got = out.cpu().numpy()
    assert got[:2].tolist() == [0, -3] and got[4:8].tolist() == [3, 0, 1, 0] and got[8:11].tolist() == [0, 0, 1]
    assert (got[[2, 3, 11, 12]] == 99).all() and (buf.cpu().numpy() == CANARY).all()
