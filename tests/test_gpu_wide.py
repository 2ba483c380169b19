"""Wide RS decode on the device (fec_rs_reconstruct_wide_batch / fec_rs_recover_wide_batch,
fec_wide.hip): codes of up to 256 shards, present masks of 1..8 words per block.

Codes of at most 32 shards run the wide kernels when given two mask words, and are then checked
against the oracle's ReconstructData; with one word the call must forward to the narrow one. Wider
codes are checked against an inverse-matrix reference written here (the rows of the inverse of the
first-k-present submatrix, applied with a 256 x 256 product table built from the oracle's gf_mul),
and against the original data.
"""
import numpy as np
import pytest

from arena import CANARY, GUARD, MUL, codec, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

ERASED = 0x5A


def encoded(oracle, rng, B, k, m, L, S=None):
    """Encoded shards [B, k + m, S], zero from L to S."""
    S = rup16(L) if S is None else S
    sh = np.zeros((B, k + m, S), dtype=np.uint8)
    sh[:, :k, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    oracle.rs_encode(k, m, sh)
    sh[:, :, L:] = 0
    return sh


_MATS = {}


def ref_reconstruct(oracle, MUL, k, m, shards, present, L):
    """The reference: per block, the rows of the inverse of the first-k-present submatrix of the
    systematic matrix give each erased data shard as the XOR of MUL[coef][shard] over the first k
    present shards. shards [B, n, S] is rebuilt in place over [0, L), zeros to the 16-byte boundary;
    returns the statuses (0, or -4 for fewer than k present shards)."""
    n = k + m
    if (k, n) not in _MATS:
        _MATS[(k, n)] = oracle.build_matrix(k, n)
    M = _MATS[(k, n)]
    st = np.zeros(len(shards), dtype=np.int32)
    for b in range(len(shards)):
        lost = np.flatnonzero(~present[b, :k])
        if len(lost) == 0:
            continue
        have = np.flatnonzero(present[b])
        if len(have) < k:
            st[b] = -4
            continue
        S = have[:k]
        inv = oracle.invert(M[S])
        src = shards[b, S, :L]
        for o in lost:
            shards[b, o, :L] = np.bitwise_xor.reduce(MUL[inv[o][:, None], src], axis=0)
            shards[b, o, L:rup16(L)] = 0
    return st


def damage(sh, present, fill=ERASED):
    d = sh.copy()
    d[~present] = fill
    return d


def run_wide(fec, codec, torch, k, m, dmg, masks, L):
    """In-place wide reconstruct of dmg [B, n, S] with masks [B, W]; returns (shards, statuses, sync rc)."""
    d = torch.from_numpy(dmg).cuda()
    dm = torch.from_numpy(np.ascontiguousarray(masks).view(np.int32)).cuda()
    ds = torch.full((len(dmg),), 99, dtype=torch.int32, device="cuda")
    rc = codec.rs_reconstruct_wide(k, m, d, dm, status=ds, shard_len=L)
    assert rc == fec.FEC_OK
    src = codec.lib_sync_rc()
    return d.cpu().numpy(), ds.cpu().numpy(), src


# ------------------------------------------------------------------ 1. n <= 32 through the wide kernels

NARROW_SHAPES = [(2, 1), (8, 4), (16, 8), (20, 10), (31, 1), (10, 22)]


def narrow_case(oracle, k, m, L, B=67):
    rng = np.random.default_rng(9000 + 100 * k + m + L)
    n = k + m
    sh = encoded(oracle, rng, B, k, m, L)
    present = np.ones((B, n), dtype=bool)
    for b in range(B):
        present[b, rng.choice(n, size=int(rng.integers(0, min(n, m + 1) + 1)), replace=False)] = False
    clean = (present * (1 << np.arange(n, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    return rng, sh, present, clean


@pytest.mark.parametrize("k,m", NARROW_SHAPES)
@pytest.mark.parametrize("L", [1, 17, 513, 1202])
def test_wide_kernels_match_oracle_reconstruct(fec, codec, oracle, torch, k, m, L):
    rng, sh, present, clean = narrow_case(oracle, k, m, L)
    B, n = present.shape
    masks = rng.integers(0, 1 << 32, (B, 2), dtype=np.uint64).astype(np.uint32)   # word 1: garbage
    high = np.uint32((0xFFFFFFFF << n) & 0xFFFFFFFF)
    masks[:, 0] = clean | (masks[:, 0] & high)                                    # garbage above bit n
    dmg = damage(sh, present)
    ref = dmg.copy()
    st_ref = oracle.rs_reconstruct(k, m, ref, clean, length=L)
    for b in range(B):   # rebuilt shards carry zero padding up to the 16-byte boundary of their slot
        if st_ref[b] == 0:
            ref[b, :k][~present[b, :k], L:rup16(L)] = 0
    got, st, sync = run_wide(fec, codec, torch, k, m, dmg, masks, L)
    assert np.array_equal(st == 0, st_ref == 0) and set(np.unique(st)) <= {0, -4}
    assert np.array_equal(got, ref)
    ok = st_ref == 0
    assert np.array_equal(got[ok, :k, :L], sh[ok, :k, :L])
    assert sync == (fec.FEC_ERR_TOO_FEW_SHARDS if (st_ref != 0).any() else fec.FEC_OK)


@pytest.mark.parametrize("k,m", NARROW_SHAPES)
@pytest.mark.parametrize("L", [1, 17, 513, 1202])
def test_one_mask_word_forwards_to_narrow_call(fec, codec, oracle, torch, k, m, L):
    rng, sh, present, clean = narrow_case(oracle, k, m, L)
    B = len(sh)
    dmg = damage(sh, present)
    got, st, sync = run_wide(fec, codec, torch, k, m, dmg, clean.reshape(B, 1), L)
    d = torch.from_numpy(dmg).cuda()
    dm = torch.from_numpy(clean.view(np.int32)).cuda()
    ds = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct(k, m, d, dm, status=ds, shard_len=L)
    assert sync == codec.lib_sync_rc()
    assert np.array_equal(got, d.cpu().numpy()) and np.array_equal(st, ds.cpu().numpy())
    # recover form too
    slots = max(1, min(k, m))
    outs = []
    for wide in (True, False):
        dd, dp = torch.from_numpy(dmg[:, :k].copy()).cuda(), torch.from_numpy(dmg[:, k:].copy()).cuda()
        out = torch.full((B, slots, dmg.shape[2]), CANARY, dtype=torch.uint8, device="cuda")
        ds = torch.full((B,), 99, dtype=torch.int32, device="cuda")
        if wide:
            dm1 = torch.from_numpy(clean.reshape(B, 1).view(np.int32)).cuda()
            codec.rs_recover_wide_split(k, m, dd, dp, dm1, out, status=ds, shard_len=L)
        else:
            codec.rs_recover_split(k, m, dd, dp, dm, out, status=ds, shard_len=L)
        outs.append((out.cpu().numpy(), ds.cpu().numpy(), codec.lib_sync_rc()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2]


# ------------------------------------------------------------------ 2. n > 32 against the inverse-matrix reference

WIDE_SHAPES = [(20, 13), (32, 1), (1, 32), (33, 31), (33, 32), (64, 16), (16, 240), (128, 128), (255, 1), (1, 255),
               (200, 56)]
PREFERRED = [31, 32, 63, 64]   # the mask word boundaries


def pick(rng, pool, count, first=()):
    """`count` distinct members of pool: those of `first` that are in it, then random others."""
    pool = [int(i) for i in pool]
    got = [i for i in dict.fromkeys(int(i) for i in first) if i in pool][:count]
    rest = [i for i in pool if i not in got]
    rng.shuffle(rest)
    return got + rest[:count - len(got)]


def erase_block(rng, k, m, e):
    """Present row of one recoverable block with e erased data shards (the word-boundary shards
    first) and parity erasures within what leaves k shards present (boundary shards first)."""
    n = k + m
    p = np.ones(n, dtype=bool)
    p[pick(rng, range(k), e, PREFERRED)] = False
    budget = m - e
    if budget > 0:
        npar = int(rng.integers(0, budget + 1))
        npar = max(npar, min(budget, sum(1 for i in PREFERRED if k <= i < n)))
        p[pick(rng, range(k, n), npar, PREFERRED)] = False
    return p


def wide_present(rng, k, m):
    """One batch holding: a complete block, e = 1, e = 16 and e = 17 where min(k, m) allows (the row
    pass boundary), e = min(k, m), and a block with k - 1 shards present. That is up to six kinds, so
    the batch has max(5, kinds) blocks (5 where fewer kinds exist, filled with a random e)."""
    n, top = k + m, min(k, m)
    es = [0, 1] + [e for e in (16, 17) if e <= top] + [top]
    es = sorted(set(es))
    while len(es) < 4:
        es.append(int(rng.integers(1, top + 1)))
    rows = [erase_block(rng, k, m, e) for e in es]
    fail = np.ones(n, dtype=bool)
    fail[pick(rng, range(n), m + 1, [int(rng.integers(0, k))] + PREFERRED)] = False   # k - 1 present, a data shard lost
    rows.append(fail)
    return np.array(rows), es


@pytest.mark.parametrize("k,m", WIDE_SHAPES)
@pytest.mark.parametrize("L", [17, 1202])
def test_wide_reconstruct_matches_inverse_reference(fec, codec, oracle, torch, MUL, k, m, L):
    rng = np.random.default_rng(31 * k + m + L)
    present, es = wide_present(rng, k, m)
    B = len(present)
    assert B >= 5 and present[-1].sum() == k - 1 and not present[-1, :k].all()
    sh = encoded(oracle, rng, B, k, m, L)
    dmg = damage(sh, present)
    ref = dmg.copy()
    st_ref = ref_reconstruct(oracle, MUL, k, m, ref, present, L)
    assert list(st_ref) == [0] * (B - 1) + [-4]
    assert np.array_equal(ref[:-1, :k], sh[:-1, :k])   # the reference reproduces the original data
    got, st, sync = run_wide(fec, codec, torch, k, m, dmg, fec.wide_masks(present), L)
    assert np.array_equal(st, st_ref)
    assert np.array_equal(got, ref)
    assert np.array_equal(got[:-1, :k, :L], sh[:-1, :k, :L])
    assert sync == fec.FEC_ERR_TOO_FEW_SHARDS


def test_wide_accepts_eight_mask_words(fec, codec, oracle, torch, MUL):
    """mask_words above FEC_MASK_WORDS(n): the extra words are ignored."""
    k, m, L = 20, 13, 513
    rng = np.random.default_rng(8)
    present = np.array([erase_block(rng, k, m, e) for e in (0, 1, 5, 13)])
    sh = encoded(oracle, rng, len(present), k, m, L)
    masks = rng.integers(0, 1 << 32, (len(present), 8), dtype=np.uint64).astype(np.uint32)
    w = fec.wide_masks(present)
    masks[:, 0] = w[:, 0]
    masks[:, 1] = w[:, 1] | (masks[:, 1] & np.uint32(0xFFFFFFFC))   # garbage above bit 33
    got, st, sync = run_wide(fec, codec, torch, k, m, damage(sh, present), masks, L)
    assert sync == fec.FEC_OK and not st.any()
    assert np.array_equal(got[:, :k], sh[:, :k])


# ------------------------------------------------------------------ 3. first-k rule

def test_rebuild_reads_only_the_first_k_present(fec, codec, oracle, torch):
    k, m, L, B = 40, 20, 1202, 3
    rng = np.random.default_rng(40)
    sh = encoded(oracle, rng, B, k, m, L)
    present = np.ones((B, k + m), dtype=bool)
    for b in range(B):
        present[b, pick(rng, range(k), 10, PREFERRED[:2])] = False
    dmg = damage(sh, present)
    dmg[:, k + 10:, :] = 0xEE   # present, but past the first k present shards: never read
    got, st, sync = run_wide(fec, codec, torch, k, m, dmg, fec.wide_masks(present), L)
    assert sync == fec.FEC_OK and not st.any()
    assert np.array_equal(got[:, :k], sh[:, :k])
    assert np.array_equal(got[:, k:], dmg[:, k:])


# ------------------------------------------------------------------ 4. recover form

@pytest.mark.parametrize("k,m", [(40, 20), (64, 16)])
@pytest.mark.parametrize("one_slot", [True, False])
def test_wide_recover_statuses_order_and_canaries(fec, codec, oracle, torch, k, m, one_slot):
    L, S = 1202, 1232
    maxe = min(k, m)
    slots = 1 if one_slot else maxe
    rng = np.random.default_rng(k + slots)
    es = [0, 1, 2, maxe, 1, 3]
    present = [erase_block(rng, k, m, e) for e in es]
    fail = np.ones(k + m, dtype=bool)
    fail[pick(rng, range(k + m), m + 1, [5] + PREFERRED)] = False
    present = np.array(present + [fail])
    B = len(present)
    sh = encoded(oracle, rng, B, k, m, L, S)
    dmg = damage(sh, present)
    dd, dp = torch.from_numpy(dmg[:, :k].copy()).cuda(), torch.from_numpy(dmg[:, k:].copy()).cuda()
    dm = torch.from_numpy(fec.wide_masks(present).view(np.int32)).cuda()
    out = torch.full((B, slots, S), CANARY, dtype=torch.uint8, device="cuda")
    ds = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_recover_wide_split(k, m, dd, dp, dm, out, status=ds, shard_len=L)
    sync = codec.lib_sync_rc()
    want_st = np.array([e if e <= slots else -1 for e in es] + [-4], dtype=np.int32)
    assert np.array_equal(ds.cpu().numpy(), want_st)
    assert sync == fec.FEC_ERR_TOO_FEW_SHARDS
    model = np.full((B, slots, S), CANARY, dtype=np.uint8)
    for b in range(B):
        if want_st[b] > 0:
            lost = np.flatnonzero(~present[b, :k])   # ascending
            model[b, :len(lost), :L] = sh[b, lost, :L]
            model[b, :len(lost), L:rup16(L)] = 0
    assert np.array_equal(out.cpu().numpy(), model)
    assert np.array_equal(dd.cpu().numpy(), dmg[:, :k]) and np.array_equal(dp.cpu().numpy(), dmg[:, k:])


# ------------------------------------------------------------------ 5. layouts in a guarded arena

ARENA_B = 67


class Slots:
    """Shard slots at off + b*bs + r*ss of an arena, b < B."""

    def __init__(self, off, bs, ss, rows, B=ARENA_B):
        assert off % 16 == 0 and bs % 16 == 0 and ss % 16 == 0
        self.off, self.bs, self.ss, self.rows, self.B = off, bs, ss, rows, B

    def idx(self, lo, hi):
        """[B, rows, hi - lo] arena indices of bytes [lo, hi) of every slot."""
        return (self.off + np.arange(self.B)[:, None, None] * self.bs + np.arange(self.rows)[None, :, None] * self.ss
                + np.arange(lo, hi)[None, None, :])

    def end(self):
        return self.off + (self.B - 1) * self.bs + (self.rows - 1) * self.ss + self.ss


def arena_layout(name, k, m, L, slots, B=ARENA_B):
    R, n = rup16(L), k + m
    if name == "interleaved_slack":
        ss = R + 32
        bs = n * ss + 48
        data, par = Slots(GUARD, bs, ss, k, B), Slots(GUARD + k * ss, bs, ss, m, B)
        out = Slots(GUARD, slots * ss + 32, ss, slots, B)
    elif name == "split_parity_below":
        ss = R + 16
        par = Slots(GUARD, m * ss + 16, ss, m, B)
        data = Slots(par.end() + 80, k * ss + 48, ss, k, B)
        out = Slots(GUARD, slots * ss + 32, ss, slots, B)
    else:   # shard_major: [k + m][B][sp]
        sp = R + 16
        ss = B * sp
        data, par = Slots(GUARD, sp, ss, k, B), Slots(GUARD + k * ss, sp, ss, m, B)
        out = Slots(GUARD, sp, ss, slots, B)
    return data, par, out


ARENA_KINDS = [0, 1, 2, 7, 20, -1, 16, 17]   # data shards a block of RS(40,20) loses (-1: k - 1 shards present)


def arena_case(oracle, layout, L, B=ARENA_B):
    """(kinds, present, shards) of the RS(40,20) batch of the whole-arena test: the kinds dealt in turn
    and shuffled, so a batch of eight blocks or more holds every one."""
    k, m = 40, 20
    n = k + m
    rng = np.random.default_rng(L + len(layout))
    kinds = np.array((ARENA_KINDS * 9)[:B])
    rng.shuffle(kinds)
    present = np.ones((B, n), dtype=bool)
    for b in range(B):
        if kinds[b] >= 0:
            present[b] = erase_block(rng, k, m, int(kinds[b]))
        else:
            present[b, pick(rng, range(n), m + 1, [int(rng.integers(0, k))])] = False
    return kinds, present, encoded(oracle, rng, B, k, m, L)


@pytest.mark.parametrize("layout", ["interleaved_slack", "split_parity_below", "shard_major"])
@pytest.mark.parametrize("L", [1202, 33])
def test_wide_calls_write_only_their_output_bytes(fec, codec, oracle, torch, layout, L):
    """The whole canary-filled arena, guards included, equals a model after reconstruct and after
    recover: a call may write only bytes [0, L) of the shards it rebuilds, plus zeros to their
    16-byte boundary. (The rebuilt bytes are the originals: case 2 ties them to the reference.)"""
    run_wide_arena(fec, codec, oracle, torch, layout, L)


def run_wide_arena(fec, codec, oracle, torch, layout, L, B=ARENA_B):
    k, m = 40, 20
    n, R, slots = k + m, rup16(L), min(k, m)
    kinds, present, sh = arena_case(oracle, layout, L, B)
    data, par, out = arena_layout(layout, k, m, L, slots, B)
    img = np.full(max(data.end(), par.end()) + GUARD, CANARY, dtype=np.uint8)
    dmg = damage(sh, present)
    img[data.idx(0, L)] = dmg[:, :k, :L]     # input slots hold canary bytes from L on
    img[par.idx(0, L)] = dmg[:, k:, :L]
    ok = kinds > 0
    st_want = np.where(kinds < 0, -4, 0).astype(np.int32)
    masks = torch.from_numpy(fec.wide_masks(present).view(np.int32)).cuda()
    W = fec.mask_words(n)

    # recover: the shard arena is only read
    arena = torch.from_numpy(img).cuda()
    oimg = np.full(out.end() + GUARD, CANARY, dtype=np.uint8)
    oarena = torch.from_numpy(oimg).cuda()
    ds = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    rc = codec.rs_recover_wide_raw(k, m, L, B, arena.data_ptr() + data.off, data.bs, arena.data_ptr() + par.off,
                                   par.bs, data.ss, masks.data_ptr(), W, oarena.data_ptr() + out.off, out.bs, slots,
                                   ds.data_ptr())
    assert rc == fec.FEC_OK and codec.lib_sync_rc() == fec.FEC_ERR_TOO_FEW_SHARDS
    assert np.array_equal(ds.cpu().numpy(), np.where(kinds < 0, -4, kinds))
    omodel = oimg.copy()
    oi_l, oi_r = out.idx(0, L), out.idx(L, R)
    for b in np.flatnonzero(ok):
        lost = np.flatnonzero(~present[b, :k])
        omodel[oi_l[b, :len(lost)]] = sh[b, lost, :L]
        omodel[oi_r[b, :len(lost)]] = 0
    assert np.array_equal(oarena.cpu().numpy(), omodel)
    assert np.array_equal(arena.cpu().numpy(), img)

    # reconstruct in place
    ds.fill_(99)
    rc = codec.rs_reconstruct_wide_raw(k, m, L, B, arena.data_ptr() + data.off, data.bs, arena.data_ptr() + par.off,
                                       par.bs, data.ss, masks.data_ptr(), W, ds.data_ptr(), fec.FEC_DEVICE)
    assert rc == fec.FEC_OK and codec.lib_sync_rc() == fec.FEC_ERR_TOO_FEW_SHARDS
    assert np.array_equal(ds.cpu().numpy(), st_want)
    model = img.copy()
    di_l, di_r = data.idx(0, L), data.idx(L, R)
    for b in np.flatnonzero(ok):
        lost = np.flatnonzero(~present[b, :k])
        model[di_l[b, lost]] = sh[b, lost, :L]
        model[di_r[b, lost]] = 0
    assert np.array_equal(arena.cpu().numpy(), model)


# ------------------------------------------------------------------ 6. host form

@pytest.mark.parametrize("k,m", [(40, 20), (128, 128)])
def test_wide_host_form(fec, codec, oracle, MUL, k, m):
    L, B = 1202, 9
    rng = np.random.default_rng(k)
    top = min(k, m)
    es = [0, 1, 16, 17, top, 2, 3, 5]
    present = np.array([erase_block(rng, k, m, e) for e in es] + [np.zeros(k + m, dtype=bool)])
    present[-1, pick(rng, range(k + m), k - 1)] = True   # k - 1 present
    sh = encoded(oracle, rng, B, k, m, L, S=L)           # packed: stride == shard_len
    dmg = damage(sh, present)
    ref = dmg.copy()
    st_ref = ref_reconstruct(oracle, MUL, k, m, ref, present, L)
    got = dmg.copy()
    st = np.full(B, 99, dtype=np.int32)
    rc = codec.rs_reconstruct_wide(k, m, got, fec.wide_masks(present), status=st)
    assert rc == fec.FEC_ERR_TOO_FEW_SHARDS            # a block failed; the others are still rebuilt
    assert np.array_equal(st, st_ref) and list(st_ref) == [0] * 8 + [-4]
    assert np.array_equal(got, ref)
    assert np.array_equal(got[:-1, :k], sh[:-1, :k])
    # no failing block: FEC_OK
    got2 = dmg[:-1].copy()
    assert codec.rs_reconstruct_wide(k, m, got2, fec.wide_masks(present[:-1])) == fec.FEC_OK
    assert np.array_equal(got2, ref[:-1])


# ------------------------------------------------------------------ 7. a batch larger than one launch slice

def test_wide_batch_spans_launch_slices(fec, codec, torch):
    """RS(128,128), 17-byte shards, 20000 blocks: the plan records (about 16.5 KiB each) exceed the
    plan workspace bound, so the batch runs as two slices. Parity from the device encode (checked
    against the oracle elsewhere); one data shard lost per block; the round trip gives the data back."""
    k, m, L, S, B = 128, 128, 17, 32, 20000
    g = torch.Generator(device="cuda").manual_seed(7)
    data = torch.zeros((B, k, S), dtype=torch.uint8, device="cuda")
    data[:, :, :L] = torch.randint(0, 256, (B, k, L), dtype=torch.uint8, device="cuda", generator=g)
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    rng = np.random.default_rng(7)
    lost = rng.integers(0, k, B)
    lost[:4] = [0, 31, 32, 127]
    present = np.ones((B, k + m), dtype=bool)
    present[np.arange(B), lost] = False
    dmg = data.clone()
    dmg[torch.arange(B, device="cuda"), torch.from_numpy(lost).cuda()] = ERASED
    dm = torch.from_numpy(fec.wide_masks(present).view(np.int32)).cuda()
    ds = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    assert codec.rs_reconstruct_wide_split(k, m, dmg, parity, dm, status=ds, shard_len=L) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert not ds.any().item()
    assert torch.equal(dmg, data)
