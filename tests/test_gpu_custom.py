"""Custom code matrices (include/fec_hip_matrix.h fec_ctx_set_custom_matrix, klauspost WithCustomMatrix)
through the RS calls of the device ABI that serve them, byte for byte against the definition model
(tests/custom_model.py: the matrices by formula, parity by table lookups, rebuilds by Gaussian
elimination on the whole k x k matrix). Whole images are compared: rebuilt slots hold the codeword and
zeros up to the 16-byte boundary; every other byte, every byte of a failed block among them, keeps what
it held.

The decode plans come from fec_plan_solve.hip (rs_plan_solve_kernel in block order and sorted,
rs_plan_solve_some_kernel); the rebuild kernels are the ones every other matrix runs."""
import numpy as np
import pytest

import custom_model as cu
from arena import torch  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = 0x5A        # what a missing shard's slot holds
STALE = 0xA5       # what an output slot holds before the call
TOO_FEW, SLOTS, SINGULAR = -4, -1, -11


@pytest.fixture(scope="module")
def codec(fec):
    c = fec.Codec(0).use_torch_stream()
    yield c
    c.close()


@pytest.fixture(scope="module")
def codec0(fec):
    c = fec.Codec(0).use_torch_stream()
    yield c
    c.close()


_P = {}


def prow(fec, name, k, m):
    if (name, k, m) not in _P:
        _P[name, k, m] = np.ascontiguousarray(cu.rows(name, k, m, fec))
    return _P[name, k, m]


def use(codec, fec, name, k, m):
    """Register the test matrix on the codec (identical rows reuse their code) and return n x k."""
    P = prow(fec, name, k, m)
    codec.set_custom_matrix(k, m, P)
    assert codec.matrix == "custom"
    return cu.matrix(P)


def rup16(x):
    return (x + 15) // 16 * 16


_CW = {}


def codewords(M, B, L, S, seed):
    """[B, n, S]: random data and the model's parity in bytes [0, L), zeros behind. Computed once per
    case and shared (callers copy before they change it)."""
    key = (M.tobytes(), M.shape, B, L, S, seed)
    if key not in _CW:
        rng = np.random.default_rng(seed)
        n, k = M.shape
        sh = np.zeros((B, n, S), dtype=np.uint8)
        sh[:, :k, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        sh[:, k:, :L] = cu.encode(M, sh[:, :k, :L])
        _CW[key] = sh
    return _CW[key]


def words1(pres):
    return (pres.astype(np.uint64) << np.arange(pres.shape[1], dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def damage(sh, pres):
    d = sh.copy()
    d[~pres] = FILL
    return d


def rebuilt(dmg, sh, L, which):
    ref = dmg.copy()
    b, i = np.nonzero(which)
    ref[b, i, :L] = sh[b, i, :L]
    ref[b, i, L:rup16(L)] = 0
    return ref


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(torch, a):
    return dev(torch, np.ascontiguousarray(a).view(np.int32))


def expect(M, pres, slots=0, want=None):
    """(status [B], which [B, n]) by the rule of fec_status.hpp with the singular block after it.
    want None: reconstruct (slots 0) / recover: the erased data shards. want bool [B, n]:
    reconstruct-some, the missing wanted shards, data and parity."""
    B, n = pres.shape
    k = M.shape[1]
    st = np.zeros(B, dtype=np.int32)
    which = np.zeros((B, n), dtype=bool)
    for b in range(B):
        miss = ~pres[b] & want[b] if want is not None else ~pres[b] & (np.arange(n) < k)
        e = int(miss.sum())
        if e == 0:
            continue
        if pres[b].sum() < k:
            st[b] = TOO_FEW
        elif slots and e > slots:
            st[b] = SLOTS
        elif cu.decode(M, pres[b]) is cu.SINGULAR:
            st[b] = SINGULAR
        else:
            st[b] = e if slots else 0
            which[b] = miss
            S, T = cu.decode(M, pres[b])
            assert np.array_equal(T[S], np.eye(k, dtype=np.uint8))       # the model's rows give the inputs back
    return st, which


def sync_rc(st):
    """What fec_sync returns for these statuses (fec_status.hpp sticky_rc)."""
    for code in (TOO_FEW, SLOTS, SINGULAR):
        if (st == code).any():
            return code
    return 0


def run_inplace(c, torch, k, m, sh, pres, L, M):
    dmg = damage(sh, pres)
    d = dev(torch, dmg)
    st = torch.full((len(sh),), 99, dtype=torch.int32, device="cuda")
    c.rs_reconstruct(k, m, d, i32(torch, words1(pres)), status=st, shard_len=L)
    rc = c.lib_sync_rc()
    want_st, which = expect(M, pres)
    got = d.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert np.array_equal(got, rebuilt(dmg, sh, L, which))
    assert rc == sync_rc(want_st)
    return got, st.cpu().numpy()


def run_recover(c, torch, k, m, sh, pres, L, M, slots):
    B, S = sh.shape[0], sh.shape[2]
    dmg = damage(sh, pres)
    d, p = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, slots, S), STALE, dtype=torch.uint8, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    c.rs_recover_split(k, m, d, p, i32(torch, words1(pres)), out, status=st, shard_len=L)
    rc = c.lib_sync_rc()
    want_st, which = expect(M, pres, slots=slots)
    wout = np.full((B, slots, S), STALE, dtype=np.uint8)
    for b in np.nonzero(which.any(axis=1))[0]:
        for r, i in enumerate(np.nonzero(which[b])[0]):
            wout[b, r, :L] = sh[b, i, :L]
            wout[b, r, L:rup16(L)] = 0
    got = out.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert np.array_equal(got, wout)
    assert np.array_equal(d.cpu().numpy(), dmg[:, :k]) and np.array_equal(p.cpu().numpy(), dmg[:, k:])
    assert rc == sync_rc(want_st)
    return got, st.cpu().numpy()


# ------------------------------------------------------------------ 1. the encode family
@pytest.mark.parametrize("L,S", [(1202, 1216), (40, 48)])
@pytest.mark.parametrize("name", cu.NAMES)
def test_encode_8_4(codec, torch, fec, name, L, S):
    M = use(codec, fec, name, 8, 4)
    want = codewords(M, 300, L, S, 1).copy()
    sh = want.copy()
    sh[:, 8:] = STALE
    want[:, 8:, rup16(L):] = STALE
    d = dev(torch, sh)
    codec.rs_encode(8, 4, d, shard_len=L)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), want)


# k > 32 (no decode tables at all), and 20 parity rows: two row passes of 16
@pytest.mark.parametrize("k,m", [(100, 4), (5, 20)])
def test_encode_wide_shapes(codec, torch, fec, k, m):
    M = use(codec, fec, "cauchy255", k, m)
    L, S, B = 1202, 1216, 37
    want = codewords(M, B, L, S, 2).copy()
    sh = want.copy()
    sh[:, k:] = STALE
    want[:, k:, rup16(L):] = STALE
    d = dev(torch, sh)
    codec.rs_encode(k, m, d, shard_len=L)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize("row", [(3, 2), (1, 1)])
def test_encode_2_1_takes_the_generic_fold(codec, torch, row):
    # 03 02 is the row rs_encode23 is written for: a custom code must still take the generic kernel
    # (fixed_encode() returns none for it), and 01 01 must not be mistaken for it
    codec.set_custom_matrix(2, 1, np.array([row], dtype=np.uint8))
    rng = np.random.default_rng(23)
    x = rng.integers(0, 256, (129, 3, 1216), dtype=np.uint8)
    d = dev(torch, x)
    codec.rs_encode(2, 1, d)
    codec.sync()
    assert np.array_equal(d.cpu().numpy()[:, 2], cu.MUL[row[0]][x[:, 0]] ^ cu.MUL[row[1]][x[:, 1]])
    assert np.array_equal(d.cpu().numpy()[:, :2], x[:, :2])


def test_lrc_verify_update_encode_idx(codec, torch, fec):
    k, m, B, L, S = 8, 4, 41, 200, 208
    M = use(codec, fec, "lrc", k, m)
    sh = codewords(M, B, L, S, 3)
    rng = np.random.default_rng(4)
    st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    codec.rs_verify(k, m, dev(torch, sh), st, count=cnt, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 1).all() and int(cnt.cpu()[0]) == 0
    bad = sh.copy()
    bad[17, 5, 199] ^= 0x10                                   # one flipped byte
    codec.rs_verify(k, m, dev(torch, bad), st, count=cnt, shard_len=L)
    codec.sync()
    want = np.ones(B, dtype=np.int32)
    want[17] = 0
    assert np.array_equal(st.cpu().numpy(), want) and int(cnt.cpu()[0]) == 1
    # update of two columns: their difference folded into the parity, the old data stays
    cols = np.zeros((B, k), dtype=bool)
    for b in range(B):
        cols[b, rng.choice(k, size=2, replace=False)] = True
    new = sh[:, :k].copy()
    new[:, :, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    after = np.where(cols[:, :, None], new, sh[:, :k])
    masks = dev(torch, fec.wide_masks(cols).view(np.int32))
    d = dev(torch, sh)
    codec.rs_update(k, m, d, dev(torch, new), masks, shard_len=L)
    codec.sync()
    wantu = sh.copy()
    wantu[:, k:, :L] = cu.encode(M, after[:, :, :L])
    assert np.array_equal(d.cpu().numpy(), wantu)
    # encode-idx over a partial column mask into zeroed parity: the parity of the masked columns alone
    z = sh.copy()
    z[:, k:] = 0
    d = dev(torch, z)
    codec.rs_encode_idx(k, m, d, masks, shard_len=L)
    codec.sync()
    part = z.copy()
    part[:, k:, :L] = cu.encode(M, np.where(cols[:, :, None], sh[:, :k], 0)[:, :, :L])
    assert np.array_equal(d.cpu().numpy(), part)


# ------------------------------------------------------------------ 2. every pattern of (8, 4)
def pattern_batch(name, P):
    """The 778 patterns (asserted against the model first), every pattern with 5 missing (too few), and
    three whole blocks."""
    pats, sing = cu.check_8_4(name, P)
    few = cu.patterns(12, 8, [5])
    return np.concatenate([pats, few, np.ones((3, 12), dtype=bool)]), len(pats)


@pytest.mark.parametrize("L,S", [(48, 48), (1202, 1216)], ids=["tile", "wave"])
@pytest.mark.parametrize("name", cu.NAMES)
def test_every_pattern_8_4(codec, codec0, torch, fec, name, L, S):
    # L = 48: 3 chunks, block-order plans and the workgroup-tile rebuild; L = 1202: 76 chunks, sorted
    # plans and the wave rebuild (in place, where no row has a zero, through the routed kernel)
    k, m = 8, 4
    M = use(codec, fec, name, k, m)
    pres, npat = pattern_batch(name, prow(fec, name, k, m))
    sh = codewords(M, len(pres), L, S, 5)
    got = [run_inplace(codec, torch, k, m, sh, pres, L, M),
           run_recover(codec, torch, k, m, sh, pres, L, M, 4),
           run_recover(codec, torch, k, m, sh, pres, L, M, 1)]    # the direct route where no row has a zero
    want_st, _ = expect(M, pres)
    assert (want_st == TOO_FEW).sum() == 792 and (want_st == SINGULAR).sum() == cu.SINGULAR_8_4[name]
    # only singular blocks fail: fec_sync says so (with the too-few blocks above it said too few)
    _, st = run_inplace(codec, torch, k, m, sh[:npat], pres[:npat], L, M)
    assert ((st == SINGULAR).sum() > 0) == (name in ("par1", "lrc"))
    if name == "default":
        # the same rows as kind 0: the same bytes and statuses from a codec that never heard of them
        M0 = fec.rs_matrix(k, m)
        assert np.array_equal(M, M0)
        ref = [run_inplace(codec0, torch, k, m, sh, pres, L, M0),
               run_recover(codec0, torch, k, m, sh, pres, L, M0, 4),
               run_recover(codec0, torch, k, m, sh, pres, L, M0, 1)]
        for (a, sa), (b, sb) in zip(got, ref):
            assert np.array_equal(a, b) and np.array_equal(sa, sb)


# ------------------------------------------------------------------ 3. other shapes under cauchy255
def drawn(rng, B, k, m, lo, hi):
    """bool [B, n] present: U{lo..hi} shards lost per block, a data shard always among them."""
    n = k + m
    pres = np.ones((B, n), dtype=bool)
    for b in range(B):
        e = int(rng.integers(lo, hi + 1))
        gone = rng.choice(n, size=e, replace=False)
        if gone.min() >= k:
            gone[0] = rng.integers(0, k)
        pres[b, gone] = False
    return pres


SHAPES = [
    (20, 10, 1216, 1216),    # sorted plans, then rs_rebuild_k
    (16, 8, 1202, 1216),
    (16, 8, 40, 48),         # block-order plans, the tile
    (31, 1, 1202, 1216), (31, 1, 40, 48),
    (1, 31, 1202, 1216), (1, 31, 40, 48),
]


@pytest.mark.parametrize("k,m,L,S", SHAPES)
def test_other_shapes(codec, torch, fec, k, m, L, S):
    rng = np.random.default_rng(1000 * k + m + L)
    B = 512
    M = use(codec, fec, "cauchy255", k, m)
    pres = drawn(rng, B, k, m, 1, m)
    pres[0] = True
    pres[0, :min(k, m)] = False                    # the most data shards a block can lose
    pres[1] = True
    pres[1, :m + 1] = False                        # too few: k - 1 shards present
    sh = codewords(M, B, L, S, 6)
    run_inplace(codec, torch, k, m, sh, pres, L, M)
    run_recover(codec, torch, k, m, sh, pres, L, M, min(k, m))


def test_4_8_every_lost_data_set(codec, torch, fec):
    # every set of 1..4 lost data shards, with every set of up to 2 lost parity shards beside it
    import itertools
    k, m, L, S = 4, 8, 200, 208
    M = use(codec, fec, "cauchy255", k, m)
    rows = []
    for e in range(1, 5):
        for dl in itertools.combinations(range(k), e):
            for pe in range(0, 3):
                for pl in itertools.combinations(range(k, k + m), pe):
                    p = np.ones(k + m, dtype=bool)
                    p[list(dl) + list(pl)] = False
                    rows.append(p)
    pres = np.array(rows)
    assert len(pres) == 15 * 37
    sh = codewords(M, len(pres), L, S, 7)
    got, st = run_inplace(codec, torch, k, m, sh, pres, L, M)
    assert (st == 0).all()
    run_recover(codec, torch, k, m, sh, pres, L, M, 4)
    run_recover(codec, torch, k, m, sh, pres, L, M, 2)


# ------------------------------------------------------------------ 4. reconstruct-some
@pytest.mark.parametrize("name", ["lrc", "par1"])
def test_reconstruct_some(codec, torch, fec, name):
    k, m, n, L, S = 8, 4, 12, 200, 208
    M = use(codec, fec, name, k, m)
    pats, sing = cu.check_8_4(name, prow(fec, name, k, m))
    pres = np.concatenate([pats, cu.patterns(12, 8, [5])[::8]])
    B = len(pres)
    sh = codewords(M, B, L, S, 8)
    dmg = damage(sh, pres)
    one_data = np.zeros((B, n), dtype=bool)
    one_data[np.arange(B), (~pres[:, :k]).argmax(axis=1)] = True     # the first missing data shard
    one_par = np.zeros((B, n), dtype=bool)
    one_par[:, 9] = True
    wants = {"one data shard": one_data, "parity shard 9": one_par, "everything": None,
             "nothing": np.zeros((B, n), dtype=bool)}
    for what, want in wants.items():
        d = dev(torch, dmg)
        st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
        codec.rs_reconstruct_some(k, m, d, i32(torch, words1(pres)),
                                  want=None if want is None else i32(torch, words1(want)), status=st, shard_len=L)
        rc = codec.lib_sync_rc()
        want_st, which = expect(M, pres, want=np.ones((B, n), dtype=bool) if want is None else want)
        assert np.array_equal(st.cpu().numpy(), want_st), what
        assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, L, which)), what
        assert rc == sync_rc(want_st), what
        if what == "everything":
            assert (want_st == SINGULAR).sum() >= sing.sum() and (want_st == TOO_FEW).sum() == B - len(pats)
        if what == "nothing":
            assert (want_st == 0).all()


# ------------------------------------------------------------------ 5. ragged and host forms under lrc
def test_ragged_reconstruct_lrc(codec, torch, fec):
    k, m, n, S = 8, 4, 12, 1216
    M = use(codec, fec, "lrc", k, m)
    rng = np.random.default_rng(9)
    pats, sing = cu.check_8_4("lrc", prow(fec, "lrc", k, m))
    pres = np.concatenate([pats[rng.choice(len(pats), size=200, replace=False)], cu.patterns(12, 8, [5])[:8]])
    B = len(pres)
    lens = rng.choice(np.array([16, 40, 1202], dtype=np.int32), size=B)
    sh = np.zeros((B, n, S), dtype=np.uint8)
    for b in range(B):
        sh[b, :k, :lens[b]] = rng.integers(0, 256, (k, lens[b]), dtype=np.uint8)
        sh[b, k:, :lens[b]] = cu.encode(M, sh[b, :k, :lens[b]])
    dmg = damage(sh, pres)
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_ragged(k, m, d, i32(torch, words1(pres)), dev(torch, lens), status=st)
    rc = codec.lib_sync_rc()
    want_st, which = expect(M, pres)
    assert (want_st == SINGULAR).any() and (want_st == 0).any()
    ref = dmg.copy()
    for b, i in zip(*np.nonzero(which)):
        ref[b, i, :lens[b]] = sh[b, i, :lens[b]]
        ref[b, i, lens[b]:rup16(lens[b])] = 0
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert np.array_equal(d.cpu().numpy(), ref)
    assert rc == TOO_FEW


@pytest.mark.parametrize("L", [16, 40, 1202])
def test_host_encode_and_reconstruct_lrc(codec, fec, L):
    # FEC_HOST: the staging pipeline around the same device cores; stride == shard_len
    k, m, B = 8, 4, 100
    M = use(codec, fec, "lrc", k, m)
    rng = np.random.default_rng(L)
    want = codewords(M, B, L, L, 10).copy()
    sh = want.copy()
    sh[:, k:] = STALE
    codec.rs_encode(k, m, sh)
    assert np.array_equal(sh, want)
    pats, sing = cu.check_8_4("lrc", prow(fec, "lrc", k, m))
    pres = pats[rng.choice(len(pats), size=B, replace=False)]
    want_st, which = expect(M, pres)
    assert (want_st == SINGULAR).any() and (want_st == 0).any()
    got = damage(want, pres)
    st = np.full(B, 7, dtype=np.int32)
    assert codec.rs_reconstruct(k, m, got, words1(pres), status=st) == fec.FEC_ERR_SINGULAR
    assert np.array_equal(st, want_st)
    ref = damage(want, pres)
    ref[which] = want[which]
    assert np.array_equal(got, ref)
    # with a too-few block among them the call says too few
    pres2 = pres.copy()
    pres2[0] = True
    pres2[0, :5] = False
    got = damage(want, pres2)
    assert codec.rs_reconstruct(k, m, got, words1(pres2), status=st) == fec.FEC_ERR_TOO_FEW_SHARDS
    assert st[0] == TOO_FEW and np.array_equal(st[1:], want_st[1:])


# ------------------------------------------------------------------ 6. kinds queued back to back
def test_kinds_queued_without_a_sync(fec, torch):
    k, m, n, B, L = 8, 4, 12, 300, 1216
    rng = np.random.default_rng(66)
    Pc, Pl = prow(fec, "cauchy255", k, m), prow(fec, "lrc", k, m)
    Mc, Ml, M0 = cu.matrix(Pc), cu.matrix(Pl), fec.rs_matrix(k, m)
    pats, _ = cu.check_8_4("lrc", Pl)
    pres = pats[rng.choice(len(pats), size=B, replace=False)]
    shl, shc = codewords(Ml, B, L, L, 11), codewords(Mc, B, L, L, 12)
    data = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    c = fec.Codec(0).use_torch_stream()
    try:
        d = dev(torch, data)
        p = [torch.zeros((B, m, L), dtype=torch.uint8, device="cuda") for _ in range(4)]
        st = [torch.full((B,), 99, dtype=torch.int32, device="cuda") for _ in range(2)]
        masks = i32(torch, words1(pres))
        dl, dc = dev(torch, damage(shl, pres)), dev(torch, damage(shc, pres))
        c.set_custom_matrix(k, m, Pc)
        c.rs_encode_split(k, m, d, p[0])
        c.set_matrix(0)
        assert c.matrix == "vandermonde"
        c.rs_encode_split(k, m, d, p[1])
        c.set_custom_matrix(k, m, Pl)
        c.rs_encode_split(k, m, d, p[2])
        c.rs_reconstruct(k, m, dl, masks, status=st[0], shard_len=L)
        c.set_matrix("custom")
        assert c.matrix == "custom"
        c.rs_encode_split(k, m, d, p[3])
        c.set_custom_matrix(k, m, Pc)
        c.rs_reconstruct(k, m, dc, masks, status=st[1], shard_len=L)
        rc = c.lib_sync_rc()
        enc = [cu.encode(M, data) for M in (Mc, M0, Ml)]
        assert len({e.tobytes() for e in enc}) == 3
        for got, want in zip(p, [enc[0], enc[1], enc[2], enc[2]]):
            assert np.array_equal(got.cpu().numpy(), want)
        stl, whichl = expect(Ml, pres)
        stc, whichc = expect(Mc, pres)
        assert (stl == SINGULAR).any() and (stc == 0).all() and rc == SINGULAR
        assert np.array_equal(st[0].cpu().numpy(), stl) and np.array_equal(st[1].cpu().numpy(), stc)
        assert np.array_equal(dl.cpu().numpy(), rebuilt(damage(shl, pres), shl, L, whichl))
        assert np.array_equal(dc.cpu().numpy(), rebuilt(damage(shc, pres), shc, L, whichc))
    finally:
        c.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_under_kind_custom(fec, torch):
    rng = np.random.default_rng(7)
    c = fec.Codec(0).use_torch_stream()
    try:
        M = use(c, fec, "cauchy255", 8, 4)
        use(c, fec, "cauchy255", 33, 7)
        B, L = 5, 64

        def refused(call):
            with pytest.raises(fec.FecError) as e:
                call()
            assert e.value.code == fec.FEC_ERR_NO_MATRIX

        wide = dev(torch, rng.integers(0, 256, (B, 40, L), dtype=np.uint8))
        wmask = dev(torch, fec.wide_masks(np.ones((B, 40), dtype=bool)).view(np.int32))
        out = torch.zeros((B, 7, L), dtype=torch.uint8, device="cuda")
        st = torch.zeros((B,), dtype=torch.int32, device="cuda")
        refused(lambda: c.rs_reconstruct_wide(33, 7, wide, wmask, status=st))
        refused(lambda: c.rs_recover_wide_split(33, 7, wide[:, :33].contiguous(), wide[:, 33:].contiguous(), wmask,
                                                out, status=st))
        refused(lambda: c.rs_reconstruct_some_wide(33, 7, wide, wmask, status=st))
        sh = dev(torch, codewords(M, B, L, L, 13))
        nmask = dev(torch, fec.wide_masks(np.ones((B, 12), dtype=bool)).view(np.int32))
        refused(lambda: c.rs_locate(8, 4, sh, st))
        refused(lambda: c.rs_locate_multi(8, 4, sh, st))
        refused(lambda: c.rs_locate_partial(8, 4, sh, nmask, st))
        refused(lambda: c.rs_encode(5, 3, dev(torch, np.zeros((B, 8, L), dtype=np.uint8))))   # nothing registered
        assert c.lib_sync_rc() == 0
        # the ctx keeps working: an encode and a reconstruct under the registered matrix
        full = codewords(M, B, L, L, 13)
        z = full.copy()
        z[:, 8:] = STALE
        d = dev(torch, z)
        c.rs_encode(8, 4, d)
        c.sync()
        assert np.array_equal(d.cpu().numpy(), full)
        pres = np.ones((B, 12), dtype=bool)
        pres[:, [1, 6, 9]] = False
        run_inplace(c, torch, 8, 4, full, pres, L, M)
        # and the built-in kinds serve those calls again
        c.set_matrix(0)
        c.rs_locate(8, 4, sh, st)
        c.sync()
    finally:
        c.close()
