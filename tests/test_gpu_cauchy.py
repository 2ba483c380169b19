"""The Cauchy matrix kind (include/fec_hip_matrix.h, fec_ctx_set_matrix) through every RS call of the
device ABI, byte for byte against the definition model (tests/cauchy_model.py: the matrix from its
definition, parity by table lookups, rebuilds by Gaussian elimination). Whole images are compared:
rebuilt slots carry zeros up to the 16-byte boundary, everything else keeps what it held.

Beside each case, the branch of fec_cores.cpp's dispatch that it reaches."""
import numpy as np
import pytest

import cauchy_model as cm
import cauchy_oracle
from arena import gf, torch  # noqa: F401
from locate_model import UNKNOWN, model_batch

pytestmark = pytest.mark.gpu

FILL = 0x5A        # what a missing shard's slot holds
STALE = 0xA5       # what an output slot holds before the call


@pytest.fixture(scope="module")
def codec(fec):
    c = fec.Codec(0, matrix="cauchy").use_torch_stream()
    assert c.matrix == "cauchy"
    yield c
    c.close()


_M = {}


def mat(k, m):
    if (k, m) not in _M:
        _M[k, m] = cm.matrix(k, m)
    return _M[k, m]


def rup16(x):
    return (x + 15) // 16 * 16


def codewords(rng, M, B, L, S):
    """[B, n, S]: random data and the model's parity in bytes [0, L), zeros behind."""
    n, k = M.shape
    sh = np.zeros((B, n, S), dtype=np.uint8)
    sh[:, :k, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    sh[:, k:, :L] = cm.encode(M, sh[:, :k, :L])
    return sh


def lose(rng, B, n, counts, among=None):
    """bool [B, n] present: block b misses counts[b] shards drawn from `among` (default: all n)."""
    pres = np.ones((B, n), dtype=bool)
    among = np.arange(n) if among is None else np.asarray(among)
    for b in range(B):
        pres[b, rng.choice(among, size=int(counts[b]), replace=False)] = False
    return pres


def words1(pres):
    """uint32 [B] masks of the narrow calls."""
    return (pres.astype(np.uint64) << np.arange(pres.shape[1], dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def damage(sh, pres):
    d = sh.copy()
    d[~pres] = FILL
    return d


def rebuilt(dmg, sh, pres, L, which):
    """The image after a rebuild in place: shard i of block b, where which[b, i], holds the codeword's
    bytes [0, L) and zeros up to the 16-byte boundary; every other byte is as it was."""
    ref = dmg.copy()
    b, i = np.nonzero(which)
    ref[b, i, :L] = sh[b, i, :L]
    ref[b, i, L:rup16(L)] = 0
    return ref


def check_model_rebuild(M, dmg, sh, pres, L, blocks=3):
    """The codeword is what the model's Gaussian elimination gives from the present shards."""
    for b in range(min(blocks, dmg.shape[0])):
        if pres[b].sum() >= M.shape[1]:
            assert np.array_equal(cm.rebuild(M, dmg[b, :, :L], pres[b]), sh[b, :, :L])


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(torch, a):
    return dev(torch, np.ascontiguousarray(a).view(np.int32))


# ------------------------------------------------------------------ encode
ENCODES = [
    # generic kernel, tables in LDS, a 2-byte tail chunk
    (5, 3, 50, 64, 67),
    # generic kernel, tables not in LDS (m * k > 2048)
    (140, 16, 33, 48, 5),
    # m > 16: two passes of parity rows
    (100, 20, 33, 48, 5),
    # rs_encode_bits_cauchy_kernel<16, 8, SP> / <20, 10, SP>: an odd item count, so the last lane pair is
    # half empty
    (16, 8, 1202, 1216, 37),
    (20, 10, 1202, 1216, 37),
    # the generic kernel: the Cauchy row 8e f4 must not take rs_encode23 (written for 03 02)
    (2, 1, 1202, 1216, 129),
    # the dyadic rs_encode_fixed_kernel<8, 4> from the Cauchy leaf tables
    (8, 4, 1202, 1216, 300),
]


@pytest.mark.parametrize("split", [False, True], ids=["interleaved", "split"])
@pytest.mark.parametrize("k,m,L,S,B", ENCODES)
def test_encode(codec, torch, k, m, L, S, B, split):
    # split: parity in a region of its own (sc1 stores in the fixed kernels); interleaved: nt stores
    rng = np.random.default_rng(31 * k + m + L)
    M = mat(k, m)
    want = codewords(rng, M, B, L, S)
    sh = want.copy()
    sh[:, k:] = STALE
    want[:, k:, rup16(L):] = STALE
    if split:
        d, p = dev(torch, sh[:, :k]), dev(torch, sh[:, k:])
        codec.rs_encode_split(k, m, d, p, shard_len=L)
        codec.sync()
        assert np.array_equal(d.cpu().numpy(), want[:, :k])
        assert np.array_equal(p.cpu().numpy(), want[:, k:])
    else:
        d = dev(torch, sh)
        codec.rs_encode(k, m, d, shard_len=L)
        codec.sync()
        assert np.array_equal(d.cpu().numpy(), want)


def test_encode_2_1_is_8e_f4(codec, torch):
    rng = np.random.default_rng(23)
    x = rng.integers(0, 256, (129, 3, 1216), dtype=np.uint8)
    d = dev(torch, x)
    codec.rs_encode(2, 1, d)
    codec.sync()
    assert np.array_equal(d.cpu().numpy()[:, 2], cm.MUL[0x8E][x[:, 0]] ^ cm.MUL[0xF4][x[:, 1]])


# ------------------------------------------------------------------ narrow reconstruct and recover
def run_inplace(codec, torch, k, m, L, S, B, pres, rng):
    M = mat(k, m)
    sh = codewords(rng, M, B, L, S)
    dmg = damage(sh, pres)
    check_model_rebuild(M, dmg, sh, pres, L)
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct(k, m, d, i32(torch, words1(pres)), status=st, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    which = ~pres
    which[:, k:] = False          # reconstruct rebuilds data shards only
    assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, pres, L, which))


def run_recover(codec, torch, k, m, L, S, B, pres, rng, slots):
    M = mat(k, m)
    sh = codewords(rng, M, B, L, S)
    dmg = damage(sh, pres)
    d, p = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, slots, S), STALE, dtype=torch.uint8, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_recover_split(k, m, d, p, i32(torch, words1(pres)), out, status=st, shard_len=L)
    codec.sync()
    e = (~pres[:, :k]).sum(axis=1)
    assert np.array_equal(st.cpu().numpy(), e)
    want = np.full((B, slots, S), STALE, dtype=np.uint8)
    for b in range(B):
        for r, i in enumerate(np.nonzero(~pres[b, :k])[0]):
            want[b, r, :L] = sh[b, i, :L]
            want[b, r, L:rup16(L)] = 0
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(d.cpu().numpy(), dmg[:, :k]) and np.array_equal(p.cpu().numpy(), dmg[:, k:])


# single erasures at 1202 bytes (76 chunks per shard): recover into one slot takes the direct form
# (rs_recover_direct): (8,4) PermTabs in LDS, (20,10) / (16,8) rows from the device table, (2,1) the
# k2m1 kernel, (5,3) runtime k. In place, (8,4) takes the routed kernel's direct body, the others the
# sorted plans' one-erasure row and the wave rebuild / rebuild_k.
@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (16, 8), (2, 1), (5, 3)])
def test_single_erasure(codec, torch, k, m):
    rng = np.random.default_rng(77 * k + m)
    B, L, S = 65, 1202, 1216
    # one data shard lost; in half of the blocks the first parity shards too, so the row used is a later one
    pres = lose(rng, B, k + m, np.ones(B, dtype=int), among=np.arange(k))
    for b in range(0, B, 2):
        pres[b, k:k + int(rng.integers(0, m))] = False
    run_recover(codec, torch, k, m, L, S, B, pres, rng, slots=1)
    run_inplace(codec, torch, k, m, L, S, B, pres, rng)


def test_routed_8_4_in_place(codec, torch):
    # rs_route_classify + rs_plan_sorted (complement form) + rs_reconstruct_routed: 1..4 shards lost per block
    rng = np.random.default_rng(84)
    B = 300
    pres = lose(rng, B, 12, rng.integers(1, 5, B))
    run_inplace(codec, torch, 8, 4, 1202, 1216, B, pres, rng)


# e >= 2 with parity among the missing shards, so the inputs reach past the first present parity:
# len 50 the tile form (rs_plan_kernel + rs_reconstruct_kernel), len 1202 the wave form
# (rs_plan_sorted + wave rebuild; (16,8) / (20,10): rs_plan_code_kernel + rebuild_k)
MULTI = [
    (8, 4), (12, 5),      # sorted plans, complement sums (n - k < k)
    (4, 8), (3, 29),      # sorted plans, direct sums (n - k >= k)
    (16, 8), (20, 10),    # form 3
]


@pytest.mark.parametrize("L,S", [(50, 64), (1202, 1216)])
@pytest.mark.parametrize("k,m", MULTI)
def test_multi_erasure(codec, torch, k, m, L, S):
    rng = np.random.default_rng(1000 * k + m + L)
    B, n = 67, k + m
    emax = min(k, m)
    pres = np.ones((B, n), dtype=bool)
    for b in range(B):
        e = int(rng.integers(2, emax + 1)) if emax >= 2 else 1
        pres[b, rng.choice(k, size=e, replace=False)] = False
        par = int(rng.integers(0, m - e + 1))      # missing parity shards, the first one among them
        if par:
            gone = {k} | set(int(x) for x in rng.choice(np.arange(k, n), size=par, replace=False))
            pres[b, sorted(gone)[:par]] = False
    pres[0, :] = True
    pres[0, :emax] = False                          # the most data shards a block can lose
    run_inplace(codec, torch, k, m, L, S, B, pres, rng)
    run_recover(codec, torch, k, m, L, S, B, pres, rng, slots=emax)


def test_small_batch_block_order_plan(codec, torch):
    # three blocks of short shards: one workgroup of rs_plan_kernel, one tile
    rng = np.random.default_rng(3)
    pres = lose(rng, 3, 12, [2, 3, 4])
    run_inplace(codec, torch, 8, 4, 50, 64, 3, pres, rng)


# ------------------------------------------------------------------ wide calls and reconstruct-some
@pytest.mark.parametrize("k,m", [(33, 7), (100, 156), (128, 128)])
def test_wide_reconstruct_recover_and_some(codec, torch, fec, k, m):
    # rs_plan_wide_kernel<false> (reconstruct, recover) and <true> (reconstruct-some) + the wide tile
    rng = np.random.default_rng(k + m)
    B, L, S, n = 9, 50, 64, k + m
    M = mat(k, m)
    sh = codewords(rng, M, B, L, S)
    pres = lose(rng, B, n, rng.integers(1, m + 1, B))
    pres[0] = True
    pres[0, rng.choice(n, size=m, replace=False)] = False     # m missing
    pres[1] = True
    pres[1, :min(k, m)] = False                               # the first data shards
    dmg = damage(sh, pres)
    check_model_rebuild(M, dmg, sh, pres, L, blocks=2)
    masks = dev(torch, fec.wide_masks(pres).view(np.int32))
    data_lost = ~pres
    data_lost[:, k:] = False
    # in place
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_wide(k, m, d, masks, status=st, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, pres, L, data_lost))
    # recover
    slots = min(k, m)
    dd, pp = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, slots, S), STALE, dtype=torch.uint8, device="cuda")
    codec.rs_recover_wide_split(k, m, dd, pp, masks, out, status=st, shard_len=L)
    codec.sync()
    assert np.array_equal(st.cpu().numpy(), data_lost.sum(axis=1))
    got = out.cpu().numpy()
    for b in range(B):
        lost = np.nonzero(data_lost[b])[0]
        for r, i in enumerate(lost):
            assert np.array_equal(got[b, r, :L], sh[b, i, :L]) and not got[b, r, L:rup16(L)].any()
        assert (got[b, len(lost):] == STALE).all() and (got[b, :, rup16(L):] == STALE).all()
    # reconstruct-some: every missing shard, then only the wanted ones (parity among them)
    d = dev(torch, dmg)
    codec.rs_reconstruct_some_wide(k, m, d, masks, status=st, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, pres, L, ~pres))
    want = rng.integers(0, 2, (B, n)).astype(bool)
    want[:, k:] |= ~pres[:, k:] & (np.arange(B)[:, None] % 2 == 0)   # even blocks: all missing parity wanted
    d = dev(torch, dmg)
    codec.rs_reconstruct_some_wide(k, m, d, masks, want=dev(torch, fec.wide_masks(want).view(np.int32)),
                                   status=st, shard_len=L)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, pres, L, ~pres & want))


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10)])
@pytest.mark.parametrize("L,S", [(50, 64), (1202, 1216)])
def test_narrow_reconstruct_some(codec, torch, k, m, L, S):
    # rs_plan_some_kernel + the wide tile: data and parity rebuilt
    rng = np.random.default_rng(k * L)
    B, n = 67, k + m
    M = mat(k, m)
    sh = codewords(rng, M, B, L, S)
    pres = lose(rng, B, n, rng.integers(0, m + 1, B))
    pres[0] = True
    pres[0, k:] = False                  # every parity shard
    pres[1] = True
    pres[1, :min(k, m)] = False
    dmg = damage(sh, pres)
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_some(k, m, d, i32(torch, words1(pres)), status=st, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, pres, L, ~pres))
    want = rng.integers(0, 2, (B, n)).astype(bool)
    d = dev(torch, dmg)
    codec.rs_reconstruct_some(k, m, d, i32(torch, words1(pres)), want=i32(torch, words1(want)), shard_len=L)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), rebuilt(dmg, sh, pres, L, ~pres & want))


# ------------------------------------------------------------------ verify
@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (64, 16)])
def test_verify(codec, torch, fec, k, m):
    # rs_verify_kernel over the Cauchy PermTabs
    rng = np.random.default_rng(k)
    B, L, S, n = 41, 1202, 1216, k + m
    sh = codewords(rng, mat(k, m), B, L, S)
    st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    codec.rs_verify(k, m, dev(torch, sh), st, count=cnt, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 1).all() and int(cnt.cpu()[0]) == 0
    bad = sh.copy()
    flips = {2: (0, 0), 5: (k - 1, L - 1), 17: (k, 600), 40: (n - 1, L - 1)}   # block: (shard, byte)
    for b, (i, x) in flips.items():
        bad[b, i, x] ^= 1 << int(rng.integers(0, 8))
    codec.rs_verify(k, m, dev(torch, bad), st, count=cnt, shard_len=L)
    codec.sync()
    want = np.ones(B, dtype=np.int32)
    want[list(flips)] = 0
    assert np.array_equal(st.cpu().numpy(), want) and int(cnt.cpu()[0]) == len(flips)
    # blocks encoded with the default matrix are not Cauchy codewords
    dflt = sh.copy()
    dflt[:, k:, :L] = cm.encode(fec.rs_matrix(k, m), sh[:, :k, :L])
    codec.rs_verify(k, m, dev(torch, dflt), st, count=cnt, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all() and int(cnt.cpu()[0]) == B


# ------------------------------------------------------------------ update and encode-idx
@pytest.mark.parametrize("k,m", [(8, 4), (100, 4)])
@pytest.mark.parametrize("ncols", ["one", "half"])
def test_update_and_encode_idx(codec, torch, fec, k, m, ncols):
    # rs_update_kernel over the Cauchy PermTabs: the masked columns' difference folded into the parity
    rng = np.random.default_rng(k + len(ncols))
    B, L, S = 19, 200, 208
    M = mat(k, m)
    sh = codewords(rng, M, B, L, S)
    cols = np.zeros((B, k), dtype=bool)
    for b in range(B):
        cols[b, rng.choice(k, size=1 if ncols == "one" else k // 2, replace=False)] = True
    new = sh[:, :k].copy()
    new[:, :, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    after = np.where(cols[:, :, None], new, sh[:, :k])
    masks = dev(torch, fec.wide_masks(cols).view(np.int32))
    d = dev(torch, sh)
    codec.rs_update(k, m, d, dev(torch, new), masks, shard_len=L)
    codec.sync()
    want = sh.copy()                                   # the old data stays; the parity is the new data's
    want[:, k:, :L] = cm.encode(M, after[:, :, :L])
    assert np.array_equal(d.cpu().numpy(), want)
    # encode-idx: the masked columns folded into zeroed parity, then the rest: the whole parity
    z = sh.copy()
    z[:, k:] = 0
    d = dev(torch, z)
    codec.rs_encode_idx(k, m, d, masks, shard_len=L)
    codec.rs_encode_idx(k, m, d, dev(torch, fec.wide_masks(~cols).view(np.int32)), shard_len=L)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), sh)


# ------------------------------------------------------------------ locate family
def planted(rng, sh, L, sets):
    """sh with every byte [0, L) of shard i of block b changed, for b: shards in sets."""
    bad = sh.copy()
    for b, shards in sets.items():
        for i in shards:
            bad[b, i, :L] = cm.corrupt(rng, bad[b, i, :L])
    return bad


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (64, 16), (140, 20)])
def test_locate(codec, torch, fec, k, m):
    # rs_locate_kernel with the table of the Cauchy rows' ratios; (140,20): the carry tables of the second pass
    rng = np.random.default_rng(k * m)
    B, L, S, n = 23, 1202, 1216, k + m
    W = fec.mask_words(n)
    sh = codewords(rng, mat(k, m), B, L, S)
    sets = {1: [0], 4: [k - 1], 9: [k], 15: [n - 1], 22: [int(rng.integers(0, n))]}
    bad = planted(rng, sh, L, sets)
    verdict = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    present = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    counts = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    codec.rs_locate(k, m, dev(torch, bad), verdict, present_out=present, counts=counts, shard_len=L)
    codec.sync()
    want = np.full(B, fec.FEC_LOCATE_CLEAN, dtype=np.int32)
    pres = np.ones((B, n), dtype=bool)
    for b, (i,) in sets.items():
        want[b] = i
        pres[b, i] = False
    assert np.array_equal(verdict.cpu().numpy(), want)
    assert np.array_equal(present.cpu().numpy().view(np.uint32), fec.wide_masks(pres))
    assert counts.cpu().tolist() == [len(sets), 0]


LOCATE_MULTI = [(8, 4, 2), (20, 10, 5), (64, 16, 8)]


@pytest.mark.parametrize("k,m,T", LOCATE_MULTI)
def test_locate_multi(codec, torch, fec, k, m, T):
    # the scan over the Cauchy PermTabs, then the solve over locate_multi_table(log v)
    rng = np.random.default_rng(k + T)
    B, L, S, n = 23, 200, 208, k + m
    W = fec.mask_words(n)
    sh = codewords(rng, mat(k, m), B, L, S)
    others = lambda cnt, base: list(base) + [int(x) for x in rng.choice(   # noqa: E731
        [i for i in range(1, n - 1) if i not in base], size=cnt - len(base), replace=False)]
    sets = {0: [0], 3: [n - 1], 6: [int(rng.integers(1, k))],
            9: others(T, [0]), 12: others(T, [k, n - 1][:T]), 18: others(T, [])}
    bad = planted(rng, sh, L, sets)
    cnt = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    present = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    counts = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    codec.rs_locate_multi(k, m, dev(torch, bad), cnt, max_bad=T, present_out=present, counts=counts, shard_len=L)
    codec.sync()
    want = np.zeros(B, dtype=np.int32)
    pres = np.ones((B, n), dtype=bool)
    for b, shards in sets.items():
        want[b] = len(shards)
        pres[b, shards] = False
    assert np.array_equal(cnt.cpu().numpy(), want)
    assert np.array_equal(present.cpu().numpy().view(np.uint32), fec.wide_masks(pres))
    assert counts.cpu().tolist() == [len(sets), 0]


@pytest.mark.parametrize("k,m,T", LOCATE_MULTI)
@pytest.mark.parametrize("missing", ["one", "half"])
def test_locate_partial_then_heal(codec, torch, fec, k, m, T, missing):
    # the plan (lambda(k + i) per block), the scaled scan and the solve with a present set; then
    # reconstruct-some (narrow: rs_plan_some_kernel; (64,16): rs_plan_wide_kernel<true>) heals the block
    rng = np.random.default_rng(k + T + len(missing))
    B, L, S, n = 23, 200, 208, k + m
    W = fec.mask_words(n)
    e = 1 if missing == "one" else m // 2
    tmax = min(T, (m - e) // 2)
    sh = codewords(rng, mat(k, m), B, L, S)
    pres = lose(rng, B, n, np.full(B, e))
    pres[0] = True
    pres[0, :e] = False                       # shard 0 missing
    sets = {}
    for b, t in {0: 1, 3: tmax, 6: 1, 9: tmax, 14: tmax}.items():
        here = np.nonzero(pres[b])[0]
        pick = [int(x) for x in rng.choice(here, size=t, replace=False)]
        if b == 9:
            pick[0] = int(here[0])            # the first present shard
        if b == 14:
            pick[0] = int(here[-1])           # the last one: a parity shard unless it is missing
        sets[b] = sorted(set(pick))
    bad = planted(rng, damage(sh, pres), L, sets)
    bad[~pres] = FILL
    d = dev(torch, bad)
    masks = dev(torch, fec.wide_masks(pres).view(np.int32))
    cnt = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    present = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    counts = torch.full((3,), 9, dtype=torch.int32, device="cuda")
    codec.rs_locate_partial(k, m, d, masks, cnt, max_bad=T, present_out=present, counts=counts, shard_len=L)
    codec.sync()
    want = np.zeros(B, dtype=np.int32)
    good = pres.copy()
    for b, shards in sets.items():
        want[b] = len(shards)
        good[b, shards] = False
    assert np.array_equal(cnt.cpu().numpy(), want)
    assert np.array_equal(present.cpu().numpy().view(np.uint32), fec.wide_masks(good))
    assert counts.cpu().tolist() == [len(sets), 0, 0]
    # heal: every shard that is missing or located, from the masks the call wrote
    if n <= 32:
        codec.rs_reconstruct_some(k, m, d, present.reshape(B), shard_len=L)
    else:
        codec.rs_reconstruct_some_wide(k, m, d, present, shard_len=L)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), rebuilt(bad, sh, good, L, ~good))
    assert np.array_equal(d.cpu().numpy()[:, :, :L], sh[:, :, :L])


# ------------------------------------------------------------------ ragged
@pytest.mark.parametrize("k,m", [(8, 4), (20, 10)])
def test_ragged_encode_reconstruct_recover(codec, torch, k, m):
    # rs_encode_ragged_kernel; rs_plan_kernel (with log v) + the ragged tile rebuild
    rng = np.random.default_rng(k)
    B, S, n = 64, 1216, k + m
    M = mat(k, m)
    lens = rng.integers(1, 1203, B).astype(np.int32)
    lens[0], lens[1] = 1, 1202
    sh = np.zeros((B, n, S), dtype=np.uint8)
    for b in range(B):
        sh[b, :k, :lens[b]] = rng.integers(0, 256, (k, lens[b]), dtype=np.uint8)
        sh[b, k:, :lens[b]] = cm.encode(M, sh[b, :k, :lens[b]])
    dl = dev(torch, lens)
    enc = sh.copy()
    enc[:, k:] = STALE
    want = sh.copy()
    for b in range(B):
        want[b, k:, rup16(lens[b]):] = STALE
    d = dev(torch, enc)
    codec.rs_encode_ragged(k, m, d, dl)
    codec.sync()
    assert np.array_equal(d.cpu().numpy(), want)
    pres = lose(rng, B, n, rng.integers(0, m + 1, B))
    pres[2] = True
    pres[2, :min(k, m)] = False
    dmg = damage(sh, pres)
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_ragged(k, m, d, i32(torch, words1(pres)), dl, status=st)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    ref = dmg.copy()
    for b in range(B):
        for i in np.nonzero(~pres[b, :k])[0]:
            ref[b, i, :lens[b]] = sh[b, i, :lens[b]]
            ref[b, i, lens[b]:rup16(lens[b])] = 0
    assert np.array_equal(d.cpu().numpy(), ref)
    slots = min(k, m)
    dd, pp = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, slots, S), STALE, dtype=torch.uint8, device="cuda")
    codec.rs_recover_ragged_split(k, m, dd, pp, i32(torch, words1(pres)), dl, out, status=st)
    codec.sync()
    assert np.array_equal(st.cpu().numpy(), (~pres[:, :k]).sum(axis=1))
    wout = np.full((B, slots, S), STALE, dtype=np.uint8)
    for b in range(B):
        for r, i in enumerate(np.nonzero(~pres[b, :k])[0]):
            wout[b, r, :lens[b]] = sh[b, i, :lens[b]]
            wout[b, r, lens[b]:rup16(lens[b])] = 0
    assert np.array_equal(out.cpu().numpy(), wout)


# ------------------------------------------------------------------ host-resident
@pytest.mark.parametrize("pinned", [False, True], ids=["FEC_HOST", "FEC_HOST_PINNED"])
def test_host_resident_encode_and_reconstruct(codec, torch, fec, pinned):
    # host_encode / host_reconstruct_rs: the staging pipeline around the same device cores
    rng = np.random.default_rng(11)
    k, m, B, L = 8, 4, 100, 1202
    M = mat(k, m)
    want = codewords(rng, M, B, L, L)          # packed host layout, stride == shard_len
    sh = want.copy()
    sh[:, k:] = STALE
    masks = words1(lose(rng, B, k + m, rng.integers(0, m + 1, B)))
    pres = np.array([cm.mask_bits(x, k + m) for x in masks])
    st = np.full(B, 7, dtype=np.int32)
    if pinned:
        h = torch.from_numpy(sh).pin_memory()
        codec.rs_encode(k, m, h)
        assert np.array_equal(h.numpy(), want)
        hd = torch.from_numpy(damage(want, pres)).pin_memory()
        hm, hs = torch.from_numpy(masks.view(np.int32)).pin_memory(), torch.from_numpy(st).pin_memory()
        assert codec.rs_reconstruct(k, m, hd, hm, status=hs) == fec.FEC_OK
        got, st = hd.numpy(), hs.numpy()
    else:
        codec.rs_encode(k, m, sh)
        assert np.array_equal(sh, want)
        got = damage(want, pres)
        assert codec.rs_reconstruct(k, m, got, masks, status=st) == fec.FEC_OK
    assert (st == 0).all()
    assert np.array_equal(got[:, :k], want[:, :k])
    assert np.array_equal(got[:, k:], damage(want, pres)[:, k:])


# ------------------------------------------------------------------ kind switching
def test_kind_switches_between_calls_without_a_sync(fec, torch):
    # the code cache is keyed by (kind, k, m): queued launches keep their own code's tables
    rng = np.random.default_rng(99)
    k, m, B, L = 8, 4, 300, 1216
    c = fec.Codec(0).use_torch_stream()
    try:
        assert c.matrix == "vandermonde"
        data = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        d = dev(torch, data)
        p = [torch.zeros((B, m, L), dtype=torch.uint8, device="cuda") for _ in range(3)]
        c.rs_encode_split(k, m, d, p[0])
        c.set_matrix("cauchy")
        assert c.matrix == "cauchy"
        c.rs_encode_split(k, m, d, p[1])
        c.set_matrix(0)
        assert c.matrix == "vandermonde"
        c.rs_encode_split(k, m, d, p[2])
        with pytest.raises(fec.FecError) as e:
            c.set_matrix(5)
        assert e.value.code == fec.FEC_ERR_INVALID_ARG and c.matrix == "vandermonde"
        c.sync()
        dflt, cauchy = cm.encode(fec.rs_matrix(k, m), data), cm.encode(mat(k, m), data)
        assert not np.array_equal(dflt, cauchy)
        assert np.array_equal(p[0].cpu().numpy(), dflt)
        assert np.array_equal(p[1].cpu().numpy(), cauchy)
        assert np.array_equal(p[2].cpu().numpy(), dflt)
        # the XOR calls have no matrix
        x = dev(torch, np.concatenate([data[:, :3], np.zeros((B, 1, L), dtype=np.uint8)], axis=1))
        c.set_matrix("cauchy")
        c.xor_encode(3, x)
        c.sync()
        assert np.array_equal(x.cpu().numpy()[:, 3], data[:, 0] ^ data[:, 1] ^ data[:, 2])
    finally:
        c.close()


def test_kind_switches_between_queued_decode_and_locate_calls(fec, torch, oracle, gf):
    """RS(12,17), 1202-byte shards, a fresh ctx: decode and locate calls of both kinds queued with no sync
    in between. Each kind's code object is built inside the sequence and then used again; the plan
    workspace is shared by all of the calls, and the tables must be those of the kind that was current at
    each launch. The data multipliers of this code differ (1, 103, ...), so a Cauchy plan computed with
    kind 0's tables, or the reverse, gives other bytes."""
    rng = np.random.default_rng(1217)
    k, m, B, L, S = 12, 5, 67, 1202, 1216
    n, T = k + m, m // 2
    v = cauchy_oracle.code_multipliers(k, m)
    assert len(set(v[:k].tolist())) > 1
    # the two prepared batches: the oracle's codewords and the Cauchy model's, of the same data
    shC = codewords(rng, mat(k, m), B, L, S)
    sh0 = shC.copy()
    oracle.rs_encode(k, m, sh0)
    assert not sh0[:, :, L:].any() and not np.array_equal(sh0[:, k:], shC[:, k:])
    pres0 = lose(rng, B, n, rng.integers(0, m + 1, B))
    presC = lose(rng, B, n, rng.integers(0, m + 1, B))
    pres0[0], presC[0] = True, True
    pres0[0, :m], presC[0, :m] = False, False          # the first data shards: every input past them
    presC[1] = True
    presC[1, [0, 5, k]] = False                       # data shards of both multipliers and a parity shard
    dmg0, dmgC = damage(sh0, pres0), damage(shC, presC)
    # the corrupted Cauchy batch: single bytes in t shards of a block, t = b % 4 (3 is past the radius: the
    # code has distance 6, so three errors are never within 2 of another codeword)
    bad = shC.copy()
    hit = [sorted(int(s) for s in rng.choice(n, size=b % 4, replace=False)) for b in range(B)]
    for b in range(B):
        for j, s in enumerate(hit[b]):
            bad[b, s, [0, L - 1, int(rng.integers(L))][(b + j) % 3]] ^= int(rng.integers(1, 256))
    want4, sets4 = model_batch(gf, k, m, bad, L, 8, v=v)
    assert [int(x) for x in want4] == [len(h) if len(h) <= T else UNKNOWN for h in hit]
    assert all(sets4[b] == frozenset(hit[b]) for b in range(B) if len(hit[b]) <= T)
    want7, _ = model_batch(gf, k, m, bad, L, 8)        # to kind 0 the Cauchy codewords are no codewords
    assert (want7 == UNKNOWN).all()
    good = np.ones((B, n), dtype=bool)
    for b in np.flatnonzero(want4 > 0):
        good[b, sorted(sets4[b])] = False

    c = fec.Codec(0).use_torch_stream()
    try:
        # every buffer is on the device before the first call, so no copy waits between the calls
        d1, d3, dbad = dev(torch, dmg0), dev(torch, dmgC), dev(torch, bad)
        d6, p6 = dev(torch, dmg0[:, :k]), dev(torch, dmg0[:, k:])
        mk0, mkC = i32(torch, words1(pres0)), i32(torch, words1(presC))
        st = [torch.full((B,), 99, dtype=torch.int32, device="cuda") for _ in range(4)]
        cnt4, cnt7 = (torch.full((B,), 99, dtype=torch.int32, device="cuda") for _ in range(2))
        pm4, pm7 = (torch.full((B, 1), 0x5EED, dtype=torch.int32, device="cuda") for _ in range(2))
        two4, two7 = (torch.full((2,), 9, dtype=torch.int32, device="cuda") for _ in range(2))
        out6 = torch.full((B, m, S), STALE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert c.matrix == "vandermonde"
        c.rs_reconstruct(k, m, d1, mk0, status=st[0], shard_len=L)                              # 1
        c.set_matrix("cauchy")                                                                  # 2
        c.rs_reconstruct(k, m, d3, mkC, status=st[1], shard_len=L)                              # 3
        c.rs_locate_multi(k, m, dbad, cnt4, present_out=pm4, counts=two4, shard_len=L)          # 4
        c.set_matrix(0)                                                                         # 5
        c.rs_recover_split(k, m, d6, p6, mk0, out6, status=st[2], shard_len=L)                  # 6
        c.rs_locate_multi(k, m, dbad, cnt7, present_out=pm7, counts=two7, shard_len=L)          # 7
        c.set_matrix("cauchy")                                                                  # 8
        c.rs_reconstruct_some(k, m, dbad, pm4.reshape(B), status=st[3], shard_len=L)
        c.sync()
        assert c.matrix == "cauchy"
        lost0, lostC = ~pres0, ~presC
        lost0[:, k:], lostC[:, k:] = False, False
        assert (st[0].cpu().numpy() == 0).all()
        assert np.array_equal(d1.cpu().numpy(), rebuilt(dmg0, sh0, pres0, L, lost0))
        assert (st[1].cpu().numpy() == 0).all()
        assert np.array_equal(d3.cpu().numpy(), rebuilt(dmgC, shC, presC, L, lostC))
        assert np.array_equal(cnt4.cpu().numpy(), want4)
        assert np.array_equal(pm4.cpu().numpy().view(np.uint32).reshape(B), words1(good))
        assert two4.cpu().tolist() == [int((want4 > 0).sum()), int((want4 == UNKNOWN).sum())]
        assert np.array_equal(st[2].cpu().numpy(), lost0.sum(axis=1))
        wout = np.full((B, m, S), STALE, dtype=np.uint8)
        for b in range(B):
            for r, i in enumerate(np.nonzero(lost0[b])[0]):
                wout[b, r, :L] = sh0[b, i, :L]
                wout[b, r, L:rup16(L)] = 0
        assert np.array_equal(out6.cpu().numpy(), wout)
        assert np.array_equal(d6.cpu().numpy(), dmg0[:, :k]) and np.array_equal(p6.cpu().numpy(), dmg0[:, k:])
        got7 = cnt7.cpu().numpy()
        assert (got7 != 0).all() and np.array_equal(got7, want7)
        assert (pm7.cpu().numpy().view(np.uint32) == (1 << n) - 1).all() and two7.cpu().tolist() == [0, B]
        assert (st[3].cpu().numpy() == 0).all()
        healed = d = dbad.cpu().numpy()
        assert np.array_equal(healed, rebuilt(bad, shC, good, L, ~good))
        ok = want4 >= 0
        assert ok.sum() > B // 2 and np.array_equal(d[ok], shC[ok]) and np.array_equal(d[~ok], bad[~ok])
    finally:
        c.close()
