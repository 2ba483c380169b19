"""Every erasure pattern under the Cauchy code (a ctx with FEC_MATRIX_CAUCHY), one block per pattern,
through each form of the decode plans. The expected bytes are the codeword itself (random data, parity
from cauchy_model.encode), so the device side needs no decoding model: missing slots hold FILL, output
slots start as STALE, and whole images are compared: a rebuilt slot holds the codeword in [0, L) and
zeros up to the 16-byte boundary, every other byte is untouched. Statuses: 0 for every block of a
reconstruct, the number of lost data shards for a recover.

Why these codes (test_cauchy_oracle.py, cauchy_oracle.multipliers): the decode adds log v_o - log v_s
per output o and input s. Where k is a power of two, (8,4), (4,8), (16,8), all data shards have one
multiplier (and all parity shards of (8,4) and (16,8) another), so a wrong term shows only in patterns
whose inputs include parity; the exhaustive lists hold every such pattern. In (5,3), (12,5), (20,10)
and (33,7) the data multipliers differ among themselves.

"All <= e": every subset of the n shards of size 0 .. e is lost. Every pattern is decodable and none
is left out on the device. Beside each case, the branch of fec_cores.cpp's dispatch that it reaches
(cps = chunks per shard: 50 bytes 4, 200 bytes 13, 520 bytes 33, the smallest past the 32 of
wave_recon_applies with an 8-byte tail, 1202 bytes 76, past the 64 of rebuild_k_applies).

The pattern lists are checked without a device at the end of this module.
"""
import itertools

import numpy as np
import pytest

import cauchy_model as cm
import cauchy_oracle
from arena import torch  # noqa: F401
from test_gpu_cauchy import FILL, STALE, codec, damage, dev, i32, mat, rup16, words1  # noqa: F401

gpu = pytest.mark.gpu

_PATTERNS = {}


def all_le(n, e):
    """bool [N, n] present: every subset of at most e of the n shards lost, by size, then in order."""
    key = ("all", n, e)
    if key not in _PATTERNS:
        pres = np.ones((sum(1 for s in range(e + 1) for _ in itertools.combinations(range(n), s)), n), dtype=bool)
        b = 0
        for s in range(e + 1):
            for lost in itertools.combinations(range(n), s):
                pres[b, list(lost)] = False
                b += 1
        pres.setflags(write=False)
        _PATTERNS[key] = pres
    return _PATTERNS[key]


def drawn(k, m, count, extremes=True):
    """All <= 2, then `count` patterns of 3 .. m lost shards drawn with a fixed seed, then the first
    min(k, m) data shards, and all parity shards but the last with data shard k - 1."""
    key = ("drawn", k, m, count)
    if key not in _PATTERNS:
        n = k + m
        rng = np.random.default_rng(1000 * k + m)
        more = np.ones((count + 2, n), dtype=bool)
        for b in range(count):
            more[b, rng.choice(n, size=int(rng.integers(3, m + 1)), replace=False)] = False
        more[count, :min(k, m)] = False
        more[count + 1, k:n - 1] = False
        more[count + 1, k - 1] = False
        pres = np.concatenate([all_le(n, 2), more if extremes else more[:count]])
        pres.setflags(write=False)
        _PATTERNS[key] = pres
    return _PATTERNS[key]


def patterns(k, m):
    """The pattern list of a code."""
    if (k, m) in ((16, 8), (20, 10)):
        return drawn(k, m, 1500)
    if (k, m) == (33, 7):
        return drawn(k, m, 500, extremes=False)
    return all_le(k + m, m)


def codewords(rng, M, B, lens, S):
    """[B, n, S]: random data and the model's parity in bytes [0, lens[b]), zeros behind."""
    n, k = M.shape
    L = int(np.max(lens))
    sh = np.zeros((B, n, S), dtype=np.uint8)
    sh[:, :k, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    sh[:, :k, :L] *= np.arange(L)[None, None, :] < np.asarray(lens).reshape(-1, 1, 1)
    sh[:, k:, :L] = cm.encode(M, sh[:, :k, :L])
    return sh


def rebuilt(dmg, sh, lens, which):
    """The image after a rebuild in place: shard i of block b, where which[b, i], holds the codeword's
    bytes [0, lens[b]) and zeros up to the 16-byte boundary (sh holds zeros there); every other byte is
    as it was."""
    upto = rup16(np.asarray(lens)).reshape(-1, 1, 1)
    sel = which[:, :, None] & (np.arange(dmg.shape[2])[None, None, :] < upto)
    return np.where(sel, sh, dmg)


def recovered(sh, pres, k, lens, slots):
    """[B, slots, S]: slot r of block b holds its r-th lost data shard as `rebuilt` does, the rest STALE."""
    B, _, S = sh.shape
    lost = ~pres[:, :k]
    assert lost.sum(axis=1).max() <= slots
    b, i = np.nonzero(lost)
    r = (np.cumsum(lost, axis=1) - 1)[b, i]
    upto = rup16(np.asarray(lens)).reshape(-1, 1) * np.ones((B, 1), dtype=np.int64)
    cols = np.arange(S)[None, :] < upto[b]
    want = np.full((B, slots, S), STALE, dtype=np.uint8)
    want[b, r] = np.where(cols, sh[b, i], STALE)
    return want


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d bytes differ, first at (block, shard, byte) %s, %d blocks" % (
            what, len(bad), bad[0].tolist(), len(np.unique(bad[:, 0]))))


def run_narrow(codec, torch, k, m, L, pres, slots, rng):
    """Reconstruct in place, then recover into `slots` slots, over one block per pattern."""
    M = mat(k, m)
    B, S = len(pres), rup16(L) + 16
    sh = codewords(rng, M, B, L, S)
    dmg = damage(sh, pres)
    masks = i32(torch, words1(pres))
    lost_data = ~pres
    lost_data[:, k:] = False
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct(k, m, d, masks, status=st, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    same(d.cpu().numpy(), rebuilt(dmg, sh, L, lost_data), "in place")
    run_recover(codec, torch, k, m, L, sh, dmg, pres, slots)
    return sh, dmg


def run_recover(codec, torch, k, m, L, sh, dmg, pres, slots):
    B, _, S = sh.shape
    d, p = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, slots, S), STALE, dtype=torch.uint8, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_recover_split(k, m, d, p, i32(torch, words1(pres)), out, status=st, shard_len=L)
    codec.sync()
    assert np.array_equal(st.cpu().numpy(), (~pres[:, :k]).sum(axis=1))
    same(out.cpu().numpy(), recovered(sh, pres, k, L, slots), "recover into %d slots" % slots)
    assert np.array_equal(d.cpu().numpy(), dmg[:, :k]) and np.array_equal(p.cpu().numpy(), dmg[:, k:])


NARROW = [
    # in place: rs_route_classify + rs_plan_sorted (complement sums through dall) + rs_reconstruct_routed;
    # recover with 4 slots: rs_plan_sorted + the wave rebuild
    (8, 4, 1202),
    # block-order rs_plan_kernel + the tile rebuild
    (8, 4, 50),
    # runtime k, data multipliers all different. 50: rs_plan_kernel; 520: sorted plans, complement sums
    # (n - k < k), the wave rebuild
    (5, 3, 50), (5, 3, 520),
    # complement sums with unequal data multipliers (1, 103, ...)
    (12, 5, 50), (12, 5, 520),
    # n - k >= k: the sorted plans' direct sums, `else if (a.logv)`; at most 4 data shards can be lost
    (4, 8, 50), (4, 8, 520),
    # form 3: rs_plan_code_kernel + rs_rebuild_k_kernel (76 chunks >= 64)
    (16, 8, 1202), (20, 10, 1202),
    # the same lists through the block-order plans
    (16, 8, 50), (20, 10, 50),
]


@gpu
@pytest.mark.parametrize("k,m,L", NARROW)
def test_every_pattern_in_place_and_recover(codec, torch, k, m, L):
    rng = np.random.default_rng(10000 * k + 100 * m + L)
    pres = patterns(k, m)
    sh, dmg = run_narrow(codec, torch, k, m, L, pres, min(k, m), rng)
    if (k, m, L) == (8, 4, 1202):
        # one output slot: rs_recover_direct (direct_recon_applies: single slot, 76 chunks >= 32), on the
        # patterns with one data shard lost, whatever parity is lost beside it
        one = (~pres[:, :k]).sum(axis=1) == 1
        assert one.sum() == 8 * (1 + 4 + 6 + 4)
        run_recover(codec, torch, k, m, L, sh[one], dmg[one], pres[one], 1)


@gpu
def test_every_pattern_wide_33_7(codec, torch, fec):
    # rs_plan_wide_kernel<false> (reconstruct, recover) and <true> (reconstruct-some) with wide_logsum, and
    # the wide tile; 33 data multipliers, all different
    k, m, L = 33, 7, 50
    rng = np.random.default_rng(337)
    pres = patterns(k, m)
    B, S = len(pres), rup16(L) + 16
    sh = codewords(rng, mat(k, m), B, L, S)
    dmg = damage(sh, pres)
    masks = dev(torch, fec.wide_masks(pres).view(np.int32))
    lost_data = ~pres
    lost_data[:, k:] = False
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    d = dev(torch, dmg)
    codec.rs_reconstruct_wide(k, m, d, masks, status=st, shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    same(d.cpu().numpy(), rebuilt(dmg, sh, L, lost_data), "wide in place")
    dd, pp = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, m, S), STALE, dtype=torch.uint8, device="cuda")
    st.fill_(99)
    codec.rs_recover_wide_split(k, m, dd, pp, masks, out, status=st, shard_len=L)
    codec.sync()
    assert np.array_equal(st.cpu().numpy(), lost_data.sum(axis=1))
    same(out.cpu().numpy(), recovered(sh, pres, k, L, m), "wide recover")
    assert np.array_equal(dd.cpu().numpy(), dmg[:, :k]) and np.array_equal(pp.cpu().numpy(), dmg[:, k:])
    d = dev(torch, dmg)
    st.fill_(99)
    codec.rs_reconstruct_some_wide(k, m, d, masks, status=st, shard_len=L)      # every missing shard
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    same(d.cpu().numpy(), rebuilt(dmg, sh, L, ~pres), "wide reconstruct-some")


@gpu
def test_every_pattern_and_want_mask_reconstruct_some_5_3(codec, torch):
    # rs_plan_some_kernel + the wide tile: every decodable pattern x every want mask; parity shards are
    # rebuilt under their own multiplier v_o, from inputs that include parity
    k, m, L = 5, 3, 50
    n = k + m
    rng = np.random.default_rng(53)
    base = patterns(k, m)
    assert len(base) == 93
    pres = np.repeat(base, 256, axis=0)
    want = np.tile(((np.arange(256)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool), (len(base), 1))
    B, S = len(pres), rup16(L) + 16
    sh = codewords(rng, mat(k, m), B, L, S)
    dmg = damage(sh, pres)
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_some(k, m, d, i32(torch, words1(pres)), want=i32(torch, words1(want)), status=st,
                              shard_len=L)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    same(d.cpu().numpy(), rebuilt(dmg, sh, L, ~pres & want), "reconstruct-some with want")


@gpu
def test_every_pattern_ragged_12_5(codec, torch):
    # rs_plan_kernel (with log v) + the ragged tile rebuild; the lengths cycle over the blocks, so each
    # meets every residue of the pattern index
    k, m, L = 12, 5, 200
    rng = np.random.default_rng(125)
    pres = patterns(k, m)
    B, S = len(pres), rup16(L) + 16
    lens = np.array([1, 15, 16, 17, 199, 200], dtype=np.int32)[np.arange(B) % 6]
    sh = codewords(rng, mat(k, m), B, lens, S)
    dmg = damage(sh, pres)
    dl = dev(torch, lens)
    masks = i32(torch, words1(pres))
    lost_data = ~pres
    lost_data[:, k:] = False
    d = dev(torch, dmg)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_ragged(k, m, d, masks, dl, status=st)
    codec.sync()
    assert (st.cpu().numpy() == 0).all()
    same(d.cpu().numpy(), rebuilt(dmg, sh, lens, lost_data), "ragged in place")
    dd, pp = dev(torch, dmg[:, :k]), dev(torch, dmg[:, k:])
    out = torch.full((B, m, S), STALE, dtype=torch.uint8, device="cuda")
    st.fill_(99)
    codec.rs_recover_ragged_split(k, m, dd, pp, masks, dl, out, status=st)
    codec.sync()
    assert np.array_equal(st.cpu().numpy(), lost_data.sum(axis=1))
    same(out.cpu().numpy(), recovered(sh, pres, k, lens, m), "ragged recover")
    assert np.array_equal(dd.cpu().numpy(), dmg[:, :k]) and np.array_equal(pp.cpu().numpy(), dmg[:, k:])


# ------------------------------------------------------------------ the lists, without a device
COUNTS = {(8, 4): 794, (5, 3): 93, (12, 5): 9402, (4, 8): 3797, (16, 8): 1 + 24 + 276 + 1502,
          (20, 10): 1 + 30 + 435 + 1502, (33, 7): 1 + 40 + 780 + 500}


@pytest.mark.parametrize("k,m", sorted(COUNTS))
def test_every_listed_pattern_is_decodable(k, m):
    """For each distinct set S of the first k present shards of the list, cauchy_model.decode_rows
    finds M[S] invertible (it asserts so); no pattern twice in the exhaustive part; for 50 sampled
    patterns the model's rebuild returns the codeword; the helpers of this module on a small case."""
    M = mat(k, m)
    n = k + m
    pres = patterns(k, m)
    assert pres.shape == (COUNTS[k, m], n)
    lost = (~pres).sum(axis=1)
    assert lost.max() == m and lost.min() == 0 and (pres.sum(axis=1) >= k).all()
    nall = len(all_le(n, m if (k, m) not in ((16, 8), (20, 10), (33, 7)) else 2))
    assert len({row.tobytes() for row in pres[:nall]}) == nall
    firsts = {tuple(np.nonzero(row)[0][:k]) for row in pres}
    for S in firsts:
        row = np.zeros(n, dtype=bool)
        row[list(S)] = True
        got, T = cm.decode_rows(M, row)
        assert tuple(got) == S and np.array_equal(T[list(S)], np.eye(k, dtype=np.uint8))
    assert any(max(S) >= k for S in firsts), "inputs among the parity shards"
    # the term log v_o - log v_s does not cancel: patterns with a lost data shard o and an input s of
    # another multiplier, among the parity inputs in every code, among the data inputs where k is no
    # power of two
    v = cauchy_oracle.code_multipliers(k, m)
    mixed = {"data": 0, "parity": 0}
    for row in pres:
        S = np.nonzero(row)[0][:k]
        for o in np.nonzero(~row[:k])[0]:
            mixed["data"] += bool((v[S[S < k]] != v[o]).any())
            mixed["parity"] += bool((v[S[S >= k]] != v[o]).any())
    assert mixed["parity"] >= len(pres) // 2
    assert (mixed["data"] > 0) == bool(k & (k - 1)), mixed
    rng = np.random.default_rng(k + m)
    sh = codewords(rng, M, 1, 19, 32)[0]
    for b in rng.choice(len(pres), size=50, replace=False):
        assert np.array_equal(cm.rebuild(M, np.where(pres[b][:, None], sh, FILL)[:, :19], pres[b]), sh[:, :19])


def test_expected_images():
    rng = np.random.default_rng(2)
    k, m, S = 3, 2, 48
    pres = np.array([[1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [1, 1, 0, 0, 1]], dtype=bool)
    lens = np.array([17, 1, 32])
    sh = codewords(rng, mat(k, m), 3, lens, S)
    for b in range(3):
        assert not sh[b, :, lens[b]:].any() and sh[b, :, :lens[b]].any()
        assert np.array_equal(sh[b, k:, :lens[b]], cm.encode(mat(k, m), sh[b, :k, :lens[b]]))
    dmg = damage(sh, pres)
    ref = rebuilt(dmg, sh, lens, ~pres)
    assert np.array_equal(ref[0], dmg[0])
    assert np.array_equal(ref[1, 0, :16], sh[1, 0, :16]) and (ref[1, 0, 16:] == FILL).all()
    assert np.array_equal(ref[2, 2, :32], sh[2, 2, :32]) and (ref[2, 3, 32:] == FILL).all()
    out = recovered(sh, pres, k, lens, 2)
    assert (out[0] == STALE).all()
    assert np.array_equal(out[1, 0, :16], sh[1, 0, :16]) and np.array_equal(out[1, 1, :16], sh[1, 2, :16])
    assert (out[1, :, 16:] == STALE).all()
    assert np.array_equal(out[2, 0, :32], sh[2, 2, :32]) and (out[2, 1] == STALE).all()
    assert np.array_equal(rebuilt(dmg, sh, 32, ~pres)[2, 3, :32], sh[2, 3, :32])
