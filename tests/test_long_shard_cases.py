"""The cases of test_gpu_long_shards.py (long_shard_cases.py), built without a device: what the device
tests rest on. Every length has more than 256 chunks, a chunk count that is no multiple of 64 and a
partial tail; every narrow batch holds all the block kinds its code can have; the oracle's reconstruct
gives back the original data of every recoverable block and leaves the others as they were; the wide
cases hold a block with more than 16 lost data shards where they say so; no case builds a host array
of 256 MB.
"""
import numpy as np
import pytest

import long_shard_cases as lc
from arena import GUARD, MUL, place, rup16  # noqa: F401
from test_gpu_layouts import classify
from test_gpu_some import bits
from test_gpu_wide import arena_case, arena_layout

LIMIT = 256 << 20


def note(what, *arrays, extra=0):
    """The largest host array (or arena of `extra` bytes) a case builds stays under 256 MB."""
    assert max([a.nbytes for a in arrays] + [extra]) < LIMIT, what


def dict_arrays(c):
    return [a for a in c.values() if isinstance(a, np.ndarray)]


@pytest.mark.parametrize("L", lc.LENS)
def test_lengths_leave_one_workgroup_and_have_a_tail(L):
    cps = (L + 15) // 16
    assert cps > 256 and cps % 64 != 0 and L % 16 != 0
    # the flat grid of the batch is no multiple of 8: both sides of the XCD order's full-rounds boundary
    assert -(-lc.BATCH[L] * cps // 256) % 8 != 0
    assert lc.CUT_L % 16 == 0 and lc.CUT_L // 16 > 256


def check_narrow(c, k, m, B, single_only=False):
    n = k + m
    lost, e_d, few, kind = classify(c["masks"], k, m)
    kinds = {0, 1, 2, 4} | ({3} if min(k, m) >= 2 and not single_only else set())
    assert set(kind.tolist()) == kinds and len(kind) == B
    if B == len(kinds):
        assert sorted(kind.tolist()) == sorted(kinds)          # one block of each kind
    sh, dmg, rec = c["sh"], c["dmg"], c["rec"]
    assert sh.shape == (B, n, sh.shape[2]) and np.array_equal(lost, c["lost"]) and np.array_equal(few, c["few"])
    assert np.array_equal(dmg[~lost], sh[~lost]) and (dmg[lost] == lc.ERASED).all()
    assert np.array_equal(rec[~few][:, :k], sh[~few][:, :k])   # recoverable blocks: the original data
    assert np.array_equal(rec[few], dmg[few])                   # the others as they were
    assert np.array_equal(rec[:, k:], dmg[:, k:])               # parity is never rebuilt
    assert few.any() and (e_d[~few] == 1).any()                 # a -4 block, and one a single-slot recover rebuilds
    if single_only:
        assert e_d[~few].max() == 1


@pytest.mark.parametrize("k,m,L", [(k, m, lc.L_SHORT) for k, m in lc.NARROW_CODES] +
                         [(k, m, lc.L_LONG) for k, m in lc.NARROW_LONG_CODES])
def test_narrow_batches_hold_every_block_kind(oracle, k, m, L):
    B = lc.BATCH[L]
    c = lc.narrow_case(oracle, k, m, L)
    assert c["sh"].shape[2] == L
    check_narrow(c, k, m, B)
    if (k, m) == (8, 4):
        check_narrow(lc.narrow_case(oracle, k, m, L, single_only=True), k, m, B, single_only=True)
    note(("narrow", k, m, L), *dict_arrays(c),
         extra=max(lc.narrow_arena_bytes(lay, k, m, L, B) for lay in lc.NARROW_LAYOUTS))


@pytest.mark.parametrize("k,m", lc.HOST_CODES)
def test_host_batches_hold_every_block_kind(oracle, k, m):
    c = lc.host_case(oracle, k, m)
    assert c["sh"].shape == (lc.HOST_B, k + m, lc.HOST_L)
    check_narrow(c, k, m, lc.HOST_B)
    assert -(-lc.HOST_B // lc.HOST_CHUNK) == 5 and lc.HOST_B % lc.HOST_CHUNK == 1   # five chunks, the last of one block
    note(("host", k, m), *dict_arrays(c))


@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k,m", lc.WIDE_ENCODES)
def test_wide_encode_cases(oracle, k, m, L):
    sh = lc.wide_encode_case(oracle, k, m, L)
    assert sh.shape == (lc.WIDE_B, k + m, L) and sh[:, k:].any()
    assert m > 16 and (16 * k > 2048) == ((k, m) == (130, 20))   # two row passes; tables in global memory
    note(("wide encode", k, m, L), sh)


@pytest.mark.parametrize("k,m,L", [(k, m, L) for L in lc.LENS for (k, m) in lc.WIDE_CODES[L]])
def test_wide_cases_hold_their_three_blocks(oracle, fec, MUL, k, m, L):
    c = lc.wide_case(oracle, fec, MUL, k, m, L)
    present, sh, ref, dmg = c["present"], c["sh"], c["ref"], c["dmg"]
    e_d = (~present[:, :k]).sum(axis=1)
    assert sh.shape == (lc.WIDE_B, k + m, rup16(L)) and not sh[:, :, L:].any()
    assert 1 <= e_d[0] <= 2 and present[0].sum() >= k
    assert e_d[1] == lc.WIDE_BIG_LOSS[(k, m)] <= 24 and present[1].sum() >= k
    if (k, m) in ((40, 20), (128, 128)):
        assert e_d[1] > 16                                      # a second row pass
    assert present[2].sum() == k - 1 and e_d[2] >= 1            # short of shards
    assert list(c["st_ref"]) == [0, 0, -4]
    assert np.array_equal(ref[:2, :k], sh[:2, :k]) and np.array_equal(ref[2], dmg[2])
    assert np.array_equal(ref[:, k:], dmg[:, k:])
    words = c["masks"].shape[1]
    assert words == (2 if k + m <= 32 else fec.mask_words(k + m))
    assert np.array_equal(bits(c["masks"][:, 0], min(k + m, 32)), present[:, :32])
    note(("wide", k, m, L), *dict_arrays(c), extra=lc.WIDE_B * (min(k, m) + k + m) * (rup16(L) + 16))


def test_wide_host_case_is_a_wide_case():
    k, m, L, B = lc.HOST_WIDE
    assert (k, m) in lc.WIDE_CODES[L] and B == lc.WIDE_B and k + m > 32


@pytest.mark.parametrize("layout", ["interleaved_slack", "shard_major"])
def test_wide_arena_case_holds_every_kind(oracle, layout):
    k, m, L, B = 40, 20, lc.L_SHORT, lc.WIDE_ARENA_B
    kinds, present, sh = arena_case(oracle, layout, L, B)
    assert set(kinds.tolist()) == {0, 1, 2, 7, 20, -1, 16, 17}
    e_d = (~present[:, :k]).sum(axis=1)
    assert np.array_equal(e_d[kinds >= 0], kinds[kinds >= 0]) and (present[kinds >= 0].sum(axis=1) >= k).all()
    assert (present[kinds < 0].sum(axis=1) == k - 1).all()
    data, par, out = arena_layout(layout, k, m, L, min(k, m), B)
    idx = data.idx(0, L)                                        # the runner's largest array
    note(("wide arena", layout), sh, idx, extra=max(data.end(), par.end(), out.end()) + GUARD)


@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k,m", lc.SOME_CODES)
def test_reconstruct_some_cases(oracle, k, m, L):
    B = lc.BATCH[L]
    c = lc.some_case(oracle, k, m, L)
    lost, ok = c["lost"], c["ok"]
    assert lost.shape == (B, k + m) and (~ok).any()
    assert (ok & lost[:, k:].any(axis=1)).any() and (ok & lost[:, :k].any(axis=1)).any()   # parity and data rebuilt
    assert np.array_equal(c["full"][ok], c["sh"][ok])
    s, want = lc.some_subset_case(oracle, k, m, L)
    named = bits(want, k + m) & s["lost"]
    assert (s["lost"].sum(axis=1) == 4).all() and (named.sum(axis=1) == 2).all() and s["ok"].all()   # a strict subset
    assert (named[:, :k].sum(axis=1) == 1).all()
    data, par = place("interleaved_slack", k, m, L, B)
    note(("some", k, m, L), *dict_arrays(c), *dict_arrays(s), extra=max(data.end(), par.end()) + GUARD)


@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k", lc.XOR_KS)
def test_xor_cases(oracle, k, L):
    c = lc.xor_case(oracle, k, L)
    B = lc.BATCH[L]
    assert c["sh"].shape == (B, k + 1, L) and set(c["kind"].tolist()) == {0, 1, 2, 3}
    lost = c["lost"]
    assert not lost[c["kind"] == 0].any()
    assert (lost[c["kind"] == 1] == ([False] * k + [True])).all()
    assert (lost[c["kind"] == 2].sum(axis=1) == 1).all() and not lost[c["kind"] == 2][:, k].any()
    assert (lost[c["kind"] == 3].sum(axis=1) == 2).all() and lost[c["kind"] == 3][:, :k].any(axis=1).all()
    good = ~c["fail"]
    assert np.array_equal(c["rec"][good][:, :k], c["sh"][good][:, :k])
    assert np.array_equal(c["rec"][c["fail"]], c["dmg"][c["fail"]])
    assert np.array_equal(c["rec"][:, k], c["dmg"][:, k])
    note(("xor", k, L), *dict_arrays(c))


def test_cut_batch_is_one_block_past_the_launch_limit():
    per_launch, B, cps, nchunks = lc.cut_shape()
    assert cps == 4375 and B == per_launch + 1 and nchunks == B + cps - 1
    assert per_launch * cps <= 1 << 31 < B * cps               # (kMaxItems = 2^31 today)
    # three streams with their guards, the statuses and the masks
    note("cut", np.empty(0), extra=GUARD + 3 * (nchunks * 16 + GUARD))
    assert 8 * B < LIMIT
