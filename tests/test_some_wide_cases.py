"""some_wide_cases.py checked on the CPU: every batch of the wide reconstruct-some device tests holds
each kind of block it claims, the expected bytes (inverse-matrix rows from the oracle) equal the
oracle's encode for every recoverable block, the mask helpers keep the wide calls' bit order, and the
far cases fit the arena of far_cases.py by its rule."""
import numpy as np
import pytest

import far_cases as fc
import some_wide_cases as sw


@pytest.mark.parametrize("k,m", sw.CODES)
def test_every_batch_holds_the_kinds_it_claims(oracle, k, m):
    n = k + m
    for L in (1, 33):
        c = sw.rs_case(oracle, k, m, L)
        lost, kind, ok = c["lost"], c["kind"], c["ok"]
        assert len(lost) == sw.B == 67
        sw.check_kinds(lost, kind, k, m)
        nl, nd = lost.sum(axis=1), lost[:, :k].sum(axis=1)
        assert (nl == 0).any(), "an intact block"
        assert (n - nl == k - 1).any() and not ok[n - nl == k - 1].any(), "k - 1 present"
        if m >= 1:
            assert ((nd == 0) & (nl > 0)).any(), "parity-only loss"
            assert ((nd == 1) & (nl == 1)).any(), "one data shard lost"
        if m >= 2:
            assert ((nl == m) & (nd >= 1) & (nd < nl) & ok).any(), "mixed loss of exactly m shards"
        if m >= k:
            assert (lost[:, :k].all(axis=1) & (n - nl == k)).any(), "k present, all of them parity"
        if m:
            assert nl[ok].max() == m, "some block loses as many shards as the code bears"
        # the recoverable blocks are those with k or more present, and the rest stay damaged
        assert np.array_equal(ok, n - nl >= k)
        assert np.array_equal(c["full"][~ok], c["dmg"][~ok])
        assert np.array_equal(c["full"][ok], c["sh"][ok])     # (make_case asserts it too)
    if (k, m) in ((16, 240), (1, 255)):
        # a block rebuilds m rows: 15 and 16 row passes of 16
        assert c["lost"][c["ok"]].sum(axis=1).max() == m and -(-m // 16) == {240: 15, 255: 16}[m]


def test_boundary_shards_are_lost_somewhere(oracle):
    for k, m in ((33, 32), (64, 16), (128, 128)):
        lost = sw.rs_case(oracle, k, m, 33)["lost"]
        for i in sw.BOUNDARY:
            assert lost[sw.rs_case(oracle, k, m, 33)["ok"], i].any(), (k, m, i)


def test_expected_rows_do_not_read_past_the_first_k_present(oracle):
    """rebuild_rows takes the first k present shards only: garbage in a later present shard changes
    nothing, garbage in one of the first k does."""
    k, m, L = 20, 13, 33
    rng = np.random.default_rng(5)
    blk = np.zeros((1, k + m, L), dtype=np.uint8)
    blk[0, :k] = rng.integers(0, 256, (k, L), dtype=np.uint8)
    oracle.rs_encode(k, m, blk)
    lost = np.zeros(k + m, dtype=bool)
    lost[[3, k + 1]] = True
    want = sw.rebuild_rows(oracle, k, k + m, lost, blk[0])
    assert np.array_equal(want[3], blk[0, 3]) and np.array_equal(want[k + 1], blk[0, k + 1])
    g = blk[0].copy()
    g[k + 2:] = 0xEE                       # inputs: data but 3, parity 0; parity 2.. unused
    got = sw.rebuild_rows(oracle, k, k + m, lost, g)
    assert all(np.array_equal(got[o], want[o]) for o in want)
    g[k] ^= 1
    assert not np.array_equal(sw.rebuild_rows(oracle, k, k + m, lost, g)[3], want[3])
    lost[:14] = True
    assert sw.rebuild_rows(oracle, k, k + m, lost, blk[0]) is None     # 19 present


def test_mask_helpers(fec):
    rng = np.random.default_rng(3)
    p = rng.integers(0, 2, (5, 65)).astype(bool)
    w = fec.wide_masks(p)
    assert w.shape == (5, 3) and np.array_equal(sw.bits(w, 65), p)
    s = sw.stray(w, 65)
    assert np.array_equal(sw.bits(s, 65), p) and (s[:, 2] | 1 == 0xFFFFFFFF).all()
    w8 = np.zeros((5, 8), dtype=np.uint32)
    w8[:, :3] = w
    s8 = sw.stray(w8, 65, rng)
    assert np.array_equal(sw.bits(s8, 65), p) and (s8[:, 3:] != 0).any()


@pytest.mark.parametrize("family", fc.FAMILIES)
@pytest.mark.parametrize("L", sw.FAR_LENS)
def test_far_cases_fit_the_far_arena(family, L):
    """The layouts of the far test obey the rule of far_cases.py within the arena its cases size, and the
    loss is mixed: block 4, the farthest, rebuilds data and parity and reads the last parity shards."""
    k, m = sw.FAR_CODE
    lay = fc.far_layout(family, k, m, L)
    assert lay.size <= fc.arena_bytes() <= fc.CAP
    lost = sw.far_lost(k, m)
    n = k + m
    assert len(lost) == fc.B
    present = (~lost).sum(axis=1)
    assert present.tolist()[:2] == [n, k - 1] and (present[2:] >= k).all()
    assert lost[4, :k].any() and lost[4, k:].any() and lost[4, k - 1] and not lost[4, n - 1]
    assert lost[2, :k].sum() == 1 and lost[2, k:].sum() == 1 and not lost[3, :k].any() and lost[3, n - 1]
