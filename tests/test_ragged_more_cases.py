"""ragged_more_cases.py on the CPU: the batches of the ragged verify and reconstruct-some tests hold
what they are meant to hold, and their expected statuses and images agree with the oracle run block
by block at each block's own length (the model, not the library); the far layouts obey the no-fault
rule of far_cases.py and stress what they say they stress."""
import numpy as np
import pytest

import far_cases as fc
import ragged_more_cases as rc
from arena import CANARY, GUARD, rup16


def parity_by_oracle(oracle, k, m, data, L):
    sh = np.zeros((1, k + m, L), dtype=np.uint8)
    sh[0, :k] = data[:, :L]
    oracle.rs_encode(k, m, sh)
    return sh[0, k:]


@pytest.mark.parametrize("k,m,nb", rc.VERIFY_SHAPES)
@pytest.mark.parametrize("key", [None, "oversize"])
def test_verify_batches_hold_every_kind_and_agree_with_the_oracle(oracle, k, m, nb, key):
    lens = None
    if key:
        lens = rc.default_lens(nb).copy()
        lens[[5, 17]] = rc.MAXL + 1
        lens[11] = 0xFFFFFFFF
    c = rc.verify_case(rc.oracle_encode(oracle), k, m, nb, lens=lens, key=key)
    st, ok, slots = c["status"], c["ok"], c["slots"]
    assert (st == 1).any() and (st == 0).any()
    assert ((st == rc.SHARD_SIZE).sum() == 3) if key else not (st == rc.SHARD_SIZE).any()
    assert (st[c["lens"] == 0] == 1).all() and c["count"] == (st == 0).sum()
    # a bad block whose only wrong byte is its last one; bad blocks whose byte is in the first and
    # in a middle chunk, in a data and in a parity shard
    per_block = {}
    for b, j, x in c["flips"]:
        per_block.setdefault(b, []).append((j, x))
    assert all(len(v) == 1 for v in per_block.values())
    where = {(j >= k, "last" if x == ok[b] - 1 else "first" if x == 0 else "mid") for b, j, x in c["flips"]}
    assert {(False, "last"), (True, "last"), (False, "first"), (True, "mid"), (False, "mid")} <= where
    assert any(x == ok[b] - 1 and ok[b] > 16 and ok[b] % 16 for b, j, x in c["flips"])   # in a partial tail chunk
    if m > 16:   # a parity row of the second row pass alone
        assert any(j >= k + 16 for b, j, x in c["flips"]) and (c["kind"] == rc.V_PAR_HIGH).any()
    # the model: each block's parity below its length equals the oracle's encode of its data below
    # its length exactly when its status is 1; what lies from the length on is garbage in clean blocks
    rng = np.random.default_rng(1)
    sample = set(rng.choice(nb, size=min(nb, 60), replace=False).tolist()) | set(list(per_block)[:40])
    for b in sorted(sample):
        L = int(ok[b])
        if L == 0:
            assert st[b] == (rc.SHARD_SIZE if c["lens"][b] > rc.MAXL else 1)
            continue
        want = parity_by_oracle(oracle, k, m, slots[b, :k], L)
        assert np.array_equal(want, slots[b, k:, :L]) == (st[b] == 1), b
    clean = np.flatnonzero((st == 1) & (ok > 0) & (ok % 16 != 0))
    assert any((slots[b, :, ok[b]:rup16(ok[b])] != 0).any() and (slots[b, :, rup16(ok[b]):] != 0).any() for b in clean)
    img, data, par = rc.verify_image(c, "split")
    assert np.array_equal(data.view(img), slots[:, :k]) and np.array_equal(par.view(img), slots[:, k:])
    assert (img[:GUARD] == CANARY).all() and (img[-GUARD:] == CANARY).all()


@pytest.mark.parametrize("k,m", rc.SOME_SHAPES)
def test_some_batches_hold_every_kind_and_agree_with_the_oracle(oracle, k, m):
    n = k + m
    c = rc.some_case(rc.oracle_encode(oracle), k, m)
    lost, want, ok, lens = c["lost"], c["want"], c["ok"], c["lens"]
    present = (~lost).sum(axis=1)
    assert np.array_equal(rc.bits(c["masks"], n), ~lost) and np.array_equal(rc.bits(c["wants"], n), want)
    for which, w in (("all", np.ones_like(want)), ("want", want)):
        st, reb = c["st_" + which], c["rebuilt_" + which]
        R = lost & w
        assert (~R.any(axis=1)).any()                                   # nothing to do
        assert ((st == rc.TOO_FEW) & (ok > 0)).any() and ((st == rc.TOO_FEW) & (lens == 0)).any()
        assert (lens == 0).any() and not reb[ok == 0].any()
        assert not reb[st != 0].any() and np.array_equal(reb.any(axis=1), (st == 0) & R.any(axis=1) & (ok > 0))
        if m:
            d, p = reb[:, :k].any(axis=1), reb[:, k:].any(axis=1)
            assert (d & ~p).any() and (p & ~d).any()                    # data-only and parity-only rebuilds
            if m >= 2:
                assert (d & p).any()                                    # mixed
        else:
            assert not reb.any() and set(st.tolist()) == {0, rc.TOO_FEW}
    if m:
        assert (present == k).any() and (present == k - 1).any() and (present == n).any()
        assert {rc.W_ALL, rc.W_DATA, rc.W_PARITY, rc.W_ZERO, rc.W_RANDOM} == set(c["wkind"].tolist())
        hit = c["rebuilt_want"].any(axis=1)
        assert all((hit & (c["wkind"] == wk)).any() for wk in (rc.W_ALL, rc.W_DATA, rc.W_PARITY, rc.W_RANDOM))
        assert not hit[c["wkind"] == rc.W_ZERO].any()
    # the model: the oracle's reconstruct of each damaged block at its own length gives back the data
    # shards the case expects, and its encode of them the parity shards
    img, model, data, par = rc.some_images(c, "interleaved", "want")
    dv, pv = data.view(model), par.view(model)
    rng = np.random.default_rng(2)
    for b in rng.choice(rc.B, size=50, replace=False):
        L = int(ok[b])
        reb = c["rebuilt_want"][b]
        if not reb.any():
            assert np.array_equal(data.view(img)[b], dv[b]) and np.array_equal(par.view(img)[b], pv[b])
            continue
        one = np.zeros((1, n, L), dtype=np.uint8)
        one[0, :k], one[0, k:] = data.view(img)[b, :, :L], par.view(img)[b, :, :L]
        assert (oracle.rs_reconstruct(k, m, one, c["masks"][b:b + 1] & np.uint32((1 << n) - 1)) == 0).all()
        oracle.rs_encode(k, m, one)
        for j in np.flatnonzero(reb):
            got = dv[b, j] if j < k else pv[b, j - k]
            assert np.array_equal(got[:L], one[0, j]) and not got[L:rup16(L)].any()
            assert (got[rup16(L):] == rc.ERASED).all()
        for j in np.flatnonzero(~reb):
            before = data.view(img)[b, j] if j < k else par.view(img)[b, j - k]
            assert np.array_equal(dv[b, j] if j < k else pv[b, j - k], before)


def test_sync_code_ranks_too_few_first():
    assert rc.sync_code([0, 1, 0]) == 0 and rc.sync_code([0, rc.SHARD_SIZE]) == rc.SHARD_SIZE
    assert rc.sync_code([rc.SHARD_SIZE, rc.TOO_FEW]) == rc.TOO_FEW
    assert rc.sync_code([rc.SHARD_SIZE], [rc.TOO_FEW]) == rc.TOO_FEW
    assert rc.sync_code([rc.SINGULAR, rc.SHARD_SIZE]) == rc.SHARD_SIZE and rc.sync_code([rc.SINGULAR]) == rc.SINGULAR


@pytest.mark.parametrize("call", ["verify", "some"])
def test_far_layouts_cannot_fault_and_stress_both_distances(call):
    k, m = 8, 4
    lay = rc.far_layout(k, m)     # (FarLayout asserts that no alias lies below the arena)
    assert lay.size <= fc.arena_bytes() <= fc.CAP
    d, p = lay.regions["data"], lay.regions["parity"]
    assert d.bs == p.bs == 2**30 + 16 * 4099 and p.off - d.off == 2**32 + 16 * 777
    assert d.at(2, 0) - d.off >= 2**31 and d.at(4, 0) - d.off >= 2**32 and d.ss < 2**32
    size = fc.arena_bytes()
    for P in lay.bases().values():
        for A in fc.slot_addresses(lay):
            assert 0 <= A and A + 16 <= size
            assert all(0 <= x and x + 16 <= size for x in fc.aliases(P, A))
    spans = sorted((r.at(b, j), r.at(b, j) + r.win) for r in lay.regions.values() for b in range(r.B)
                   for j in range(r.rows))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    lost = rc.far_some_lost(k, m)
    T = rc.far_verify_touched(k, m) if call == "verify" else rc.far_some_touched(lost, k)
    formed = {lay.regions[name].at(b, j) for name, b, j in T}
    for s in rc.far_stress(lay, T):
        assert s.A in formed, s.what
        trunc, sext = fc.aliases(s.P, s.A)
        if s.kind == "both":
            assert trunc != s.A and sext != s.A, s.what
        else:
            assert 0 < s.A - s.P < 2**32 and trunc == s.A and sext != s.A, s.what
    if call == "some":
        present = (~lost).sum(axis=1)
        assert (present >= k).tolist() == [True, False, True, True, True]
        assert lost[4, k - 1] and lost[4, k + m - 1] and lost[0, :k].any() and lost[0, k:].any()
        assert max(b for _, b, _ in T) == fc.B - 1 and len(rc.FAR_LENS) == fc.B and rc.FAR_LENS[4] == rc.MAXL
