"""far_cases.py on the CPU: every case of the far-offset device tests obeys the no-fault rule, stresses
what it says it stresses at an address the call really forms, fits the arena, holds the block kinds it
names, and starts from contents the oracle gives back; the table of entry points is that of the header."""
import os
import re

import numpy as np
import pytest

import far_cases as fc
from arena import GUARD, folded_parity, recover_statuses, rup16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_layout():
    seen = {}
    for c in fc.CASES:
        seen.setdefault((c.family, c.k, c.m, c.L, c.step if c.step == "update" else fc.slots_of(c),
                         c.call.endswith("_wide_batch"), c.opt == "past4g"), c)
    return list(seen.values())


@pytest.mark.parametrize("c", by_layout(), ids=fc.case_id)
def test_no_alias_leaves_the_arena(c):
    lay = fc.layout_of(c)
    size = fc.arena_bytes()
    assert lay.size <= size <= fc.CAP
    regs = list(lay.regions.values())
    assert min(r.off for r in regs) >= fc.LEAD and max(r.end() for r in regs) + GUARD <= size
    for pname, P in lay.bases().items():
        assert P % 16 == 0
        for A in fc.slot_addresses(lay):
            assert 0 <= A and A + 16 <= size
            for x in fc.aliases(P, A):
                assert 0 <= x and x + 16 <= size, (pname, hex(P), hex(A), hex(x))


@pytest.mark.parametrize("c", by_layout(), ids=fc.case_id)
def test_slots_do_not_overlap(c):
    lay = fc.layout_of(c)
    spans = sorted((r.at(b, j), r.at(b, j) + r.win) for r in lay.regions.values() for b in range(r.B)
                   for j in range(r.rows))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_the_stressed_address_is_formed_and_its_aliases_differ(c):
    """Every stressed pair names a slot that the call, by the case's masks, reads or writes; both of its
    32-bit aliases differ from it ("both"), or the one that can ("sign", "wrap")."""
    lay = fc.layout_of(c)
    T = fc.touched(c)
    assert all(b < fc.B and j < lay.regions[name].rows for name, b, j in T)
    formed = {lay.regions[name].at(b, j): (name, b, j) for name, b, j in T}
    stress = fc.stress_of(c)
    assert stress, "a case that stresses nothing proves nothing"
    for s in stress:
        assert s.A in formed, s.what
        trunc, sext = fc.aliases(s.P, s.A)
        if s.kind == "both":
            assert trunc != s.A and sext != s.A, s.what
        elif s.kind == "sign":
            assert 0 < s.A - s.P < 2**32 and trunc == s.A and sext != s.A, s.what
        else:
            assert s.kind == "wrap" and -2**32 < s.A - s.P < 0 and trunc != s.A, s.what
    kinds = {s.what: s.kind for s in stress}
    if c.family == "far_blocks":
        # every region: a slot of block 4 (past 2^32) and one of block 2 or 3 (past 2^31) is touched
        assert set(lay.regions) <= {"data", "parity", "out", "old"}
        for name in lay.regions:
            assert kinds["b * %s block stride" % name] == "both"
            assert kinds["b * %s block stride past 2^31" % name] == "sign"
            assert max(b for n, b, _ in T if n == name) == fc.B - 1
    elif c.family == "far_shards":
        sign = (c.k, c.m) == (40, 20) and c.opt != "past4g"      # the stride the wide case is given
        assert kinds == {"j * shard stride": "sign" if sign else "both"}
    else:
        assert kinds["parity - data"] == kinds["data - parity"] == "both"
        assert all(kd in ("sign", "wrap") for what, kd in kinds.items() if what.startswith(("out", "old")))


def test_families_are_those_of_the_issue():
    lay = fc.far_layout("far_blocks", 8, 4, 1202, "out", 4)
    d = lay.regions["data"]
    assert d.bs == 2**30 + 16 * 4099 and d.at(2, 0) - d.off >= 2**31 and d.at(4, 0) - d.off >= 2**32
    assert d.at(3, 7) - d.off < 2**32
    assert max(r.off for r in lay.regions.values()) - d.off < 16384
    lay = fc.far_layout("far_parity_above", 8, 4, 1202, "out", 4)
    assert lay.regions["parity"].off - lay.regions["data"].off == 2**32 + 16 * 777
    assert lay.regions["out"].off - lay.regions["data"].off == 2**31 + 16 * 333
    lay = fc.far_layout("far_parity_below", 8, 4, 1202, "old", 8)
    assert lay.regions["data"].off - lay.regions["parity"].off > 2**32
    assert lay.regions["parity"].off == min(r.off for r in lay.regions.values())
    lay = fc.far_layout("far_shards", 8, 4, 1202, "out", 4)
    d, p = lay.regions["data"], lay.regions["parity"]
    assert d.ss == 2**29 + 16 * 257 and d.bs == rup16(1202) + 16
    assert d.at(0, 4) - d.off >= 2**31 and p.at(0, 0) - d.off >= 2**32 and p.off == d.at(0, 8)
    lay = fc.far_layout("far_shards", 40, 20, 1202, None, 0, fc.WIDE_SHARD_STRIDE)
    assert lay.regions["data"].ss == 2**26 + 16 * 257
    for k, m in sorted({(c.k, c.m) for c in fc.CASES}):
        assert fc.shard_stride_for(k, m) < fc.REFUSED_STRIDE
    # (10,22): the first shard past 2^32 is shard 13, and block 4 reads parity shards 17..21
    assert 12 * fc.shard_stride_for(10, 22) < 2**32 <= 13 * fc.shard_stride_for(10, 22)
    assert np.flatnonzero(~fc.far_lost(10, 22)[4])[-5:].tolist() == [27, 28, 29, 30, 31]


def test_arena_is_at_most_12_gib():
    assert fc.arena_bytes() <= 12 << 30
    assert fc.arena_bytes() % 4096 == 0
    assert round(fc.arena_bytes() / 2**30, 2) == 11.85


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_every_block_kind_is_present_where_the_case_says(c):
    """Every case that decodes holds one block of each kind, placed: the rebuilt kinds at blocks 2 and 4
    (the ragged lengths leave both with bytes to rebuild); every other case is given all its shards,
    or names its columns."""
    lost = fc.lost_of(c)
    if c.call.startswith("fec_xor") and lost is not None:
        assert fc.block_kinds(lost, c.k).tolist() == [0, 4, 2, 1, 2]
    elif c.step == "locate_partial":
        assert lost.sum(axis=1).tolist() == [0, 1, 1, 0, 1]
    elif lost is not None:
        mode = fc.mode_of(c)
        kinds = fc.block_kinds(lost, c.k).tolist()
        assert kinds == fc.kinds_wanted(c.k, c.m, mode)
        full = {0, 1, 2, 3, 4} if min(c.k, c.m) >= 2 and mode != "single" else {0, 1, 2, 4}
        assert set(kinds) == (full - {0} if mode == "one_slot" and 3 in full else full)
        assert lost[2, :c.k].any() and lost[4, c.k - 1] and kinds[1] == 4
        if c.step == "recover_1":
            assert lost[4, :c.k].sum() == 1
        if c.opt == "single":
            assert 3 not in kinds
    elif c.step == "update":
        assert fc.column_sets(c.k).sum(axis=1).tolist() == [0, 1, c.k, (c.k + 1) // 2, 1]
    elif c.step == "encode_idx":
        cols = fc.idx_columns(c.k)
        assert (cols.sum(axis=1) == 2).all() and cols[:, c.k - 1].all()
    if "ragged" in c.call:
        assert fc.RAGGED_LENS[2] > 0 and fc.RAGGED_LENS[4] == c.L and len(fc.RAGGED_LENS) == fc.B


def test_the_oracle_gives_the_original_data_back(oracle):
    for k, m, L, mode in sorted({(c.k, c.m, c.L, fc.mode_of(c)) for c in fc.CASES
                                 if c.k + c.m <= 32 and c.step in ("reconstruct", "recover_m", "recover_1")
                                 and not c.call.startswith("fec_xor")}):
        cs = fc.far_rs_case(oracle, k, m, L, mode)      # (asserts it itself)
        assert cs["few"].tolist() == [False, True, False, False, False]
        # every block has contents of its own: an aliased read cannot return the right bytes
        assert len({cs["sh"][b].tobytes() for b in range(fc.B)}) == fc.B
    cs = fc.far_xor_case(oracle, 3, fc.L_LONG)
    assert len({cs["sh"][b].tobytes() for b in range(fc.B)}) == fc.B


def device_calls():
    """The entry points of fec_hip.h that take device memory: those declared with a `flags` parameter."""
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(name for name, args in re.findall(r"\b(fec_[a-z0-9_]+)\s*\(([^)]*)\)", src)
                  if re.search(r"\bint\s+flags\b", args))


def test_the_table_names_every_device_entry_point():
    names = device_calls()
    assert len(names) == 17 and "fec_rs_encode_batch" in names and "fec_sync" not in names
    assert sorted(fc.TABLE) == names
    for call, row in fc.TABLE.items():
        assert row["run"] == fc.FAMILIES, call          # no call is refused a family whose strides fit 32 bits
        assert row["routes"] and all(r in fc.ROUTES for r in row["routes"])
        assert row["refused"] == (["shard_stride_4gib"] if call in fc.REBUILD_CALLS else [])
    assert {c.call for c in fc.CASES} == set(fc.TABLE)
    assert fc.TABLE["fec_rs_encode_batch"]["routes"] == ["generic", "own"]
    assert set(fc.TABLE["fec_rs_reconstruct_batch"]["routes"]) == {"direct", "routed", "noroute", "wave", "rebuild_k",
                                                                    "tile", "short"}
    assert len({fc.case_id(c) for c in fc.CASES}) == len(fc.CASES)


def test_models_shared_with_the_near_tests(oracle, fec):
    e_d, few = np.array([0, 1, 2, 3, 2]), np.array([False, False, False, False, True])
    assert recover_statuses(fec, e_d, few, 2).tolist() == [0, 1, 2, fec.FEC_ERR_INVALID_ARG,
                                                           fec.FEC_ERR_TOO_FEW_SHARDS]
    rng = np.random.default_rng(5)
    k, m, L = 3, 2, 7
    sh = np.zeros((2, k + m, L), dtype=np.uint8)
    sh[:, :k] = rng.integers(0, 256, (2, k, L), dtype=np.uint8)
    oracle.rs_encode(k, m, sh)
    cols = np.array([[True, True, True], [False, False, False]])
    zero = np.zeros((2, m, L), dtype=np.uint8)
    got = folded_parity(oracle, k, m, sh[:, :k], cols, zero)
    assert np.array_equal(got[0], sh[0, k:]) and not got[1].any()
