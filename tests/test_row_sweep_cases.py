"""The cases of test_gpu_row_sweep.py (row_sweep_cases.py), built without a device: what the device
tests rest on. The instance lists of the seven launchers that share the generic fold body are read from
the sources, and for every instance the sweep holds a pass at its top and at its bottom row count, as a
first pass and as a later one; every k mod 8 occurs, the table-edge codes lie on both sides of the LDS
limit, every radius of locate-multi and locate-partial occurs, the oracle's parity of every case makes a
clean block under the oracle's matrix and field, and every locate model builds.
"""
import numpy as np
import pytest

import row_sweep_cases as rs
import test_gpu_locate as lo
import test_gpu_locate_multi as lm
import test_gpu_locate_partial as lp
import test_gpu_ragged as rag
import test_gpu_update as up
import test_gpu_verify as vr
from arena import CANARY, gf, oracle_arena, place, rup16  # noqa: F401

# The codes the enumerated whole-arena tests give each launcher (their CODES lists and the codes their
# other arena tests name; (16,8) is the one shape of test_gpu_sequences.py with 8 rows), for the table below.
ENUMERATED = {
    "update / encode-idx": up.CODES + [(8, 4), (33, 4), (100, 156), (130, 20), (16, 8)],
    "verify": vr.CODES + [(100, 156), (130, 20)],
    "locate": lo.CODES,
    "locate-multi scan": lm.CODES + [(16, 8)],
    "locate-partial scan": lp.CODES + [(40, 16), (16, 8)],
    "encode": [],       # the generic encode is reached through many modules; the sweep's own table only
    "ragged encode": [(k, m) for k, m, _ in rag.ENC_SHAPES] + [(4, 2)],
}


@pytest.mark.parametrize("name", list(rs.LAUNCHERS))
def test_launcher_instances_are_read_from_the_sources(name):
    inst = rs.instances(name)
    assert inst[-1] == 16 and inst[0] in (1, 2) and len(inst) >= 4
    # the passes restated in row_sweep_cases.py never ask for more rows than the widest instance
    passes = rs.LAUNCHERS[name][3]
    for _, m in rs.LAUNCHERS[name][4]:
        assert passes(m) and all(1 <= rows <= inst[-1] for rows, _ in passes(m))
        covered = sum(rows for rows, _ in passes(m))
        assert covered == (m + len(passes(m)) - 1 if name == "locate" and m > 1 else m)   # (locate: row 0 in every pass)


def test_constants_are_read_from_the_sources():
    assert rs.constant("kLocateRows", "fec_locate.hpp") == 16
    assert rs.constant("kInGroup", "fec_kernels.hpp") == 8
    assert rs.constant("kMaxLdsTabs", "fec_kernels.hpp") == 2048
    with pytest.raises(AssertionError):
        rs.constant("kNoSuchConstant", "fec_kernels.hpp")


def test_pass_shapes():
    assert rs.flat_passes(16) == [(16, False)] and rs.flat_passes(17) == [(16, False), (1, True)]
    assert rs.flat_passes(33) == [(16, False), (16, True), (1, True)]
    assert rs.locate_passes(1) == [(1, False)] and rs.locate_passes(16) == [(16, False)]
    assert rs.locate_passes(17) == [(16, False), (2, True)]
    assert rs.locate_passes(31) == [(16, False), (16, True)]
    assert rs.locate_passes(33) == [(16, False), (16, True), (3, True)]
    assert rs.single_pass(16) == [(16, False)]
    with pytest.raises(AssertionError):
        rs.single_pass(17)


@pytest.mark.parametrize("name", list(rs.LAUNCHERS))
def test_every_instance_gets_its_top_and_bottom_row_count(name):
    """An instance added to a launcher fails here until the sweep reaches it."""
    got, want = rs.reached(name, rs.LAUNCHERS[name][4]), rs.wanted(name)
    print("%s, the enumerated tests:\n  %s" % (name, "\n  ".join(rs.table(name, ENUMERATED[name]))))
    print("%s, with the sweep:\n  %s" % (name, "\n  ".join(rs.table(name, ENUMERATED[name] + rs.LAUNCHERS[name][4]))))
    assert sorted(got) == sorted(want)
    for n in want:
        assert want[n] <= got[n], "%s <%d>: no pass of (rows, later) %s" % (name, n, sorted(want[n] - got[n]))
    if ENUMERATED[name]:
        # the gap this sweep closes: the enumerated lists leave some of these passes out
        before = rs.reached(name, ENUMERATED[name])
        assert any(want[n] - before[n] for n in want)


def test_codes_and_shapes():
    group = rs.constant("kInGroup", "fec_kernels.hpp")
    for codes in (rs.INPUT_SWEEP[:17], rs.INPUT_SWEEP[17:], rs.MULTI_CODES):
        assert {k % group for k, _ in codes} == set(range(group))
    assert {3, 5} <= {k % group for k, _ in rs.ROW_SWEEP}                # the residues no enumerated code has
    assert [m for _, m in rs.ROW_SWEEP] == list(range(1, 34))
    for m in (3, 6):
        assert [k for k, mm in rs.INPUT_SWEEP if mm == m] == list(range(1, 2 * group + 2))
    assert not set(rs.FLAT_CODES + rs.RAGGED_CODES + [rs.CARRY_CODE]) & set(rs.FIXED_ENCODES)
    assert len(set(rs.FLAT_CODES)) == len(rs.FLAT_CODES) and len(set(rs.MULTI_CODES)) == len(rs.MULTI_CODES)
    assert all(k >= 1 and m >= 1 and k + m <= 256 for k, m in rs.LOCATE_CODES + rs.MULTI_CODES)
    assert {rs.layout_of(k, m) for k, m in rs.FLAT_CODES} == set(vr.LAYOUTS)
    cps = (rs.L + 15) // 16
    assert cps == 3 and rs.L % 16 == 1 and rs.B * cps == 201 and 201 % 64 != 0
    lens = rag.default_lens(rs.RAGGED_NB)
    assert lens.tolist() == rag.PATTERN * 2


def test_table_edge_codes_lie_on_both_sides_of_the_lds_limit():
    lim = rs.constant("kMaxLdsTabs", "fec_kernels.hpp")
    (k0, m0), (k1, m1), (k2, m2) = rs.TABLE_EDGE
    assert k0 * m0 == lim and m0 == m1 == 16 and k1 == k0 + 1            # the last LDS code, the first past it
    assert [rows * k2 <= lim for rows, _ in rs.flat_passes(m2)] == [False, True]   # a memory pass, then an LDS pass
    k, m = rs.CARRY_CODE
    rows = rs.constant("kLocateRows", "fec_locate.hpp")
    assert len(rs.locate_passes(m)) == 3 == 1 + (m - 16 + 14) // 15      # fec_locate.hpp locate_passes
    assert m > rows and rows * k > lim                                   # locate_needs_carry_tabs
    # the later passes start at r0 = 16 and 31: carry slabs r0 / 15 - 1 = 0 and 1; the last one fits LDS
    assert [r0 // (rows - 1) - 1 for r0 in (16, 31)] == [0, 1]
    assert [r * k <= lim for r, _ in rs.locate_passes(m)] == [False, False, True]
    assert rs.CARRY_CODE in rs.LOCATE_CODES and rs.CARRY_CODE not in rs.FLAT_CODES


def test_every_radius_occurs():
    T = {min(lm.MAX_BAD, m // 2) for _, m in rs.MULTI_CODES}
    assert T == set(range(0, 9))
    # every T >= 1 with a spare sum (odd m) and without one, but T = 8: 17 rows are more than the call takes
    assert {(min(8, m // 2), m % 2) for _, m in rs.MULTI_CODES if m >= 2} == \
        {(t, p) for t in range(1, 8) for p in (0, 1)} | {(8, 0)}
    assert all(n_ <= lm.BRUTE_N for n_ in (k + m for k, m in rs.BRUTE_CODES))
    assert {m // 2 for _, m in rs.BRUTE_CODES} == set(range(0, 6))       # T = 1 .. 5 against the definition
    assert all((k, m) in rs.MULTI_CODES for k, m in rs.BRUTE_CODES)
    below = {(k, m): mb for k, m, mb in rs.MULTI_BELOW}
    for k, m in rs.MULTI_CODES:
        t = min(lm.MAX_BAD, m // 2)
        assert ((k, m) in below) == (t >= 2)
        if t >= 2:
            assert below[(k, m)] == t - 1 >= 1


def syndromes(oracle, gf, k, m, data, par):
    """parity ^ P data by the oracle's matrix and field, [B, m, L]."""
    mul, _ = gf
    P = oracle.build_matrix(k, k + m)[k:]
    s = par.copy()
    for j in range(k):
        s ^= mul[P[:, j][None, :, None], data[:, j][:, None, :]]
    return s


@pytest.mark.parametrize("k,m", rs.LOCATE_CODES + [c for c in rs.MULTI_CODES if c not in rs.LOCATE_CODES])
def test_oracle_parity_makes_a_clean_block(oracle, gf, k, m):
    layout = rs.layout_of(k, m)
    img, data, par = oracle_arena(oracle, layout, k, m, rs.L, rs.B, np.random.default_rng(rs.seed_of(k, m)))
    d, p = data.view(img, 0, rs.L), par.view(img, 0, rs.L)
    assert p.any() and not syndromes(oracle, gf, k, m, d, p).any()
    # the regions, canaries and data bytes of encoded_arena: everything but the parity bytes is the canary
    # image with the same draws from the same rng
    want = np.full_like(img, CANARY)
    data2, par2 = place(layout, k, m, rs.L, rs.B)
    want[data2.index(0, rs.L)] = np.random.default_rng(rs.seed_of(k, m)).integers(0, 256, (rs.B, k, rs.L), dtype=np.uint8)
    want[par2.index(0, rs.L)] = p
    assert np.array_equal(img, want)
    assert (par.view(img, rs.L, rup16(rs.L)) == CANARY).all()
    if (k, m) in rs.FLAT_CODES:
        before, after, _, par3 = rs.encode_case(oracle, k, m)
        assert (par3.view(before) == CANARY).all() and not par3.view(after, rs.L, rup16(rs.L)).any()
        assert np.array_equal(par3.view(after, 0, rs.L), p)
        vb = rs.verify_batch(None, None, None, oracle, k, m)
        assert np.array_equal(vb.img, img) and not vb.img.flags.writeable


@pytest.mark.parametrize("k,m", rs.LOCATE_CODES)
def test_locate_models_build(oracle, gf, k, m):
    b = rs.locate_batch(None, None, None, oracle, gf, k, m)
    want = set(b.want.tolist())
    assert lo.CLEAN in want and lo.UNKNOWN in want and ((b.want >= 0).any() or m < 2)
    assert not syndromes(oracle, gf, k, m, b.data.view(b.clean, 0, rs.L), b.par.view(b.clean, 0, rs.L)).any()


@pytest.mark.parametrize("k,m", rs.MULTI_CODES)
def test_locate_multi_models_build(oracle, gf, k, m):
    below = [mb for kk, mm, mb in rs.MULTI_BELOW if (kk, mm) == (k, m)]
    for max_bad in [lm.MAX_BAD] + below:
        b = rs.multi_batch(None, None, None, oracle, gf, k, m, max_bad)
        assert b.T == min(max_bad, m // 2) and b.brute == (k + m <= 12)
        assert (b.want == 0).any()
        if b.brute or m - b.T > b.T:      # (the theorem's codes keep to m - T corrupt shards)
            assert (b.want == lm.UNKNOWN).any()
        if b.T:
            assert (b.want == 1).any() and (b.want == b.T).any()             # the solver runs at its full radius
        assert not syndromes(oracle, gf, k, m, b.data.view(b.clean, 0, rs.L), b.par.view(b.clean, 0, rs.L)).any()


@pytest.mark.parametrize("k,m", rs.MULTI_CODES)
def test_locate_partial_models_build(oracle, gf, k, m):
    b = rs.partial_batch(None, None, None, oracle, gf, k, m)
    for max_bad in rs.partial_max_bads(m):
        want, _ = b.expect(max_bad)
        assert (want == lp.TOO_FEW).any() and (want == 0).any()
        if max_bad and m >= 2:
            assert (want > 0).any()


def test_locate_partial_radii(oracle, gf):
    """Every T_b = 0 .. 8 with both parities of m - e_b over the blocks of the row sweep's batches; T_b = 8
    needs 16 or 17 sums, and a code has at most 16 rows here, so it occurs with an even count alone."""
    radii = set()
    for k, m in rs.ROW_SWEEP[:16]:
        b = rs.partial_batch(None, None, None, oracle, gf, k, m)
        radii.update((int(t), int(m - e) % 2) for t, e, few in zip(b.Tb, b.e, b.few) if not few)
    assert radii == {(t, p) for t in range(8) for p in (0, 1)} | {(8, 0)}
