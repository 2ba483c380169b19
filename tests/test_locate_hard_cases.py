"""The hard locate batches of locate_hard_cases.py and the Berlekamp-Welch model of locate_model.py,
checked without a device:
  - the anchors of the model: the oracle's encode gives, per byte column, the values of a polynomial of
    degree < k at the points 0 .. n - 1 (the model finds no error at radius 0), and for the codes of
    n <= 12 the model equals the brute-force models of test_gpu_locate_multi.py and
    test_gpu_locate_partial.py block for block on those modules' batches (the oracle's parity in place
    of the device's);
  - every block's result by construction equals the model's;
  - the mix: every class in at least 3 blocks of a batch, a block located at v = T, an unknown one and a
    miscorrected one in each, at most one class a block located, every number of corrupt shards from
    T + 1 to min(n, m + 2) over the lengths of a code;
  - a Python port of the library's column solver (fec_locate_multi.hpp: locate_multi_column) agrees with
    the model on every block, and stops agreeing on blocks of classes a, c and d when its count of roots
    or its range check is taken out: the batches can tell such a solver from a right one.

All of it again for the batches under the Cauchy code (cauchy_oracle as the encoder, its multipliers
through the model, the constructions and the port), at the two lengths the device runs and at 17; there
a class e block's bytes, given to the model without the multipliers, do not decode to the planted set,
and its errors are no zero pivot under the unscaled weights: the case belongs to the Cauchy weights.
"""
import functools

import numpy as np
import pytest

import cauchy_oracle
from arena import gf, oracle_arena  # noqa: F401
from locate_hard_cases import CAUCHY_CODES, CODES, LENS, Builder, cases, max_bads, params
from locate_model import TOO_FEW, UNKNOWN, bw_column, model_batch, model_block, powers, syndromes, xdot
from test_gpu_locate import model_verdicts
from test_gpu_locate_multi import BRUTE_N, Batch
from test_gpu_locate_multi import model_brute as multi_brute
from test_gpu_locate_partial import PBatch
from test_gpu_locate_partial import model_brute as partial_brute

SMALL = [(1, 2), (2, 2), (6, 3), (8, 4)]     # the siblings' codes of 0 < m and n <= 12


@pytest.mark.parametrize("L", [1, 17, 33])
@pytest.mark.parametrize("k,m", SMALL)
def test_model_equals_locate_multi_brute_force(oracle, gf, k, m, L):
    b = Batch(None, None, None, oracle, gf, "interleaved", k, m, L, 67, 1000 * k + 10 * m + L,
              build=functools.partial(oracle_arena, oracle))
    assert b.brute
    want, sets = model_batch(gf, k, m, b.shards(b.img), L, 8)
    assert np.array_equal(want, b.want) and sets == b.sets
    assert m < 2 or ((want > 0).any() and (want == UNKNOWN).any())


@pytest.mark.parametrize("L", [1, 17, 33])
@pytest.mark.parametrize("k,m", SMALL)
def test_model_equals_locate_partial_brute_force(oracle, gf, k, m, L):
    b = PBatch(None, None, None, oracle, gf, "interleaved", k, m, L, 67, 2000 * k + 10 * m + L,
               build=functools.partial(oracle_arena, oracle))
    assert b.brute
    for max_bad in (8, 1, 0):
        brute, bsets = b.expect(max_bad)
        want, sets = model_batch(gf, k, m, b.shards(b.img), L, max_bad, b.miss)
        assert np.array_equal(want, brute) and sets == list(bsets), max_bad
    assert (want == TOO_FEW).any() and (want == UNKNOWN).any()


TAKEN = set()     # the solver's rare branches a run of the port took: ("swap" | "singular", v)


def solver_port(gf, W, n, T, present=None, mutate=None):
    """locate_multi_column on the sums W, step for step: the set of shards, or None. present: MASKED.
    mutate "range": without `ok = r < n`; "count": without `count != v`."""
    mul, inv = gf
    m = len(W)

    def has(r):
        return present is None or r in present
    if T >= 1 and W[0]:
        r = int(mul[W[1], inv[W[0]]])
        ok = (r < n or mutate == "range") and (has(r) or r >= n)
        l = 1
        while l + 1 < m and ok:
            ok = int(mul[r, W[l]]) == W[l + 1]
            l += 1
        if ok:
            return {r}
    for v in range(2, T + 1):
        M = [[W[i + j] for j in range(v)] + [W[v + i]] for i in range(v)]
        singular = False
        for c in range(v):
            p = next((i for i in range(c, v) if M[i][c]), None)
            if p is None:
                singular = True
                TAKEN.add(("singular", v))
                break
            if p != c:
                TAKEN.add(("swap", v))
            pi = inv[M[p][c]]
            row = [int(mul[x, pi]) for x in M[p]]
            M[p] = M[c]
            M[c] = row
            for i in range(v):
                f = M[i][c]
                if i != c and f:
                    M[i] = [x ^ int(mul[f, y]) for x, y in zip(M[i], M[c])]
        if singular:
            continue
        sigma = [M[j][v] for j in range(v)]
        if any(W[l + v] ^ functools.reduce(lambda a, j: a ^ int(mul[sigma[j], W[l + j]]), range(v), 0)
               for l in range(v, m - v)):
            continue
        roots = set()
        for r in range(n):
            acc = 1
            for j in range(v - 1, -1, -1):
                acc = int(mul[acc, r]) ^ sigma[j]
            if acc == 0 and has(r):
                roots.add(r)
        if len(roots) != v and mutate != "count":
            continue
        return roots
    return None


def port_batch(gf, cs, mutate=None):
    """The results the library's arithmetic gives a batch: power sums, the column solver, the merge."""
    mul, _ = gf
    want = np.zeros(cs.B, dtype=np.int32)
    sets = [frozenset()] * cs.B
    for b in range(cs.B):
        P = sorted(set(range(cs.n)) - cs.miss[b])
        bd = Builder(gf, cs.k, cs.n, P, cs.T[b], None, cs.mult)
        u = np.array([bd.u[r] for r in P], dtype=np.uint8)
        A = mul[powers(gf, P, bd.ms), u[:, None]].T                     # row l: u_r r^l
        W = xdot(mul, A, np.ascontiguousarray(cs.bad[b][P]))
        U, unknown = set(), False
        for x in np.flatnonzero(W.any(axis=0)):
            s = solver_port(gf, [int(w) for w in W[:, x]], cs.n, cs.T[b], set(P) if cs.miss[b] else None, mutate)
            unknown |= s is None
            U |= s or set()
        if unknown or len(U) > cs.T[b]:
            want[b] = UNKNOWN
        else:
            want[b], sets[b] = len(U), frozenset(U)
    return want, sets


def classes(cs):
    return [kd if kd in ("loc", "clean") else kd[0] for kd in cs.kind]


@pytest.mark.parametrize("call,k,m,L,max_bad", params())
def test_hard_batch(oracle, gf, call, k, m, L, max_bad):
    check_hard_batch(oracle, gf, cases(oracle, gf, call, k, m, L, max_bad), call, k, m, L, max_bad)


@pytest.mark.parametrize("call,k,m,L,max_bad", params(cauchy=True, lens=LENS))
def test_hard_batch_cauchy(gf, call, k, m, L, max_bad):
    v = cauchy_oracle.code_multipliers(k, m)
    cs = cases(cauchy_oracle, gf, call, k, m, L, max_bad, v)
    check_hard_batch(cauchy_oracle, gf, cs, call, k, m, L, max_bad)
    # the batch is not the kind-0 batch under another name: its blocks are no codewords without v
    assert syndromes(gf, list(range(k + m)), cs.clean[0], k).any(axis=0).all()
    # class e is specific to the scaled weights: without the multipliers the same bytes do not decode to
    # the planted set, and the planted errors are no zero pivot under the weights u_r
    specific = 0
    for b in [b for b in range(cs.B) if cs.kind[b] == "e"]:
        P = sorted(set(range(k + m)) - cs.miss[b])
        (col,) = cs.cols[b].values()
        plain = model_block(gf, k, m, P, cs.bad[b], L, max_bad)
        W = Builder(gf, k, k + m, P, cs.T[b], None).sums(col.errs, 3)
        zero = W[0] == 0 if len(col.errs) == 2 else gf[0][W[0], W[2]] == gf[0][W[1], W[1]]
        specific += plain != (len(col.want), col.want) and not zero
    assert specific >= 1 or not any(kd == "e" for kd in cs.kind)


def check_hard_batch(oracle, gf, cs, call, k, m, L, max_bad):
    v = cs.mult
    n, B = k + m, cs.B
    # the anchor: the oracle's blocks are polynomials of degree < k at the points 0 .. n - 1
    pts = list(range(n))
    for b in (0, B - 1):
        assert not syndromes(gf, pts, cs.clean[b], k, v).any()
        assert bw_column(gf, pts, cs.clean[b][:, L - 1], k, 0, v) == frozenset()
    flip = cs.clean[0][:, 0].copy()
    flip[n - 1] ^= 1
    assert bw_column(gf, pts, flip, k, 0, v) is None
    # by construction == by the model
    for b in range(B):
        if cs.built[b] is not None:
            assert cs.built[b] == (cs.want[b], cs.sets[b]), (b, cs.kind[b], cs.T[b], cs.built[b], cs.want[b], cs.sets[b])
    if n <= BRUTE_N:    # (8,4): every subset of shards can be tried as well
        if call == "multi":
            bw, bs = multi_brute(oracle, gf, k, m, min(max_bad, m // 2), cs.bad, L)
        else:
            both = [partial_brute(oracle, gf, k, m, cs.T[b], sorted(set(pts) - cs.miss[b]), cs.bad[b], L) for b in range(B)]
            bw, bs = np.array([r for r, _ in both]), [s for _, s in both]
        assert np.array_equal(bw, cs.want) and list(bs) == cs.sets
    # the library's arithmetic, ported, gives the same
    TAKEN.clear()
    pw, ps = port_batch(gf, cs)
    assert np.array_equal(pw, cs.want) and ps == cs.sets, np.flatnonzero(pw != cs.want)
    # class e takes the solver's pivot swap and, with three errors, its singular system at v = 2
    zero = [cs.t[b] for b in range(B) if cs.kind[b] == "e"]
    assert ("swap", 2) in TAKEN or 2 not in zero
    assert {("singular", 2), ("swap", 3)} <= TAKEN or 3 not in zero
    # the mix
    cl = classes(cs)
    applicable = {"a", "b", "f"} | ({"c"} if n < 256 else set()) | ({"d"} if call == "partial" else set())
    if min(max_bad, (m - (call == "partial")) // 2) >= 2:
        applicable.add("e")
    for c in sorted(applicable):
        assert cl.count(c) >= 3, (c, cl.count(c))
    assert set(cl) <= applicable | {"loc", "clean"}
    changed = [set().union(*[set(c.errs) for c in cs.cols[b].values()]) if cs.cols[b] else set() for b in range(B)]
    assert any(cs.want[b] == cs.T[b] and cs.sets[b] == changed[b] and len(cs.cols[b]) == 1 for b in range(B)), "v = T"
    assert (cs.want == UNKNOWN).any()
    mis = [b for b in range(B) if cs.want[b] > 0 and not (cs.sets[b] & changed[b])]
    assert len(mis) >= 3 and all(cl[b] in "ab" for b in mis)
    assert sum(1 for b in range(B) if cl[b] == "a" and cs.want[b] != UNKNOWN) <= 1
    for b in range(B):
        if cl[b] in ("c", "d") or cs.kind[b] in ("f1", "f2", "f3"):
            assert cs.want[b] == UNKNOWN, (b, cs.kind[b])
        if cl[b] in ("e", "loc") or cs.kind[b] == "f4":
            assert cs.want[b] == len(cs.sets[b]) > 0 and cs.sets[b] == changed[b], (b, cs.kind[b])
        assert len(cs.cols[b]) <= 8 and not (changed[b] & cs.miss[b])
    # what a located block heals to: a codeword that agrees with every present shard outside the set
    for b in np.flatnonzero(cs.want >= 0):
        xs = sorted(cs.cols[b]) + [0]
        keep = sorted(set(pts) - cs.miss[b] - cs.sets[b])
        assert not syndromes(gf, pts, cs.final[b][:, xs], k, v).any(), (b, cs.kind[b])
        assert np.array_equal(cs.final[b][keep], cs.bad[b][keep]), (b, cs.kind[b])
        assert cs.kind[b] in ("a", "b") or np.array_equal(cs.final[b], cs.clean[b])
    if call == "multi" and n < 256:
        # a single pseudo-root outside the code: fec_rs_locate_batch's definition calls it unknown too
        one = [b for b in range(B) if cl[b] == "c" and cs.v[b] == 1]
        assert one and (model_verdicts(oracle, gf, k, m, cs.bad, L)[one] == UNKNOWN).all()
    if call == "partial":
        sums = sorted({m - len(x) for x in cs.miss})
        assert sums == sorted({m - 1, m - 2, 2}) and any(s % 2 for s in sums)


def cauchy_cases(gf, call, k, m, L, max_bad):
    return cases(cauchy_oracle, gf, call, k, m, L, max_bad, cauchy_oracle.code_multipliers(k, m))


@pytest.mark.parametrize("call", ["multi", "partial"])
@pytest.mark.parametrize("k,m", CODES)
def test_class_a_reaches_every_number_of_corrupt_shards(oracle, gf, call, k, m):
    check_class_a(functools.partial(cases, oracle, gf), call, k, m)


@pytest.mark.parametrize("call", ["multi", "partial"])
@pytest.mark.parametrize("k,m", CAUCHY_CODES)
def test_class_a_reaches_every_number_of_corrupt_shards_cauchy(gf, call, k, m):
    check_class_a(functools.partial(cauchy_cases, gf), call, k, m)


def check_class_a(get, call, k, m):
    """Over the lengths of a code and radius: every t from T + 1 to min(n, m' + 2), none capped. (The 23
    blocks of a (240,16) batch, spread over three numbers of missing shards, hold 2 or 3 class a blocks
    of each: there at least 6 values of t, T + 1 among them.)"""
    for max_bad in max_bads(k, m):
        seen = {}
        for L in LENS:
            cs = get(call, k, m, L, max_bad)
            for b in range(cs.B):
                if cs.kind[b] == "a":
                    seen.setdefault(len(cs.miss[b]), set()).add(cs.t[b])
        # missing shards of the class a blocks: 1, 2 and m - 2 (not in 256 shards: locate_hard_cases.py)
        assert sorted(seen) == ([0] if call == "multi" else [1, 2] if k + m == 256 else sorted({1, 2, m - 2}))
        for e, ts in seen.items():
            T = min(max_bad, (m - e) // 2)
            full = set(range(T + 1, min(k + m - e, m - e + 2) + 1))
            if call == "partial" and k + m == 256:
                assert ts <= full and T + 1 in ts and len(ts) >= min(len(full), 6), (e, sorted(ts))
            else:
                assert ts == full, (e, sorted(ts))


@pytest.mark.parametrize("call", ["multi", "partial"])
@pytest.mark.parametrize("k,m", CODES)
def test_the_batches_catch_a_solver_without_its_root_checks(oracle, gf, call, k, m):
    check_catch(gf, cases(oracle, gf, call, k, m, 33, 8), call, k, m)


@pytest.mark.parametrize("call", ["multi", "partial"])
@pytest.mark.parametrize("k,m", CAUCHY_CODES)
def test_the_batches_catch_a_solver_without_its_root_checks_cauchy(gf, call, k, m):
    check_catch(gf, cauchy_cases(gf, call, k, m, 33, 8), call, k, m)


def check_catch(gf, cs, call, k, m):
    """The port without `count != v`, and without `ok = r < n`: each names shards in blocks of classes
    a, c or d that the model calls unknown (a code of 256 shards has no point at or above n: only the
    count of roots can go wrong there)."""
    cl = classes(cs)
    for mutate in ("count", "range"):
        pw, _ = port_batch(gf, cs, mutate)
        wrong = [b for b in np.flatnonzero(pw != cs.want)]
        assert all(cs.want[b] == UNKNOWN and pw[b] >= 0 for b in wrong)
        if mutate == "count" and max(cs.T) < 2:     # (8,4) with a missing shard: no v = 2, no root search
            assert not wrong
        elif mutate == "count":
            assert any(cl[b] in "acd" for b in wrong), [cs.kind[b] for b in wrong]
            assert {cl[b] for b in wrong} <= set("acdf")
        elif k + m < 256 and call == "multi":
            assert any(cl[b] == "c" for b in wrong) and {cl[b] for b in wrong} <= set("acf")
        else:
            assert k + m < 256 or not wrong


def test_no_point_outside_a_code_of_256_shards(oracle, gf):
    bd = Builder(gf, 240, 256, range(256), 8, np.random.default_rng(1))
    assert bd.outside() is None
    with pytest.raises(ValueError):
        bd.pseudo(1, bd.outside())
    assert Builder(gf, 20, 30, range(30), 5, np.random.default_rng(1)).outside() >= 30
