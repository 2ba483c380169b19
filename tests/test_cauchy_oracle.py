"""cauchy_oracle.py without a device: the stand-in's three members against the oracle's field and the
definition model, and the multipliers, which come from the matrix alone, against the Berlekamp-Welch
model's syndromes: a Cauchy codeword divided shard by shard by v is the values of one polynomial of
degree < k at the points 0 .. n - 1, and undivided it is not.

Why the codes of the Cauchy tests are what they are: where every data shard has the same multiplier,
a term log v_o - log v_s that is wrong between data shards cancels. That holds for RS(8,12) (k a power
of two), the most tested code, and is asserted here, beside its failing for the others.
"""
import numpy as np
import pytest

import cauchy_model as cm
import cauchy_oracle as co
from arena import gf, oracle_arena, shards  # noqa: F401
from locate_hard_cases import CAUCHY_CODES
from locate_model import syndromes

# the codes of test_gpu_cauchy_patterns.py, of the Cauchy batches of locate_hard_cases.py and of the
# kind-switch sequence of test_gpu_cauchy.py
PATTERN_CODES = [(8, 4), (5, 3), (12, 5), (4, 8), (16, 8), (20, 10), (33, 7)]
CODES = sorted(set(PATTERN_CODES + CAUCHY_CODES + [(12, 5), (2, 1), (20, 10), (4, 16)]))


def test_field_equals_the_oracles(oracle, gf):
    mul, inv = co.gf()
    assert np.array_equal(mul, gf[0]) and np.array_equal(inv, gf[1])
    rng = np.random.default_rng(1)
    for a, b in rng.integers(0, 256, (200, 2)):
        assert co.gf_mul(int(a), int(b)) == oracle.gf_mul(int(a), int(b)) == mul[a, b]


@pytest.mark.parametrize("k,m", CODES)
def test_encode_and_matrix_equal_the_model(k, m):
    rng = np.random.default_rng(k * m)
    M = co.build_matrix(k, k + m)
    assert np.array_equal(M, cm.matrix(k, m))
    sh = rng.integers(0, 256, (3, k + m, 19), dtype=np.uint8)
    data = sh[:, :k].copy()
    assert co.rs_encode(k, m, sh) is sh
    assert np.array_equal(sh[:, :k], data) and np.array_equal(sh[:, k:], cm.encode(M, data))
    one = sh[0].copy()
    one[k:] = 0
    co.rs_encode(k, m, one)
    assert np.array_equal(one, sh[0])
    # through the arena, as the locate helpers use it
    img, d, p = oracle_arena(co, "split", k, m, 19, 3, np.random.default_rng(7))
    got = shards(img, d, p)[:, :, :19]
    assert np.array_equal(got[:, k:], cm.encode(M, got[:, :k]))


@pytest.mark.parametrize("k,m", CODES)
def test_codewords_divided_by_the_multipliers_are_polynomial_values(gf, k, m):
    rng = np.random.default_rng(k + m)
    n = k + m
    v = co.code_multipliers(k, m)
    assert v[0] == 1 and v.all()
    sh = rng.integers(1, 256, (n, 23), dtype=np.uint8)
    co.rs_encode(k, m, sh)
    pts = list(range(n))
    assert not syndromes(gf, pts, sh, k, v).any()
    assert not syndromes(gf, pts, gf[0][gf[1][v][:, None], sh], k).any()
    assert syndromes(gf, pts, sh, k).any(axis=0).all(), "the code is not the one with multipliers one"
    # a punctured set of shards, as locate-partial sees it
    P = sorted(int(r) for r in rng.permutation(n)[:k + 1])
    assert not syndromes(gf, P, sh[P], k, v).any()


@pytest.mark.parametrize("k,m", [(8, 4), (20, 10), (5, 3), (40, 16), (240, 16)])
def test_multipliers_of_the_default_matrix_are_one(oracle, k, m):
    assert (co.multipliers(oracle.build_matrix(k, k + m)) == 1).all()


@pytest.mark.parametrize("k,m", CODES)
def test_data_multipliers_differ_except_where_k_is_a_power_of_two(k, m):
    v = co.code_multipliers(k, m)
    if k & (k - 1) == 0:
        # every data shard of RS(8,12) has one multiplier, and of (4,8), (16,8), (4,16) and (2,1): a term
        # wrong between data shards cancels there, and only patterns that mix data and parity can see it
        assert len(set(v[:k].tolist())) == 1
    else:
        assert len(set(v[:k].tolist())) > 1
    # between data and parity the multipliers differ in every code
    assert set(v[k:].tolist()) - set(v[:k].tolist())
    if (k, m) == (20, 10):
        assert len(set(v[:4].tolist())) == 1 and len(set(v[:k].tolist())) > 1


def test_multipliers_reject_a_matrix_that_is_no_grs_code():
    M = cm.matrix(5, 3).copy()
    M[6, 2] ^= 1
    with pytest.raises(AssertionError):
        co.multipliers(M)
