"""The Cauchy matrix kind (include/fec_hip_matrix.h) without a device: the matrix the library builds
against the definition model (tests/cauchy_model.py), the properties the encode and decode routing
rest on, the ctx calls' argument checks, and the library's own self-test of the plan and locate
arithmetic with the log v table (fec__selftest_cauchy)."""
import ctypes
import itertools

import numpy as np
import pytest

import cauchy_model as cm

SHAPES = [(1, 1), (2, 1), (8, 4), (16, 8), (20, 10), (3, 29), (100, 156), (128, 128)]


@pytest.mark.parametrize("k,m", SHAPES)
def test_matrix_kind_equals_model(fec, k, m):
    got = fec.rs_matrix(k, m, kind=1)
    assert np.array_equal(got, cm.matrix(k, m))
    assert np.array_equal(fec.rs_matrix(k, m, kind="cauchy"), got)
    # kind 0 is fec_rs_matrix, through either C call
    out = np.zeros((k + m, k), dtype=np.uint8)
    assert fec.lib.fec_rs_matrix_kind(0, k, m, out.ctypes.data) == fec.FEC_OK
    assert np.array_equal(out, fec.rs_matrix(k, m))
    assert np.array_equal(fec.rs_matrix(k, m, kind="vandermonde"), out)


def test_known_answers(fec):
    assert bytes(fec.rs_matrix(8, 4, kind=1)[8]).hex() == "ad9ddd983daa5d96"
    assert bytes(fec.rs_matrix(2, 1, kind=1)[2]).hex() == "8ef4"
    assert bytes(fec.rs_matrix(2, 1)[2]).hex() == "0302"       # the row rs_encode23 is written for
    assert bytes(cm.matrix(8, 4)[8]).hex() == "ad9ddd983daa5d96"


def test_matrix_kind_argument_errors(fec):
    out = np.zeros((12, 8), dtype=np.uint8)
    f = fec.lib.fec_rs_matrix_kind
    assert f(2, 8, 4, out.ctypes.data) == fec.FEC_ERR_INVALID_ARG
    assert f(-1, 8, 4, out.ctypes.data) == fec.FEC_ERR_INVALID_ARG
    assert f(1, 8, 4, None) == fec.FEC_ERR_INVALID_ARG
    assert f(1, 0, 4, out.ctypes.data) == fec.FEC_ERR_INV_SHARD_NUM
    assert f(1, 8, -1, out.ctypes.data) == fec.FEC_ERR_INV_SHARD_NUM
    assert f(1, 200, 57, out.ctypes.data) == fec.FEC_ERR_MAX_SHARD_NUM
    assert not out.any()
    with pytest.raises(ValueError):
        fec.rs_matrix(8, 4, kind="jerasure")
    with pytest.raises(fec.FecError) as e:
        fec.rs_matrix(8, 4, kind=7)
    assert e.value.code == fec.FEC_ERR_INVALID_ARG


def test_ctx_matrix_calls_check_their_arguments_without_a_device(fec):
    kind = ctypes.c_int(5)
    assert fec.lib.fec_ctx_set_matrix(None, 0) == fec.FEC_ERR_INVALID_ARG
    assert fec.lib.fec_ctx_set_matrix(None, 1) == fec.FEC_ERR_INVALID_ARG
    assert fec.lib.fec_ctx_set_matrix(None, 9) == fec.FEC_ERR_INVALID_ARG
    assert fec.lib.fec_ctx_get_matrix(None, ctypes.byref(kind)) == fec.FEC_ERR_INVALID_ARG
    assert kind.value == 5
    assert fec.MATRIX_KINDS == {"vandermonde": 0, "cauchy": 1}


def test_every_square_row_subset_of_cauchy_4_4_is_invertible(fec):
    M = fec.rs_matrix(4, 4, kind=1)
    subsets = list(itertools.combinations(range(8), 4))
    assert len(subsets) == 70
    for rows in subsets:
        inv = cm.invert(M[list(rows)])
        assert inv is not None, rows
        prod = np.zeros((4, 4), dtype=np.uint8)
        for t in range(4):
            prod ^= cm.MUL[M[list(rows)][:, t][:, None], inv[t][None, :]]
        assert np.array_equal(prod, np.eye(4, dtype=np.uint8)), rows


def test_cauchy_8_4_is_dyadic(fec):
    """M[8 + r][j] = 1 / (8 ^ r ^ j) depends on r ^ j only: the property the dyadic RS(8,12) encode
    kernel needs of its matrix (fec_capi.cpp dyadic_leaves)."""
    P = fec.rs_matrix(8, 4, kind=1)[8:]
    for r in range(4):
        for j in range(8):
            assert P[r, j] == P[0, r ^ j]
    # the default RS(8,12) is dyadic too; the two differ
    D = fec.rs_matrix(8, 4)[8:]
    assert all(D[r, j] == D[0, r ^ j] for r in range(4) for j in range(8))
    assert not np.array_equal(P, D)


def test_model_rebuilds_what_it_encodes():
    rng = np.random.default_rng(5)
    for k, m in [(2, 1), (5, 3), (8, 4), (3, 5)]:
        M = cm.matrix(k, m)
        data = rng.integers(0, 256, (k, 19), dtype=np.uint8)
        full = np.concatenate([data, cm.encode(M, data)])
        for lost in itertools.combinations(range(k + m), min(m, 3)):
            present = np.ones(k + m, dtype=bool)
            present[list(lost)] = False
            assert np.array_equal(cm.rebuild(M, np.where(present[:, None], full, 0x5A), present), full)


def test_library_selftest_of_cauchy_plans_and_locate(fec):
    # the narrow, reconstruct-some and wide plan arithmetic with log v against rs::invert of the
    # Cauchy submatrix; the locate-multi / locate-partial column solver over Cauchy syndromes
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_cauchy() == 0
