"""Custom code matrices (include/fec_hip_matrix.h fec_ctx_set_custom_matrix) without a device: the
library's self-test of the elimination plan, the same solver swept through its test hook against the
definition model (tests/custom_model.py), and the argument checks of the new entry point."""
import ctypes
import os
import re

import numpy as np
import pytest

import custom_model as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def clib(fec):
    lib = ctypes.CDLL(fec._LIB_PATH)
    lib.fec__custom_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def word(present):
    return int(sum(1 << int(i) for i in np.nonzero(present)[0]))


def plan(clib, P, present, want=ALL):
    """The hook's answer: a status, or (inputs [k], outputs [nout], coefficient rows [nout, k])."""
    m, k = P.shape
    P = np.ascontiguousarray(P)
    ins, outs, coef = np.zeros(k, np.uint8), np.zeros(m, np.uint8), np.zeros((m, k), np.uint8)
    rc = clib.fec__custom_plan(k, m, P.ctypes.data, word(present), want, ins.ctypes.data, outs.ctypes.data,
                               coef.ctypes.data)
    return rc if rc <= 0 else (ins, outs[:rc], coef[:rc])


def check_pattern(fec, clib, P, present, want=ALL):
    M = cu.matrix(P)
    n, k = M.shape
    got = plan(clib, P, present, want)
    missing = [i for i in range(n) if not present[i] and (want >> i) & 1]
    ref = cu.decode(M, present)
    if not missing:
        assert got == 0
    elif ref is cu.TOO_FEW:
        assert got == fec.FEC_ERR_TOO_FEW_SHARDS
    elif ref is cu.SINGULAR:
        assert got == fec.FEC_ERR_SINGULAR                     # exactly where invert() returns None
    else:
        S, T = ref
        ins, outs, coef = got
        assert np.array_equal(ins, S)                          # the first k present shards
        assert list(outs) == missing
        assert np.array_equal(coef, T[missing])


def test_library_selftest_of_the_elimination_plan(fec):
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_custom_plan() == 0


@pytest.mark.parametrize("name", cu.NAMES)
def test_every_pattern_of_8_4_against_the_model(fec, clib, name):
    P = cu.rows(name, 8, 4, fec)
    pats, sing = cu.check_8_4(name, P)
    for p in pats:
        check_pattern(fec, clib, P, p)
    # too few: five shards missing
    for p in cu.patterns(12, 8, [5]):
        check_pattern(fec, clib, P, p)
    # want masks: one data shard, one parity shard, what is missing, nothing
    for p in pats[::7]:
        for want in (1 << int(np.nonzero(~p)[0][0]), 1 << 9, word(~p), 0):
            check_pattern(fec, clib, P, p, want)


@pytest.mark.parametrize("k,m", [(20, 10), (16, 8), (16, 16), (1, 31), (31, 1)])
def test_drawn_patterns_of_other_shapes(fec, clib, k, m):
    rng = np.random.default_rng(100 * k + m)
    P = cu.rows("cauchy255", k, m)
    n = k + m
    for _ in range(48):
        p = np.ones(n, dtype=bool)
        p[rng.choice(n, size=int(rng.integers(1, m + 2)), replace=False)] = False
        check_pattern(fec, clib, P, p)
        check_pattern(fec, clib, P, p, 1 << int(rng.integers(0, n)))


def test_lrc_row_swap_and_single_erasure(fec, clib):
    P = cu.rows("lrc", 8, 4)
    p = np.ones(12, dtype=bool)
    p[[0, 4, 8]] = False           # parity rows 1 and 2 serve: A = [[0, 1], [x, y]], a swap, not a failure
    assert P[1, 0] == 0 and P[1, 4] == 1
    ins, outs, coef = plan(clib, P, p)
    assert list(ins) == [1, 2, 3, 5, 6, 7, 9, 10] and list(outs) == [0, 4, 8]
    p = np.ones(12, dtype=bool)
    p[4] = False                   # parity 8 is the first present one and does not cover column 4
    assert plan(clib, P, p) == fec.FEC_ERR_SINGULAR
    p[8] = False                   # the caller steers: with parity 8 cleared, parity 9 serves
    ins, outs, coef = plan(clib, P, p, 1 << 4)
    assert list(ins) == [0, 1, 2, 3, 5, 6, 7, 9] and list(outs) == [4]


def test_argument_checks_without_a_device(fec):
    f = fec.lib.fec_ctx_set_custom_matrix
    rows = np.ones((4, 8), dtype=np.uint8)
    assert f(None, 8, 4, rows.ctypes.data) == fec.FEC_ERR_INVALID_ARG
    assert f(None, 8, 4, None) == fec.FEC_ERR_INVALID_ARG
    assert f(None, 0, 4, rows.ctypes.data) == fec.FEC_ERR_INV_SHARD_NUM
    assert f(None, 8, -1, rows.ctypes.data) == fec.FEC_ERR_INV_SHARD_NUM
    assert f(None, 200, 57, rows.ctypes.data) == fec.FEC_ERR_MAX_SHARD_NUM
    assert (fec.FEC_MATRIX_CUSTOM, fec.FEC_ERR_SINGULAR, fec.FEC_ERR_NO_MATRIX) == (2, -11, -12)
    # kind 2 has nothing to generate; an unknown kind stays refused
    out = np.zeros((12, 8), dtype=np.uint8)
    assert fec.lib.fec_rs_matrix_kind(2, 8, 4, out.ctypes.data) == fec.FEC_ERR_INVALID_ARG
    assert fec.lib.fec_ctx_set_matrix(None, 2) == fec.FEC_ERR_INVALID_ARG
    assert fec.MATRIX_KINDS == {"vandermonde": 0, "cauchy": 1}
    with pytest.raises(ValueError):
        fec.rs_matrix(8, 4, kind="custom")


def test_strerror_names_the_new_codes(fec):
    unknown = fec.lib.fec_strerror(-99)
    texts = {fec.lib.fec_strerror(c) for c in (fec.FEC_ERR_SINGULAR, fec.FEC_ERR_NO_MATRIX)}
    assert len(texts) == 2 and unknown not in texts
    assert fec.lib.fec_strerror(fec.FEC_ERR_SINGULAR) == b"matrix is singular"      # klauspost errSingular


def test_header_declares_what_the_library_exports(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip_matrix.h")).read()
    assert re.search(r"#define\s+FEC_MATRIX_CUSTOM\s+2\b", src)
    assert re.search(r"\bint\s+fec_ctx_set_custom_matrix\s*\(\s*fec_ctx\s*\*\s*ctx\s*,\s*int\s+k\s*,\s*int\s+m\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*parity_rows\s*\)\s*;", src)
    hip = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    assert re.search(r"#define\s+FEC_ERR_SINGULAR\s+\(-11\)", hip)
    assert re.search(r"#define\s+FEC_ERR_NO_MATRIX\s+\(-12\)", hip)
    lib = ctypes.CDLL(fec._LIB_PATH)
    for name in ("fec_ctx_set_custom_matrix", "fec__selftest_custom_plan", "fec__custom_plan"):
        assert hasattr(lib, name)
