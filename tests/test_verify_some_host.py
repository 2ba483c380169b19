"""Verify and reconstruct-some (klauspost Verify, Reconstruct / ReconstructSome), the parts that need
no GPU: both entry points are declared and exported, the plan records of reconstruct-some equal the
rows of the systematic matrix times the inverse of the first-k-present rows for every missing shard,
parity rows included (fec__selftest_some_plan runs the function the plan kernel runs), and the
argument checks that return before any device work, in the uniform calls' order."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_both_calls(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(fec._LIB_PATH)
    v = re.search(r"\bint\s+fec_rs_verify_batch\s*\(([^;]*)\)\s*;", code)
    assert v
    assert re.search(r"const\s+uint8_t\s*\*\s*data\b", v.group(1)) and re.search(r"const\s+uint8_t\s*\*\s*parity\b",
                                                                                v.group(1))
    assert re.search(r"int32_t\s*\*\s*block_status\b", v.group(1))
    assert re.search(r"uint32_t\s*\*\s*mismatch_count\b", v.group(1))
    s = re.search(r"\bint\s+fec_rs_reconstruct_some_batch\s*\(([^;]*)\)\s*;", code)
    assert s
    assert re.search(r"(?<!const )uint8_t\s*\*\s*parity\b", s.group(1)), "parity is written: not const"
    assert re.search(r"const\s+uint32_t\s*\*\s*present_mask\b", s.group(1))
    assert re.search(r"const\s+uint32_t\s*\*\s*want_mask\b", s.group(1))
    assert re.search(r"int32_t\s*\*\s*block_status\b", s.group(1))
    for name in ("fec_rs_verify_batch", "fec_rs_reconstruct_some_batch"):
        assert hasattr(lib, name), name
        assert re.search(r"^ \*\s+%s\b" % name, src, flags=re.M), "%s has no row in the header's table" % name
    for meth in ["rs_verify_raw", "rs_verify", "rs_verify_split", "rs_reconstruct_some_raw", "rs_reconstruct_some",
                 "rs_reconstruct_some_split"]:
        assert callable(getattr(fec.Codec, meth)), meth


def test_some_plan_rows_equal_matrix_times_inverse(fec):
    # RS(8,12), RS(2,3), RS(20,30), RS(10,32), RS(1,32), RS(31,32): 64 seeded recoverable masks each,
    # all parity lost, exactly k present and all of them parity (m >= k); every missing shard's row
    # against M[s] * inverse(rows of the first k present); want masks, stray bits, k - 1 present
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_some_plan() == 0


def _verify(fec, k, m, L, flags):
    # no ctx, no buffers: every check below returns before any of them is used
    return fec.lib.fec_rs_verify_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, flags)


def _some(fec, k, m, L, flags):
    return fec.lib.fec_rs_reconstruct_some_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, None, flags)


@pytest.mark.parametrize("call,too_many", [(_verify, (200, 57)), (_some, (20, 13))])
def test_argument_errors_before_device_work(fec, call, too_many):
    D = fec.FEC_DEVICE
    K, M = too_many                                                             # k + m = 257 / 33
    # shard counts
    assert call(fec, 0, 4, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 4, -1, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, K, M, 16, D) == fec.FEC_ERR_MAX_SHARD_NUM
    # flags: device memory only
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 7, -1):
        assert call(fec, 8, 4, 16, flags) == fec.FEC_ERR_INVALID_ARG
    # shard_len
    assert call(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA
    assert call(fec, 8, 4, (1 << 30) + 1, D) == fec.FEC_ERR_INVALID_ARG
    # the order of the uniform calls: shard counts, then flags, then shard_len, then the ctx
    assert call(fec, 0, 4, 0, 7) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, K, M, 0, 7) == fec.FEC_ERR_MAX_SHARD_NUM
    assert call(fec, 8, 4, 0, 7) == fec.FEC_ERR_INVALID_ARG
    assert call(fec, 8, 4, 0, fec.FEC_HOST) == fec.FEC_ERR_INVALID_ARG
    assert call(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA
    assert call(fec, 8, 4, 16, D) == fec.FEC_ERR_INVALID_ARG                    # no ctx


def test_limits_of_the_two_calls(fec):
    D = fec.FEC_DEVICE
    # verify takes every code the encode takes; reconstruct-some the narrow decode's 32 shards: the
    # calls below pass the shard-count check and stop at the missing ctx
    assert _verify(fec, 100, 156, 16, D) == fec.FEC_ERR_INVALID_ARG
    assert _verify(fec, 32, 0, 16, D) == fec.FEC_ERR_INVALID_ARG
    assert _some(fec, 1, 31, 16, D) == fec.FEC_ERR_INVALID_ARG
    assert _some(fec, 32, 0, 16, D) == fec.FEC_ERR_INVALID_ARG
    assert _some(fec, 32, 1, 16, D) == fec.FEC_ERR_MAX_SHARD_NUM
