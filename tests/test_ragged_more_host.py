"""Ragged verify and ragged reconstruct-some (include/fec_hip_ragged.h), the parts that need no GPU:
the header declares them and the library exports them, the host-side arithmetic of the
reconstruct-some tile (blocks per tile, LDS size, row passes) holds over every narrow code
(fec__selftest_ragged_some), and the argument checks that return before the ctx is looked at come in
the uniform calls' order."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _verify(fec, k, m, L, flags):
    # no ctx, no buffers: every check below returns before any of them is used
    return fec.lib.fec_rs_verify_ragged_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, None, flags)


def _some(fec, k, m, L, flags):
    return fec.lib.fec_rs_reconstruct_some_ragged_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, None, None,
                                                        flags)


# this file's own call table: the entry point, its limit on k + m
CALLS = [(_verify, 256), (_some, 32)]


def test_header_declares_and_library_exports_the_two_calls(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip_ragged.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(fec._LIB_PATH)
    for name, extra in [("fec_rs_verify_ragged_batch", r"uint32_t\s*\*\s*mismatch_count\b"),
                        ("fec_rs_reconstruct_some_ragged_batch", r"const\s+uint32_t\s*\*\s*want_mask\b")]:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, name
        args = decl.group(1)
        assert re.search(r"\bmax_shard_len\b", args) and re.search(r"const\s+uint32_t\s*\*\s*block_len\b", args), name
        assert re.search(r"int32_t\s*\*\s*block_status\b", args) and re.search(extra, args), name
        assert hasattr(lib, name), name
    for meth in ["rs_verify_ragged_raw", "rs_verify_ragged", "rs_verify_ragged_split", "rs_reconstruct_some_ragged_raw",
                 "rs_reconstruct_some_ragged", "rs_reconstruct_some_ragged_split"]:
        assert callable(getattr(fec.Codec, meth)), meth
    # the overview and the shard limits of fec_hip.h name them
    top = open(os.path.join(ROOT, "include", "fec_hip.h")).read().split("#ifndef FEC_HIP_H")[0]
    assert "fec_rs_verify_ragged_batch" in top and "fec_rs_reconstruct_some_ragged_batch" in top


def test_reconstruct_some_tile_arithmetic(fec):
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_ragged_some() == 0


@pytest.mark.parametrize("call,max_n", CALLS)
def test_argument_errors_come_in_the_documented_order(fec, call, max_n):
    D = fec.FEC_DEVICE
    INV, NUM, MAX, NODATA = (fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_INV_SHARD_NUM, fec.FEC_ERR_MAX_SHARD_NUM,
                             fec.FEC_ERR_SHARD_NO_DATA)
    over = (max_n - 1, 2)      # k + m one above the call's limit
    # shard counts
    assert call(fec, 0, 4, 16, D) == NUM and call(fec, -1, 4, 16, D) == NUM and call(fec, 4, -1, 16, D) == NUM
    assert call(fec, 300, -1, 16, D) == NUM
    # k + m against 256 / 32; the limit itself passes on to the ctx check
    assert call(fec, *over, 16, D) == MAX
    assert call(fec, max_n - 1, 1, 16, D) == INV
    # flags: device memory only (1 and 2, the host kinds, are refused)
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 3, 7, -1):
        assert call(fec, 8, 4, 16, flags) == INV
    # max_shard_len
    assert call(fec, 8, 4, 0, D) == NODATA
    assert call(fec, 8, 4, (1 << 30) + 1, D) == INV
    # a length of 2^30 passes every check before the ctx, which is null
    assert call(fec, 8, 4, 1 << 30, D) == INV and call(fec, 8, 4, 17, D) == INV
    # pairs of bad arguments pin the order: counts, the limit, flags, the length, the ctx
    assert call(fec, 0, 4, 0, 7) == NUM and call(fec, 0, over[1] + 400, 0, 7) == NUM
    assert call(fec, *over, 0, 7) == MAX and call(fec, *over, 0, D) == MAX
    assert call(fec, 8, 4, 0, 7) == INV and call(fec, 8, 4, 0, fec.FEC_HOST) == INV
    assert call(fec, 8, 4, 0, fec.FEC_HOST_PINNED) == INV
    assert call(fec, 8, 4, 0, D) == NODATA


def test_reconstruct_some_refuses_more_than_32_shards_and_verify_takes_them(fec):
    assert _some(fec, 20, 13, 16, fec.FEC_DEVICE) == fec.FEC_ERR_MAX_SHARD_NUM
    assert _verify(fec, 20, 13, 16, fec.FEC_DEVICE) == fec.FEC_ERR_INVALID_ARG      # on to the null ctx
    assert _verify(fec, 200, 57, 16, fec.FEC_DEVICE) == fec.FEC_ERR_MAX_SHARD_NUM
