"""Wide reconstruct-some (fec_rs_reconstruct_some_wide_batch, include/fec_hip_some_wide.h), the parts
that need no GPU: the call is declared in its own header and exported, the Codec methods exist, the
multi-word plan records equal the inverse-matrix rows (fec__selftest_some_wide_plan), and the argument
checks that return before any device work run in the locate calls' order."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fec_rs_reconstruct_some_wide_batch"


def _code(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_and_library_exports_the_call(fec):
    code = _code("fec_hip_some_wide.h")
    assert re.search(r'#include\s+"fec_hip.h"', code)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, code)
    assert decl, "declared in fec_hip_some_wide.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["fec_ctx *ctx", "int k", "int m", "size_t shard_len", "size_t nblocks", "uint8_t *data",
                    "size_t data_block_stride", "uint8_t *parity", "size_t parity_block_stride",
                    "size_t shard_stride", "const uint32_t *present_mask", "const uint32_t *want_mask",
                    "size_t mask_words", "int32_t *block_status", "int flags"]
    # fec_hip.h declares nothing new: its comments alone speak of the call
    assert NAME not in _code("fec_hip.h")
    assert NAME in open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    assert hasattr(ctypes.CDLL(fec._LIB_PATH), NAME)
    assert len(fec.lib.fec_rs_reconstruct_some_wide_batch.argtypes) == 15
    for method in ("rs_reconstruct_some_wide_raw", "rs_reconstruct_some_wide", "rs_reconstruct_some_wide_split"):
        assert callable(getattr(fec.Codec, method)), method


def test_some_wide_plan_records_match_inverse_rows(fec):
    # RS(20,33), RS(33,65), RS(64,80), RS(16,256), RS(128,256), RS(1,256), RS(255,256): 64 masks each (all
    # parity lost; k present, all parity; shards 31, 32, 63, 64 lost; seeded losses), each with a want
    # subset, stray bits and k - 1 present, every row against M[o] * inverse(M[S]) of rs_matrix.hpp
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_some_wide_plan() == 0
    assert lib.fec__selftest_some_plan() == 0     # the one-word form is the same function


def _call(fec, k, m, L, W, flags, nblocks=1):
    # no ctx, no buffers: every check below returns before any of them is used
    return fec.lib.fec_rs_reconstruct_some_wide_batch(None, k, m, L, nblocks, None, 0, None, 0, 16, None, None, W,
                                                      None, flags)


def test_argument_errors_before_device_work(fec):
    D = fec.FEC_DEVICE
    INV, NUM, MAX, NODATA = (fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_INV_SHARD_NUM, fec.FEC_ERR_MAX_SHARD_NUM,
                             fec.FEC_ERR_SHARD_NO_DATA)
    assert _call(fec, 200, 57, 16, 8, D) == MAX                     # k + m = 257
    assert _call(fec, 0, 4, 16, 1, D) == NUM
    assert _call(fec, 4, -1, 16, 1, D) == NUM
    assert _call(fec, 300, -1, 16, 8, D) == NUM                     # the counts before their sum
    # k + m = 256 passes the count check: the next bad argument is reported
    for k, m in ((100, 156), (1, 255)):
        assert _call(fec, k, m, 0, 8, D) == NODATA
        assert _call(fec, k, m, 16, 7, D) == INV                    # FEC_MASK_WORDS(256) - 1
        assert _call(fec, k, m, 16, 8, D) == INV                    # passes every check: the null ctx
    # FEC_DEVICE only
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 3, -1):
        assert _call(fec, 40, 20, 16, 2, flags) == INV
    assert _call(fec, 40, 20, 0, 2, D) == NODATA
    assert _call(fec, 40, 20, (1 << 30) + 1, 2, D) == INV
    # mask_words: 0, FEC_MASK_WORDS(n) - 1, 9
    for W in (0, 1, 9):
        assert _call(fec, 40, 20, 16, W, D) == INV
    assert _call(fec, 64, 16, 16, 2, D) == INV                      # n = 80 needs three words
    assert _call(fec, 20, 13, 16, 1, D) == INV                      # n = 33 needs two words
    # a code of 33 shards with one word does not forward: the narrow call would say MAX_SHARD_NUM,
    # as it still does when called itself
    assert _call(fec, 32, 1, 16, 1, D) == INV
    assert fec.lib.fec_rs_reconstruct_some_batch(None, 32, 1, 16, 1, None, 0, None, 0, 16, None, None, None,
                                                 D) == MAX
    # the order: shard counts, k + m, flags, shard_len, mask_words, then the ctx
    assert _call(fec, 0, 4, 0, 0, 7) == NUM
    assert _call(fec, 200, 57, 0, 0, 7) == MAX
    assert _call(fec, 40, 20, 0, 0, 7) == INV                       # flags before shard_len ...
    assert _call(fec, 40, 20, 0, 0, D) == NODATA                    # ... shard_len before mask_words
    assert _call(fec, 40, 20, 0, 9, D) == NODATA
    assert _call(fec, 40, 20, 16, 9, D, nblocks=0) == INV           # mask_words before the empty batch
    # one word and a narrow code: the narrow call's checks, the same codes
    assert _call(fec, 8, 4, 0, 1, D) == NODATA
    assert _call(fec, 8, 4, 16, 1, 7) == INV
    assert _call(fec, 8, 4, 16, 1, D) == INV                        # the null ctx
    assert _call(fec, 8, 4, 0, 2, D) == NODATA                      # two words: the wide path, the same order


def test_narrow_call_still_refuses_more_than_32_shards(fec):
    rc = fec.lib.fec_rs_reconstruct_some_batch(None, 20, 13, 16, 1, None, 0, None, 0, 16, None, None, None,
                                               fec.FEC_DEVICE)
    assert rc == fec.FEC_ERR_MAX_SHARD_NUM
