"""Wide RS decode (codes of up to 256 shards), the parts that need no GPU: the two entry points are
declared and exported, the plan's coefficient arithmetic equals the inverse-matrix rows
(fec__selftest_wide_plan runs the functions the plan kernel runs), the argument checks that return
before any device work, and the bit order of wide_masks."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = ["fec_rs_reconstruct_wide_batch", "fec_rs_recover_wide_batch"]


def test_header_declares_and_library_exports_wide_calls(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(fec._LIB_PATH)
    for name in WIDE:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+FEC_MAX_WIDE_SHARDS\s+256\b", src)
    assert re.search(r"#define\s+FEC_MASK_WORDS\(n\)", src)
    assert re.search(r"#define\s+FEC_MAX_DECODE_SHARDS\s+32\b", src)   # the narrow limit stays
    assert fec.FEC_MAX_WIDE_SHARDS == 256 and fec.FEC_MAX_DECODE_SHARDS == 32
    assert [fec.mask_words(n) for n in (1, 32, 33, 64, 65, 255, 256)] == [1, 1, 2, 2, 3, 8, 8]


def test_wide_plan_coefficients_match_inverse_rows(fec):
    # RS(32,33), RS(20,33), RS(33,64), RS(64,80), RS(128,256), RS(255,256), RS(1,256), RS(8,12): 64
    # seeded recoverable masks each, plus all data lost where m >= k, against rs::invert of the
    # first-k-present submatrix of rs::build_matrix
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_wide_plan() == 0


def _recon(fec, k, m, L, W, flags):
    # no ctx, no buffers: every check below returns before any of them is used
    return fec.lib.fec_rs_reconstruct_wide_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, W, None, flags)


def _recover(fec, k, m, L, W, flags, slots=1):
    return fec.lib.fec_rs_recover_wide_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, W, None, 0, slots, None,
                                             flags)


@pytest.mark.parametrize("call", [_recon, _recover])
def test_wide_argument_errors_before_device_work(fec, call):
    D = fec.FEC_DEVICE
    assert call(fec, 200, 57, 16, 8, D) == fec.FEC_ERR_MAX_SHARD_NUM          # k + m = 257
    assert call(fec, 0, 4, 16, 1, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 4, -1, 16, 1, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 40, 20, 0, 2, D) == fec.FEC_ERR_SHARD_NO_DATA
    for W in (0, 9):
        assert call(fec, 40, 20, 16, W, D) == fec.FEC_ERR_INVALID_ARG
    assert call(fec, 20, 13, 16, 1, D) == fec.FEC_ERR_INVALID_ARG              # n = 33 needs two words
    assert call(fec, 40, 20, 16, 2, 7) == fec.FEC_ERR_INVALID_ARG              # bad flags
    # the order of the narrow calls: shard counts, flags, shard_len, then mask_words
    assert call(fec, 0, 4, 0, 0, 7) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 200, 57, 0, 0, 7) == fec.FEC_ERR_MAX_SHARD_NUM
    assert call(fec, 40, 20, 0, 0, 7) == fec.FEC_ERR_INVALID_ARG
    assert call(fec, 40, 20, 0, 0, D) == fec.FEC_ERR_SHARD_NO_DATA


def test_wide_recover_is_device_only(fec):
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED):
        assert _recover(fec, 40, 20, 16, 2, flags) == fec.FEC_ERR_INVALID_ARG
    assert _recover(fec, 40, 20, 16, 2, fec.FEC_DEVICE, slots=0) == fec.FEC_ERR_INVALID_ARG


def test_narrow_calls_still_refuse_more_than_32_shards(fec):
    rc = fec.lib.fec_rs_reconstruct_batch(None, 20, 13, 16, 1, None, 0, None, 0, 16, None, None, fec.FEC_DEVICE)
    assert rc == fec.FEC_ERR_MAX_SHARD_NUM


def test_wide_masks_bit_order(fec):
    idx = [0, 31, 32, 63, 64, 255]
    for i in idx:
        p = np.zeros((3, 256), dtype=bool)
        p[1, i] = True
        w = fec.wide_masks(p)
        assert w.dtype == np.uint32 and w.shape == (3, 8) and w.flags.c_contiguous
        want = np.zeros((3, 8), dtype=np.uint32)
        want[1, i // 32] = np.uint32(1) << np.uint32(i % 32)
        assert np.array_equal(w, want), i
    # widths that are no multiple of 32: the words a code of n shards needs, high bits clear
    w = fec.wide_masks(np.ones((2, 33), dtype=bool))
    assert w.shape == (2, 2) and np.array_equal(w, np.array([[0xFFFFFFFF, 1]] * 2, dtype=np.uint32))
    w = fec.wide_masks(np.ones((1, 12), dtype=bool))
    assert w.shape == (1, 1) and int(w[0, 0]) == 0xFFF
