"""Update and encode-idx (klauspost Update, EncodeIdx), the parts that need no GPU: both entry points
are declared with the right constness and exported, each has a row in the header's table, the six
Codec methods exist, the argument checks that return before any device work come in the uniform
calls' order with the mask_words bound following k (not k + m), and the per-launch argument fill of
a batch that the launch limit cuts (fec__selftest_update_slices) gives every launch the bases, mask
pointer, item count, row count and table base that the call's strides imply; and the slicing of a
batch that every call's launches share (fec__selftest_batch_slices)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fec_rs_update_batch", "fec_rs_encode_idx_batch")


def _params(name):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    d = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
    assert d, "%s is not declared" % name
    return d.group(1)


def test_header_declares_and_library_exports_both_calls(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    lib = ctypes.CDLL(fec._LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert re.search(r"^ \*\s+%s\b" % name, src, flags=re.M), "%s has no row in the header's table" % name
    for meth in ["rs_update_raw", "rs_update", "rs_update_split", "rs_encode_idx_raw", "rs_encode_idx",
                 "rs_encode_idx_split"]:
        assert callable(getattr(fec.Codec, meth)), meth


def test_parity_is_written_and_everything_else_only_read():
    u, e = _params(NAMES[0]), _params(NAMES[1])
    for p in (u, e):
        assert re.search(r"(?<!const )uint8_t\s*\*\s*parity\b", p), "parity is written: not const"
        assert re.search(r"size_t\s+mask_words\b", p)
    assert re.search(r"const\s+uint8_t\s*\*\s*old_data\b", u) and re.search(r"const\s+uint8_t\s*\*\s*new_data\b", u)
    assert re.search(r"const\s+uint32_t\s*\*\s*changed_mask\b", u)
    assert re.search(r"const\s+uint8_t\s*\*\s*data\b", e)
    assert re.search(r"const\s+uint32_t\s*\*\s*idx_mask\b", e)


def _update(fec, k, m, L, flags, W=1):
    # no ctx, no buffers: every check below returns before any of them is used
    return fec.lib.fec_rs_update_batch(None, k, m, L, 1, None, 0, None, 0, None, 0, 16, None, W, flags)


def _encode_idx(fec, k, m, L, flags, W=1):
    return fec.lib.fec_rs_encode_idx_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, W, flags)


@pytest.mark.parametrize("call", [_update, _encode_idx])
def test_argument_errors_before_device_work(fec, call):
    D = fec.FEC_DEVICE
    INV = fec.FEC_ERR_INVALID_ARG
    # shard counts
    assert call(fec, 0, 4, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 4, -1, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 200, 57, 16, D, 8) == fec.FEC_ERR_MAX_SHARD_NUM
    # flags: device memory only
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 7, -1):
        assert call(fec, 8, 4, 16, flags) == INV
    # shard_len
    assert call(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA
    assert call(fec, 8, 4, (1 << 30) + 1, D) == INV
    # mask_words: FEC_MASK_WORDS(k) .. 8
    assert call(fec, 8, 4, 16, D, 0) == INV
    assert call(fec, 8, 4, 16, D, 9) == INV
    assert call(fec, 40, 4, 16, D, fec.mask_words(40) - 1) == INV
    # the order: shard counts, then k + m, then flags, then shard_len, then mask_words, then the ctx
    assert call(fec, 0, 4, 0, 7, 9) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 200, 57, 0, 7, 9) == fec.FEC_ERR_MAX_SHARD_NUM
    assert call(fec, 8, 4, 0, 7, 9) == INV                       # flags before shard_len
    assert call(fec, 8, 4, 0, fec.FEC_HOST, 9) == INV
    assert call(fec, 8, 4, 0, D, 9) == fec.FEC_ERR_SHARD_NO_DATA     # shard_len before mask_words
    assert call(fec, 8, 4, 0, D, 0) == fec.FEC_ERR_SHARD_NO_DATA
    assert call(fec, 8, 4, 16, D, 1) == INV                      # no ctx


def _reaches_ctx(fec, call, k, m, W):
    """The code passes the shard-count checks (a shard_len of 0 is what stops it), and with a good
    shard_len the call ends at the missing ctx. That code is FEC_ERR_INVALID_ARG, as a refused
    mask_words is: that these word counts are accepted is shown where a ctx exists
    (test_gpu_update.py runs RS(100,156) with 4 words and RS(130,20) with 5)."""
    D = fec.FEC_DEVICE
    assert call(fec, k, m, 0, D, W) == fec.FEC_ERR_SHARD_NO_DATA
    return call(fec, k, m, 16, D, W) == fec.FEC_ERR_INVALID_ARG


@pytest.mark.parametrize("call", [_update, _encode_idx])
def test_the_mask_bound_follows_k_not_k_plus_m(fec, call):
    assert _reaches_ctx(fec, call, 100, 156, 8)
    assert _reaches_ctx(fec, call, 255, 1, 8)
    assert _reaches_ctx(fec, call, 32, 0, 1)
    # four words cover 100 columns although the code has 256 shards; three do not
    assert _reaches_ctx(fec, call, 100, 156, 4)
    assert call(fec, 100, 156, 16, fec.FEC_DEVICE, 3) == fec.FEC_ERR_INVALID_ARG
    # one word covers the 8 columns of a code of 40 shards
    assert _reaches_ctx(fec, call, 8, 32, 1)


def test_launch_arguments_of_a_cut_batch(fec):
    # k = 5, m = 20, 70 000-byte shards, one block past kMaxItems / 4375: two launches of two row passes;
    # region bases, mask pointer, total, m and table base of each against the call's strides
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_update_slices() == 0


def test_a_slice_of_a_batch_moves_each_base_by_its_own_stride(fec):
    # the one function every core and host chunk slices with: data, parity, out, mask and status bases
    # of blocks [b0, b0 + nb) of a layout whose strides all differ; nothing else moves
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_batch_slices() == 0
