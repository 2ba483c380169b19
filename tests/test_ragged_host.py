"""Ragged batches (a shard length per block), the parts that need no GPU: the three entry points are
declared and exported, the item arithmetic of the kernels covers every (block, chunk) exactly once
(fec__selftest_ragged_tiles walks the functions the kernels run), and the argument checks that
return before any device work, in the uniform calls' order."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ["fec_rs_encode_ragged_batch", "fec_rs_reconstruct_ragged_batch", "fec_rs_recover_ragged_batch"]


def test_header_declares_and_library_exports_ragged_calls(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(fec._LIB_PATH)
    for name in RAGGED:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, name
        assert re.search(r"\bmax_shard_len\b", decl.group(1)) and re.search(r"const\s+uint32_t\s*\*\s*block_len\b",
                                                                            decl.group(1)), name
        assert re.search(r"int32_t\s*\*\s*block_status\b", decl.group(1)), name
        assert hasattr(lib, name), name
    assert fec.Codec.TUNING_KEYS["rag_g"] == 18 and len(fec.Codec.TUNING_KEYS) == 19
    for meth in ["rs_encode_ragged", "rs_encode_ragged_split", "rs_reconstruct_ragged", "rs_reconstruct_ragged_split",
                 "rs_recover_ragged_split", "rs_encode_ragged_raw", "rs_reconstruct_ragged_raw",
                 "rs_recover_ragged_raw"]:
        assert callable(getattr(fec.Codec, meth)), meth


def test_ragged_item_arithmetic_covers_every_chunk_once(fec):
    # all-zero tiles, a zero run across a tile edge (with oversize blocks in it), a single block,
    # tile and window sums at a multiple of 256 and one off either side, several windows per tile,
    # a 2^26-chunk shard: every item of every tile and window maps to one (block, chunk) with
    # chunk < the block's count, and every (block, chunk) is met once
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_ragged_tiles() == 0


def _encode(fec, k, m, L, flags, slots=1):
    # no ctx, no buffers: every check below returns before any of them is used
    return fec.lib.fec_rs_encode_ragged_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, flags)


def _recon(fec, k, m, L, flags, slots=1):
    return fec.lib.fec_rs_reconstruct_ragged_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, None, flags)


def _recover(fec, k, m, L, flags, slots=1):
    return fec.lib.fec_rs_recover_ragged_batch(None, k, m, L, 1, None, 0, None, 0, 16, None, None, None, 0, slots,
                                               None, flags)


@pytest.mark.parametrize("call", [_encode, _recon, _recover])
def test_ragged_argument_errors_before_device_work(fec, call):
    D = fec.FEC_DEVICE
    # shard counts
    assert call(fec, 0, 4, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 4, -1, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 200, 57, 16, D) == fec.FEC_ERR_MAX_SHARD_NUM              # k + m = 257
    # flags: device memory only
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 7, -1):
        assert call(fec, 8, 4, 16, flags) == fec.FEC_ERR_INVALID_ARG
    # max_shard_len
    assert call(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA
    assert call(fec, 8, 4, (1 << 30) + 1, D) == fec.FEC_ERR_INVALID_ARG
    # the order of the uniform calls: shard counts, then flags, then max_shard_len
    assert call(fec, 0, 4, 0, 7) == fec.FEC_ERR_INV_SHARD_NUM
    assert call(fec, 200, 57, 0, 7) == fec.FEC_ERR_MAX_SHARD_NUM
    assert call(fec, 8, 4, 0, 7) == fec.FEC_ERR_INVALID_ARG
    assert call(fec, 8, 4, 0, fec.FEC_HOST) == fec.FEC_ERR_INVALID_ARG
    assert call(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA


@pytest.mark.parametrize("call", [_recon, _recover])
def test_ragged_decode_refuses_more_than_32_shards(fec, call):
    assert call(fec, 20, 13, 16, fec.FEC_DEVICE) == fec.FEC_ERR_MAX_SHARD_NUM  # n = 33
    assert call(fec, 20, 13, 0, 7) == fec.FEC_ERR_MAX_SHARD_NUM                # before flags and length


def test_ragged_recover_out_slots(fec):
    D = fec.FEC_DEVICE
    for slots in (0, -1):
        assert _recover(fec, 8, 4, 16, D, slots=slots) == fec.FEC_ERR_INVALID_ARG
    # after max_shard_len == 0, as in fec_rs_recover_batch
    assert _recover(fec, 8, 4, 0, D, slots=0) == fec.FEC_ERR_SHARD_NO_DATA
    assert _recover(fec, 8, 4, (1 << 30) + 1, D, slots=0) == fec.FEC_ERR_INVALID_ARG


def test_shard_size_error_has_a_message(fec):
    msg = fec.lib.fec_strerror(fec.FEC_ERR_SHARD_SIZE)
    assert msg and msg != fec.lib.fec_strerror(12345)
