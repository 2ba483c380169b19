"""fec_rs_locate_batch (which shard of a block that fails verify is the corrupt one), the parts that
need no GPU: the entry point and its two verdict constants are declared, exported and have a row in
the header's table, the Codec methods exist, the arithmetic the kernel shares with the host
(fec__selftest_locate: the ratio table, the per-chunk classifier, the merge rule) equals the
brute-force definition, the per-launch argument fill of a batch that the launch limit cuts
(fec__selftest_locate_slices) gives every pass and every finalize the bases, rows and tables that the
call's strides imply, and the argument checks that return before any device work come in the uniform
calls' order."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fec_rs_locate_batch"


def test_header_declares_and_library_exports_the_call(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    d = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, code)
    assert d, "%s is not declared" % NAME
    p = d.group(1)
    assert re.search(r"const\s+uint8_t\s*\*\s*data\b", p) and re.search(r"const\s+uint8_t\s*\*\s*parity\b", p)
    assert re.search(r"(?<!const )int32_t\s*\*\s*bad_shard\b", p)
    assert re.search(r"(?<!const )uint32_t\s*\*\s*present_out\b", p)
    assert re.search(r"size_t\s+mask_words\b", p)
    assert re.search(r"(?<!const )uint32_t\s*\*\s*counts\b", p)
    assert re.search(r"^#define\s+FEC_LOCATE_CLEAN\s+\(-1\)", code, flags=re.M)
    assert re.search(r"^#define\s+FEC_LOCATE_UNKNOWN\s+\(-2\)", code, flags=re.M)
    assert re.search(r"^ \*\s+%s\b" % NAME, src, flags=re.M), "%s has no row in the header's table" % NAME
    assert hasattr(ctypes.CDLL(fec._LIB_PATH), NAME)
    assert (fec.FEC_LOCATE_CLEAN, fec.FEC_LOCATE_UNKNOWN) == (-1, -2)
    for meth in ["rs_locate_raw", "rs_locate", "rs_locate_split"]:
        assert callable(getattr(fec.Codec, meth)), meth


def test_classifier_and_merge_equal_the_definition(fec):
    # (1,2), (2,2), (8,4), (20,10), (3,20), (2,33), (254,2), (31,1): the ratio table names every column
    # once, then 96 seeded blocks per code in twelve corruption patterns, classified chunk by chunk and
    # pass by pass and merged in both chunk orders, against the shard the brute-force definition names
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_locate() == 0


def test_launch_arguments_of_a_cut_batch(fec):
    # k = 5, 70 000-byte shards, one block past kMaxItems / 4375, m in {2, 16, 17, 31, 32, 40, 1, 0}:
    # two slices, each its passes (row 0 and the rows from 1, 16, 31) and then its finalize; the data,
    # parity, verdict and mask bases offset by the slice's first block; the tables of each pass
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_locate_slices() == 0


def _locate(fec, k, m, L, flags, W=None, nblocks=1):
    # no ctx, no buffers: every check below returns before any of them is used
    W = fec.mask_words(max(k + m, 1)) if W is None else W
    return fec.lib.fec_rs_locate_batch(None, k, m, L, nblocks, None, 0, None, 0, 16, None, None, W, None, flags)


def test_argument_errors_before_device_work(fec):
    D = fec.FEC_DEVICE
    INV = fec.FEC_ERR_INVALID_ARG
    # shard counts
    assert _locate(fec, 0, 4, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 4, -1, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 200, 57, 16, D, 8) == fec.FEC_ERR_MAX_SHARD_NUM
    # flags: device memory only
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 7, -1):
        assert _locate(fec, 8, 4, 16, flags) == INV
    # shard_len
    assert _locate(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA
    assert _locate(fec, 8, 4, (1 << 30) + 1, D) == INV
    # mask_words: FEC_MASK_WORDS(k + m) .. 8, although no present_out is given
    assert _locate(fec, 8, 4, 16, D, 0) == INV
    assert _locate(fec, 8, 4, 16, D, 9) == INV
    assert _locate(fec, 30, 10, 16, D, 1) == INV
    # the order: shard counts, then k + m, then flags, then shard_len, then mask_words, then the ctx
    assert _locate(fec, 0, 4, 0, 7, 9) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 4, -1, 0, 7, 9) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 200, 57, 0, 7, 9) == fec.FEC_ERR_MAX_SHARD_NUM
    assert _locate(fec, 8, 4, 0, 7, 9) == INV                           # flags before shard_len
    assert _locate(fec, 8, 4, 0, fec.FEC_HOST, 9) == INV
    assert _locate(fec, 8, 4, 0, D, 9) == fec.FEC_ERR_SHARD_NO_DATA     # shard_len before mask_words
    assert _locate(fec, 8, 4, 0, D, 0) == fec.FEC_ERR_SHARD_NO_DATA
    assert _locate(fec, 8, 4, 16, D, 1) == INV                          # no ctx
    assert _locate(fec, 8, 4, 16, D, 1, nblocks=0) == INV               # the ctx before an empty batch


def test_the_call_takes_every_code_the_encode_takes(fec):
    """A shard_len of 0 is looked at after the shard counts: it shows which codes pass them. (A
    refused mask_words and the missing ctx give the same code, so that the minimum word count is
    accepted is shown where a ctx exists: test_gpu_locate.py.)"""
    D = fec.FEC_DEVICE
    for k, m in [(100, 156), (254, 2), (255, 1), (256, 0), (32, 0), (31, 1), (1, 40), (33, 20)]:
        assert _locate(fec, k, m, 0, D) == fec.FEC_ERR_SHARD_NO_DATA, (k, m)
        assert _locate(fec, k, m, 16, D) == fec.FEC_ERR_INVALID_ARG, (k, m)      # no ctx
    assert _locate(fec, 255, 2, 0, D, 8) == fec.FEC_ERR_MAX_SHARD_NUM
