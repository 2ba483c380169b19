"""fec_rs_locate_multi_batch (up to m/2 corrupt shards of a block that fails verify), the parts that
need no GPU: the entry point and FEC_LOCATE_MAX_BAD are declared, exported and have a row in the
header's table, the Codec methods exist, the arithmetic the solve kernel shares with the host
(fec__selftest_locate_multi: the coefficient table, the per-chunk solver, the merge) equals the
brute-force definition and the two guarantees, the argument fill of a batch that the limits cut
(fec__selftest_locate_multi_slices) gives every slice the bases, workspace and tables that the call's
strides imply, and the argument checks that return before any device work come in the documented
order."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fec_rs_locate_multi_batch"


def test_header_declares_and_library_exports_the_call(fec):
    src = open(os.path.join(ROOT, "include", "fec_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    d = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, code)
    assert d, "%s is not declared" % NAME
    p = d.group(1)
    assert re.search(r"const\s+uint8_t\s*\*\s*data\b", p) and re.search(r"const\s+uint8_t\s*\*\s*parity\b", p)
    assert re.search(r"\bint\s+max_bad\b", p)
    assert re.search(r"(?<!const )int32_t\s*\*\s*bad_count\b", p)
    assert re.search(r"(?<!const )uint32_t\s*\*\s*present_out\b", p)
    assert re.search(r"size_t\s+mask_words\b", p)
    assert re.search(r"(?<!const )uint32_t\s*\*\s*counts\b", p)
    # max_bad stands between shard_stride and bad_count
    names = [re.search(r"(\w+)\s*$", a).group(1) for a in p.split(",")]
    assert names == ["ctx", "k", "m", "shard_len", "nblocks", "data", "data_block_stride", "parity",
                     "parity_block_stride", "shard_stride", "max_bad", "bad_count", "present_out", "mask_words",
                     "counts", "flags"]
    assert re.search(r"^#define\s+FEC_LOCATE_MAX_BAD\s+8\b", code, flags=re.M)
    assert re.search(r"^ \*\s+%s\b" % NAME, src, flags=re.M), "%s has no row in the header's table" % NAME
    assert hasattr(ctypes.CDLL(fec._LIB_PATH), NAME)
    assert fec.FEC_LOCATE_MAX_BAD == 8
    for meth in ["rs_locate_multi_raw", "rs_locate_multi", "rs_locate_multi_split"]:
        assert callable(getattr(fec.Codec, meth)), meth
    # the single-shard call's contract points to the new one
    old = re.search(r"/\* Locate the corrupt shard of a block.*?\*/", src, flags=re.S).group(0)
    assert NAME in old


def test_solver_and_merge_equal_the_definition(fec):
    # (1,2), (2,2), (6,3), (3,5), (8,4), (1,8), (16,8), (20,10), (4,16), (240,16), (31,1), (32,0), max_bad
    # 1 .. 8, 42 seeded blocks each in fourteen error patterns: every subset of at most T shards tried
    # where they can be counted, the two guarantees everywhere, max_bad = 1 against locate_chunk /
    # locate_merge. (Subsets are counted for n <= 12, and (16,8) at max_bad <= 2; codes of n > 12 are
    # checked against the definition, past the radius too, by test_locate_hard_cases.py's port of the
    # column solver and by test_gpu_locate_hard.py on the device.)
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_locate_multi() == 0


def test_launch_arguments_of_a_cut_batch(fec):
    # 70 000-byte shards and one block more than kPlanBytes of workspace holds: two slices, each its
    # clear size, scan, solve and finalize arguments; 16-byte shards: three slices by the workspace alone
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_locate_multi_slices() == 0


def _locate(fec, k, m, L, flags, W=None, max_bad=1, nblocks=1):
    # no ctx, no buffers: every check below returns before any of them is used
    W = fec.mask_words(max(k + m, 1)) if W is None else W
    return fec.lib.fec_rs_locate_multi_batch(None, k, m, L, nblocks, None, 0, None, 0, 16, max_bad, None, None, W,
                                             None, flags)


def test_argument_errors_before_device_work(fec):
    D = fec.FEC_DEVICE
    INV = fec.FEC_ERR_INVALID_ARG
    # shard counts
    assert _locate(fec, 0, 4, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 4, -1, 16, D) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 250, 7, 16, D, 8) == fec.FEC_ERR_MAX_SHARD_NUM
    # m > 16: not yet supported
    assert _locate(fec, 8, 17, 16, D) == INV
    assert _locate(fec, 8, 17, 0, D) == INV                             # before shard_len
    assert _locate(fec, 1, 40, 0, D, 2) == INV
    assert _locate(fec, 200, 57, 0, D, 8) == fec.FEC_ERR_MAX_SHARD_NUM  # after k + m
    assert _locate(fec, 8, 16, 0, D) == fec.FEC_ERR_SHARD_NO_DATA       # m = 16 passes
    # flags: device memory only
    for flags in (fec.FEC_HOST, fec.FEC_HOST_PINNED, 7, -1):
        assert _locate(fec, 8, 4, 16, flags) == INV
    # shard_len
    assert _locate(fec, 8, 4, 0, D) == fec.FEC_ERR_SHARD_NO_DATA
    assert _locate(fec, 8, 4, (1 << 30) + 1, D) == INV
    # max_bad in [1, FEC_LOCATE_MAX_BAD]
    for mb in (0, 9, -1, 1 << 20):
        assert _locate(fec, 8, 4, 16, D, max_bad=mb) == INV
        assert _locate(fec, 8, 4, 0, D, max_bad=mb) == fec.FEC_ERR_SHARD_NO_DATA    # shard_len before max_bad
    # mask_words: FEC_MASK_WORDS(k + m) .. 8, although no present_out is given
    assert _locate(fec, 8, 4, 16, D, 0) == INV
    assert _locate(fec, 8, 4, 16, D, 9) == INV
    assert _locate(fec, 30, 10, 16, D, 1) == INV
    # the order: shard counts, k + m, m > 16, flags, shard_len, max_bad, mask_words, then the ctx
    assert _locate(fec, 0, 17, 0, 7, 9, max_bad=0) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 4, -1, 0, 7, 9, max_bad=0) == fec.FEC_ERR_INV_SHARD_NUM
    assert _locate(fec, 240, 17, 0, 7, 9, max_bad=0) == fec.FEC_ERR_MAX_SHARD_NUM
    assert _locate(fec, 8, 17, 0, 7, 9, max_bad=0) == INV
    assert _locate(fec, 8, 4, 0, 7, 9, max_bad=0) == INV                # flags before shard_len
    assert _locate(fec, 8, 4, 0, D, 9, max_bad=0) == fec.FEC_ERR_SHARD_NO_DATA
    assert _locate(fec, 8, 4, 16, D, 1) == INV                          # no ctx
    assert _locate(fec, 8, 4, 16, D, 1, max_bad=8) == INV
    assert _locate(fec, 8, 4, 16, D, 1, nblocks=0) == INV               # the ctx before an empty batch


def test_the_call_takes_every_code_of_at_most_16_parity_rows(fec):
    """A shard_len of 0 is looked at after the shard counts and the limit on m: it shows which codes
    pass them."""
    D = fec.FEC_DEVICE
    for k, m in [(240, 16), (254, 2), (255, 1), (256, 0), (32, 0), (31, 1), (1, 16), (4, 16), (20, 10)]:
        for mb in (1, 8):
            assert _locate(fec, k, m, 0, D, max_bad=mb) == fec.FEC_ERR_SHARD_NO_DATA, (k, m)
            assert _locate(fec, k, m, 16, D, max_bad=mb) == fec.FEC_ERR_INVALID_ARG, (k, m)      # no ctx
    for k, m in [(1, 17), (33, 20), (100, 156)]:
        assert _locate(fec, k, m, 0, D, 8) == fec.FEC_ERR_INVALID_ARG, (k, m)
