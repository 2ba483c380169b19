"""Every parity-row count through the calls that share the generic fold body, against the CPU oracle.

Verify, update / encode-idx, locate, the locate-multi and locate-partial scans, the generic encode and
the ragged encode are each compiled once per row count (1, 2, 4, 8, 16; the ragged encode 12 as well),
chosen by the rows of a pass, with codes of more than 16 rows cut into passes. The enumerated tests of
these calls reach the instances through short code lists; this module sweeps them: m = 1 .. 33, k = 1 ..
17 under a predicated row, and the codes at the edge of the LDS table limit (row_sweep_cases.py, which
test_row_sweep_cases.py checks on the CPU against the launchers' own instance lists).

Every batch that starts from an encoded image takes its parity from oracle.rs_encode, so "a clean batch
verifies clean" compares the device with the oracle, not with the device's own encode. The batches,
corruption patterns, models and whole-arena checks are the sibling modules' (test_gpu_verify.py,
test_gpu_update.py, test_gpu_locate.py, test_gpu_locate_multi.py, test_gpu_locate_partial.py,
test_gpu_ragged.py), at their smallest shape: 67 blocks of 33 bytes. No code's batch is cut below that.
"""
import numpy as np
import pytest

import row_sweep_cases as rs
import test_gpu_ragged as rag
import test_gpu_update as up
import test_gpu_verify as vr
from arena import check_arena, codec, gf, torch  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,m", rs.FLAT_CODES)
def test_encode_gives_the_oracles_parity(codec, torch, fec, oracle, k, m):
    before, after, data, par = rs.encode_case(oracle, k, m)
    dev = torch.from_numpy(before).cuda()
    p = dev.data_ptr()
    assert p % 16 == 0
    assert fec.lib.fec_rs_encode_batch(codec.handle, k, m, rs.L, rs.B, p + data.off, data.bs, p + par.off, par.bs,
                                       data.ss, fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(dev.cpu().numpy(), after, "encode")


@pytest.mark.parametrize("k,m", rs.FLAT_CODES)
def test_verify(codec, torch, fec, oracle, k, m):
    """The oracle's parity is clean; a bit of the last byte of the last parity row, of byte 0 of data shard
    k - 1, and the many-bad-blocks pattern among the sibling's cases."""
    bt = rs.verify_batch(codec, fec, torch, oracle, k, m)
    assert bt.B >= 67      # run_cases: the many-bad-blocks pattern
    vr.run_cases(bt)


@pytest.mark.parametrize("k,m", rs.FLAT_CODES)
def test_update_and_encode_idx(codec, torch, fec, oracle, k, m):
    up.run_cases(rs.update_batch(codec, fec, torch, oracle, k, m))
    # every column onto zeroed parity: the oracle's parity (the model folds the oracle's encode into zeros)
    bt = rs.update_batch(codec, fec, torch, oracle, k, m, zero_parity=True)
    bt.check("encode_idx", np.ones((bt.B, k), dtype=bool), fec.mask_words(k), what="every column onto zeroed parity")


@pytest.mark.parametrize("k,m", rs.LOCATE_CODES)
def test_locate(codec, torch, fec, oracle, gf, k, m):
    rs.locate_batch(codec, fec, torch, oracle, gf, k, m).run()


@pytest.mark.parametrize("k,m", rs.MULTI_CODES)
def test_locate_multi(codec, torch, fec, oracle, gf, k, m):
    rs.multi_batch(codec, fec, torch, oracle, gf, k, m).run()


@pytest.mark.parametrize("k,m,max_bad", rs.MULTI_BELOW)
def test_locate_multi_below_the_radius(codec, torch, fec, oracle, gf, k, m, max_bad):
    b = rs.multi_batch(codec, fec, torch, oracle, gf, k, m, max_bad)
    assert b.T == max_bad == m // 2 - 1
    b.run()


@pytest.mark.parametrize("k,m", rs.MULTI_CODES)
def test_locate_partial(codec, torch, fec, oracle, gf, k, m):
    rs.partial_batch(codec, fec, torch, oracle, gf, k, m).run()


@pytest.mark.parametrize("layout", ["interleaved", "split"])
@pytest.mark.parametrize("k,m", rs.RAGGED_CODES)
def test_ragged_encode(codec, torch, fec, oracle, k, m, layout):
    rag.run_encode(codec, fec, torch, rs.ragged_case(oracle, k, m), k, m, layout)
