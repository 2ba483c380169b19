"""Ragged verify and ragged reconstruct-some past 4 GiB: one layout per call in which both the block
stride and the distance from the data to the parity region exceed 32 bits (ragged_more_cases.far_layout),
on the sparse arena of far_arena.py. The layout cannot fault: a 32-bit mistake in either product reads
or writes canary inside the arena (test_ragged_more_cases.py checks that without a device), and every
byte of the arena outside the modelled windows is checked for the canary after the call. Five blocks
of lengths 1202, 1, 17, 600 and 1202, each with contents of its own, against the oracle at each
block's own length."""
import numpy as np
import pytest

import far_cases as fc
import ragged_more_cases as rc
from arena import STALE, codec, rup16, torch  # noqa: F401
from far_arena import far  # noqa: F401

pytestmark = pytest.mark.gpu

K, M, L = 8, 4, rc.MAXL
NB = fc.B


def words(t, a):
    return t.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def stale(t, n):
    return t.full((n,), STALE, dtype=t.int32, device="cuda")


def far_args(far, lay):
    d, p = lay.regions["data"], lay.regions["parity"]
    return L, NB, far.addr(d), d.bs, far.addr(p), p.bs, d.ss


def encoded_blocks(oracle):
    """[NB, n, L]: each block's own data below its length, zero from it on, and the oracle's parity."""
    lens = np.array(rc.FAR_LENS)
    data = np.random.default_rng(4099).integers(0, 256, (NB, K, L), dtype=np.uint8)
    sh = rc.encoded(rc.oracle_encode(oracle), K, M, data, lens)
    assert len({sh[b, :, :1].tobytes() for b in range(NB)}) == NB   # an aliased read returns other bytes
    return lens, sh


def test_far_ragged_verify(far, codec, oracle, torch, fec):
    """Blocks 2 and 4 have a byte flipped in the last chunk of the farthest data and the farthest
    parity shard; the slots hold garbage from each block's length on."""
    lay = rc.far_layout(K, M)
    lens, sh = encoded_blocks(oracle)
    rng = np.random.default_rng(5)
    pre = far.blank(lay)
    for b in range(NB):
        Lb = int(lens[b])
        pre["data"][b, :, :Lb], pre["parity"][b, :, :Lb] = sh[b, :K, :Lb], sh[b, K:, :Lb]
        pre["data"][b, :, Lb:] = rng.integers(0, 256, pre["data"][b, :, Lb:].shape, dtype=np.uint8)
        pre["parity"][b, :, Lb:] = rng.integers(0, 256, pre["parity"][b, :, Lb:].shape, dtype=np.uint8)
    pre["data"][2, K - 1, lens[2] - 1] ^= 0x40
    pre["parity"][4, M - 1, lens[4] - 1] ^= 0x01
    far.write(lay, pre)
    dl, st, cnt = words(torch, lens), stale(torch, NB), stale(torch, 1)
    assert codec.rs_verify_ragged_raw(K, M, *far_args(far, lay), dl.data_ptr(), st.data_ptr(),
                                      cnt.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert st.cpu().numpy().tolist() == [1, 1, 0, 1, 0] and cnt.cpu().numpy().tolist() == [2]
    far.check(lay, pre, "far ragged verify")


def test_far_ragged_reconstruct_some(far, codec, oracle, torch, fec):
    """Every missing shard wanted: block 0 a data and a parity shard, block 1 too few, block 2 a data
    shard and parity shard 0, block 3 parity only, block 4 its farthest data and parity shards."""
    lay = rc.far_layout(K, M)
    lens, sh = encoded_blocks(oracle)
    lost = rc.far_some_lost(K, M)
    few = (~lost).sum(axis=1) < K
    assert few.tolist() == [False, True, False, False, False]
    pre = far.blank(lay)
    for b in range(NB):
        Lb = int(lens[b])
        pre["data"][b, :, :Lb], pre["parity"][b, :, :Lb] = sh[b, :K, :Lb], sh[b, K:, :Lb]
        pre["data"][b, lost[b, :K], :rup16(Lb)] = rc.ERASED
        pre["parity"][b, lost[b, K:], :rup16(Lb)] = rc.ERASED
    model = {name: w.copy() for name, w in pre.items()}
    for b in np.flatnonzero(~few):
        Lb = int(lens[b])
        for i in np.flatnonzero(lost[b]):
            win, j = (model["data"], i) if i < K else (model["parity"], i - K)
            win[b, j, :Lb] = sh[b, i, :Lb]
            win[b, j, Lb:rup16(Lb)] = 0
    far.write(lay, pre)
    dl, dm, st = words(torch, lens), words(torch, rc.pack(~lost)), stale(torch, NB)
    assert codec.rs_reconstruct_some_ragged_raw(K, M, *far_args(far, lay), dm.data_ptr(), dl.data_ptr(), None,
                                                st.data_ptr()) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_ERR_TOO_FEW_SHARDS and codec.lib_sync_rc() == fec.FEC_OK
    assert st.cpu().numpy().tolist() == [0, rc.TOO_FEW, 0, 0, 0]
    far.check(lay, model, "far ragged reconstruct-some")


def test_reconstruct_some_ragged_refuses_a_shard_stride_of_4gib(far, codec, torch, fec):
    dm, dl, st = words(torch, [0xFFE] * NB), words(torch, [L] * NB), stale(torch, NB)
    d, p = far.ptr + fc.LEAD, far.ptr + fc.LEAD + 4096
    for ss in (fc.REFUSED_STRIDE, fc.REFUSED_STRIDE + 16):
        assert codec.rs_reconstruct_some_ragged_raw(K, M, L, NB, d, 1232, p, 1232, ss, dm.data_ptr(), dl.data_ptr(),
                                                    None, st.data_ptr()) == fec.FEC_ERR_INVALID_ARG
    assert codec.lib_sync_rc() == fec.FEC_OK and (st.cpu().numpy() == STALE).all()
    assert far.first_dirty() is None
