"""fec_rs_reconstruct_some_wide_batch on batches whose byte offsets do not fit 32 bits: the four layout
families of far_cases.py in the sparse arena of far_arena.py, RS(33,32) with mixed data and parity loss
(some_wide_cases.far_lost). As in test_gpu_far_offsets.py the windows of the case are compared with a
model byte for byte and the rest of the arena must be canary, so a store through a truncated offset is
found wherever it lands; test_some_wide_cases.py checks on the CPU that the layouts obey the arena's
rule. A shard stride of 2^32 is refused."""
import numpy as np
import pytest

import far_cases as fc
import some_wide_cases as sw
from arena import codec, rup16, torch  # noqa: F401
from far_arena import far  # noqa: F401

pytestmark = pytest.mark.gpu

B = fc.B
K, M = sw.FAR_CODE
NW = 3    # FEC_MASK_WORDS(65)
W = 4     # one word more than the code needs


def words(t, a):
    return t.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def layout_args(far, lay, L):
    d, p = lay.regions["data"], lay.regions["parity"]
    assert d.ss == p.ss
    return L, B, far.addr(d), d.bs, far.addr(p), p.bs, d.ss


@pytest.mark.parametrize("L", sw.FAR_LENS)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_reconstruct_some_wide(far, codec, oracle, torch, fec, family, L):
    """Every missing shard wanted, data and parity; then a want mask of the parity shards alone."""
    k, m, n = K, M, K + M
    lost = sw.far_lost(k, m)
    cs = sw.make_case(oracle, k, m, L, lost, 99)
    lay = fc.far_layout(family, k, m, L)
    assert lay.size <= far.size
    few_all = lost.any(axis=1) & ~cs["ok"]
    assert few_all.tolist() == [False, True, False, False, False]
    masks = np.zeros((B, W), dtype=np.uint32)
    masks[:, :NW] = fec.wide_masks(~lost)
    par_only = np.zeros((B, n), dtype=bool)
    par_only[:, k:] = True
    for want in (None, par_only):
        rset = lost if want is None else lost & want
        few = rset.any(axis=1) & ~cs["ok"]
        pre = far.blank(lay)
        R = rup16(L)
        pre["data"][:, :, :L] = cs["dmg"][:, :k]
        pre["parity"][:, :, :L] = cs["dmg"][:, k:]
        pre["data"][lost[:, :k], :R] = sw.ERASED
        pre["parity"][lost[:, k:], :R] = sw.ERASED
        model = {name: w.copy() for name, w in pre.items()}
        for b in np.flatnonzero(~few):
            for i in np.flatnonzero(rset[b]):
                name, j = ("data", i) if i < k else ("parity", i - k)
                model[name][b, j, :L] = cs["full"][b, i]
                model[name][b, j, L:R] = 0
        far.write(lay, pre)
        dm = words(torch, masks)
        dw = None
        if want is not None:
            w3 = np.zeros((B, W), dtype=np.uint32)
            w3[:, :NW] = fec.wide_masks(want)
            dw = words(torch, sw.stray(w3, n))
        st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
        assert fec.lib.fec_rs_reconstruct_some_wide_batch(codec.handle, k, m, *layout_args(far, lay, L), dm.data_ptr(),
                                                          None if dw is None else dw.data_ptr(), W, st.data_ptr(),
                                                          fec.FEC_DEVICE) == fec.FEC_OK
        st_want = np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS, 0)
        assert codec.lib_sync_rc() == (fec.FEC_ERR_TOO_FEW_SHARDS if few.any() else fec.FEC_OK)
        assert codec.lib_sync_rc() == fec.FEC_OK
        assert np.array_equal(st.cpu().numpy(), st_want)
        far.check(lay, model, "%s-%d-%s" % (family, L, "all" if want is None else "parity"))


def test_a_shard_stride_of_4gib_is_refused(far, codec, torch, fec):
    """2^32 and 2^32 + 16 are refused before anything is enqueued: the return code, a clean sync, every
    status stale, the arena all canary."""
    k, m, L = K, M, 1202
    full = np.ones((B, k + m), dtype=bool)
    full[:, 0] = False                                    # data shard 0 of every block to rebuild
    dm = words(torch, fec.wide_masks(full))
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    d, p = far.ptr + fc.LEAD, far.ptr + fc.LEAD + 4096
    for ss in (fc.REFUSED_STRIDE, fc.REFUSED_STRIDE + 16):
        assert fec.lib.fec_rs_reconstruct_some_wide_batch(codec.handle, k, m, L, B, d, 1232, p, 1232, ss, dm.data_ptr(),
                                                          None, NW, st.data_ptr(),
                                                          fec.FEC_DEVICE) == fec.FEC_ERR_INVALID_ARG
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert (st.cpu().numpy() == 99).all()
    assert far.first_dirty() is None
