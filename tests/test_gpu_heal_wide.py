"""Verify -> locate -> heal for codes of more than 32 shards, queued on one stream with no sync between
the calls: the masks that fec_rs_locate_multi_batch and fec_rs_locate_partial_batch write into
present_out go straight into fec_rs_reconstruct_some_wide_batch, which puts back data and parity shards
alike, and fec_rs_verify_batch then finds every block consistent. The batch starts from the oracle's
encode, and must end as it."""
import numpy as np
import pytest

import some_wide_cases as sw
from arena import CANARY, codec, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

B, L, S = 67, 33, 64     # slots of 64 bytes: canary from L on, so a healed slot shows its zero pad


def encoded(oracle, k, m, seed):
    """[B, n, S] from the oracle: bytes [0, L) of every shard, canary from L on."""
    rng = np.random.default_rng(seed)
    sh = np.zeros((B, k + m, L), dtype=np.uint8)
    sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    oracle.rs_encode(k, m, sh)
    out = np.full((B, k + m, S), CANARY, dtype=np.uint8)
    out[:, :, :L] = sh
    return rng, out


def healed(orig, fixed):
    """The batch after healing: the original, and zeros over [L, round_up(L, 16)) of every rebuilt slot."""
    want = orig.copy()
    want[fixed, L:rup16(L)] = 0
    return want


def test_locate_multi_then_heal_then_verify(codec, oracle, torch, fec):
    """RS(64,16): blocks cycle through clean, one corrupt parity shard, one corrupt data shard, one of
    each."""
    k, m = 64, 16
    n, W = k + m, 3
    rng, orig = encoded(oracle, k, m, 64)
    bad = np.zeros((B, n), dtype=bool)
    for b in range(B):
        if b % 4 in (1, 3):
            bad[b, sw.pick(rng, range(k, n), 1, [64] if b < 8 else ())] = True
        if b % 4 in (2, 3):
            bad[b, sw.pick(rng, range(k), 1, [(31, 32, 63)[b // 4 % 3]] if b < 16 else ())] = True
    dmg = orig.copy()
    for b, i in np.argwhere(bad):
        hit = rng.integers(0, L, int(rng.integers(1, L + 1)))
        dmg[b, i, hit] ^= rng.integers(1, 256, len(hit), dtype=np.uint8)
    assert (np.any(dmg != orig, axis=2) == bad).all()
    d = torch.from_numpy(dmg).cuda()
    count = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    masks = torch.full((B, W), 0x7EADBEEF, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), 99, dtype=torch.int32, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    ok = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    nbad = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    # no sync between the three calls
    codec.rs_locate_multi(k, m, d, count, present_out=masks, counts=counts, shard_len=L)
    codec.rs_reconstruct_some_wide(k, m, d, masks, status=st, shard_len=L)
    codec.rs_verify(k, m, d, ok, count=nbad, shard_len=L)
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert np.array_equal(count.cpu().numpy(), bad.sum(axis=1))
    assert np.array_equal(sw.bits(masks.cpu().numpy().view(np.uint32), n), ~bad)
    assert counts.cpu().tolist() == [int(bad.any(axis=1).sum()), 0]
    assert not st.any().item()
    assert (ok == 1).all().item() and nbad.item() == 0
    got = d.cpu().numpy()
    # the arena equals the original encode; the slots of the shards not located are bit-identical to before
    assert np.array_equal(got[:, :, :L], orig[:, :, :L])
    assert np.array_equal(got[~bad], dmg[~bad])
    assert np.array_equal(got, healed(orig, bad))


def test_locate_partial_then_heal_in_one_go(codec, oracle, torch, fec):
    """RS(40,16): every block misses a parity shard, a quarter also a data shard, a quarter have a
    corrupt data shard; the masks are updated in place and the heal rebuilds missing and corrupt shards
    together."""
    k, m = 40, 16
    n, W = k + m, 2
    rng, orig = encoded(oracle, k, m, 40)
    lost = np.zeros((B, n), dtype=bool)
    bad = np.zeros((B, n), dtype=bool)
    for b in range(B):
        lost[b, sw.pick(rng, range(k, n), 1, [k] if b % 8 == 0 else ())] = True
        if b % 4 == 1:
            lost[b, sw.pick(rng, range(k), 1, [31, 32] if b < 8 else ())] = True
        if b % 4 == 2:
            bad[b, sw.pick(rng, range(k), 1, [32, 31] if b < 8 else ())] = True
    assert (lost[:, k:].sum(axis=1) == 1).all() and lost[:, :k].any() and bad.any() and not (lost & bad).any()
    dmg = orig.copy()
    dmg[lost, :rup16(L)] = sw.ERASED
    for b, i in np.argwhere(bad):
        dmg[b, i, int(rng.integers(0, L))] ^= 0x81
    d = torch.from_numpy(dmg).cuda()
    masks = torch.from_numpy(fec.wide_masks(~lost).view(np.int32).copy()).cuda()
    count = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    counts = torch.full((3,), 99, dtype=torch.int32, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    ok = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_locate_partial(k, m, d, masks, count, present_out=masks, counts=counts, shard_len=L)
    codec.rs_reconstruct_some_wide(k, m, d, masks, status=st, shard_len=L)
    codec.rs_verify(k, m, d, ok, shard_len=L)
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert np.array_equal(count.cpu().numpy(), bad.sum(axis=1))
    assert np.array_equal(sw.bits(masks.cpu().numpy().view(np.uint32), n), ~(lost | bad))
    assert counts.cpu().tolist() == [int(bad.any(axis=1).sum()), 0, 0]
    assert not st.any().item() and (ok == 1).all().item()
    got = d.cpu().numpy()
    assert np.array_equal(got[~(lost | bad)], dmg[~(lost | bad)])
    assert np.array_equal(got, healed(orig, lost | bad))
