"""The decode convention of fec_status.hpp through every kernel that classifies blocks: one mixed
batch per kernel, statuses against the rule computed here from the masks, and the sticky word's
return codes in their order (too few shards first, then too few slots, then clear).

Every batch has 130 blocks (two full 64-block windows or waves and a partial one); block b's mask
is chosen by b % 4: all present, one data shard lost, fewer than k shards present, more data
shards lost than the call has output slots. An in-place call has no slot limit and so three
classes: its b % 4 == 3 blocks lose one data shard again (another one). The rule, for e erased
data shards and p present shards of a block: e == 0 -> 0; p < k -> FEC_ERR_TOO_FEW_SHARDS (this
wins over the slot limit); slots and e > slots -> FEC_ERR_INVALID_ARG; else e from a recover, 0 in
place.

Which kernel a call reaches (fec_cores.cpp rs_reconstruct_device): shards under 32 chunks take
rs_plan_kernel; longer ones the sorted plans, rs_plan_code_kernel for RS(16,24); a one-slot recover
the direct kernel, RS(2,3) its own; more than 32 shards the wide plan kernel. RS(8,12) in place
takes the routed kernel: no block of its batch has two erased data shards, so the classify pass
leaves the route word zero, the sorted plan kernel exits at once, and the routed kernel runs its
direct route, whose status pass writes every status compared here. (The plan route of the same
kernel, where rs_plan_sorted_kernel writes them: test_gpu_dispatch_edges.py
test_rs_inplace_routed_k8_codes_match_oracle with multi = True.)
The shard bytes are arbitrary: only statuses and return codes are checked here (the rebuilt bytes
of these kernels: test_gpu_dispatch_edges.py, test_gpu_codec.py, test_gpu_wide.py). The ragged
calls' oversize bit: test_gpu_ragged.py test_oversize_blocks_are_skipped_and_reported.
"""
import numpy as np
import pytest

from arena import codec, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

B = 130

# (kernel, k, m, L, slots): slots 0 is an in-place call
CASES = [("rs_plan_kernel", 4, 2, 17, 1),
         ("rs_plan_sorted_kernel", 4, 3, 512, 2),
         ("rs_plan_code_kernel", 16, 8, 512, 2),
         ("rs_recover_direct_kernel", 8, 4, 512, 1),
         ("rs_recover_k2m1_kernel", 2, 1, 512, 1),
         ("rs_reconstruct_routed_kernel", 8, 4, 512, 0),
         ("rs_plan_wide_kernel", 40, 8, 17, 2),
         ("xor_reconstruct_kernel", 4, 1, 17, 0)]


def class_masks(k, m, slots):
    """[B] Python ints: the four classes by b % 4 (lost shards vary with b inside a class)."""
    n, full = k + m, (1 << (k + m)) - 1
    masks = []
    for b in range(B):
        c = b % 4
        if c == 0:
            lost = []
        elif c == 1:
            lost = [b % k]
        elif c == 2:
            lost = [(b + i) % n for i in range(m + 1)] if b % 8 == 2 else list(range(m + 1))   # data among them
        elif slots:
            lost = [(b + i) % k for i in range(min(k, slots + 1))]
        else:
            lost = [(b + 1) % k]                          # in place: no fourth class
        masks.append(full & ~sum(1 << i for i in lost))
    return masks


def rule(fec, masks, k, m, slots):
    st = []
    for mask in masks:
        e = k - bin(mask & ((1 << k) - 1)).count("1")
        p = bin(mask).count("1")
        st.append(0 if e == 0 else fec.FEC_ERR_TOO_FEW_SHARDS if p < k else
                  fec.FEC_ERR_INVALID_ARG if slots and e > slots else e if slots else 0)
    return np.array(st, dtype=np.int32)


def run(codec, torch, kernel, k, m, L, slots, masks, data, parity):
    """One call over the batch; returns its statuses."""
    n, S = k + m, rup16(L)
    words = (n + 31) // 32
    mw = np.array([[(mask >> (32 * w)) & 0xFFFFFFFF for w in range(words)] for mask in masks], dtype=np.uint32)
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    out = torch.zeros((B, max(slots, 1), S), dtype=torch.uint8, device="cuda")
    if kernel == "xor_reconstruct_kernel":
        sh = torch.cat([data, parity], dim=1).contiguous()
        codec.xor_reconstruct(k, sh, torch.from_numpy(mw[:, 0].view(np.int32).copy()).cuda(), status=st, shard_len=L)
    elif kernel == "rs_plan_wide_kernel":
        codec.rs_recover_wide_split(k, m, data, parity, torch.from_numpy(mw.view(np.int32)).cuda(), out, status=st,
                                    shard_len=L)
    elif slots:
        codec.rs_recover_split(k, m, data, parity, torch.from_numpy(mw[:, 0].view(np.int32).copy()).cuda(), out,
                               status=st, shard_len=L)
    else:
        codec.rs_reconstruct_split(k, m, data, parity, torch.from_numpy(mw[:, 0].view(np.int32).copy()).cuda(),
                                   status=st, shard_len=L)
    return st


@pytest.mark.parametrize("kernel,k,m,L,slots", CASES, ids=[c[0] for c in CASES])
def test_mixed_batch_statuses_and_sticky_codes(codec, torch, fec, kernel, k, m, L, slots):
    rng = np.random.default_rng(100 * k + m)
    S = rup16(L)
    data = torch.from_numpy(rng.integers(0, 256, (B, k, S), dtype=np.uint8)).cuda()
    parity = torch.from_numpy(rng.integers(0, 256, (B, m, S), dtype=np.uint8)).cuda()
    assert codec.lib_sync_rc() == fec.FEC_OK          # nothing pending from an earlier test

    masks = class_masks(k, m, slots)
    want = rule(fec, masks, k, m, slots)
    assert (want == 0).any() and (want == fec.FEC_ERR_TOO_FEW_SHARDS).any()
    if slots:
        assert (want == 1).any()
    else:   # one erased data shard at the most where k shards are present (RS(8,12): the route word stays zero)
        e_d = np.array([k - bin(mask & ((1 << k) - 1)).count("1") for mask in masks])
        assert e_d[want == 0].max() == 1
    st = run(codec, torch, kernel, k, m, L, slots, masks, data, parity)
    assert codec.lib_sync_rc() == fec.FEC_ERR_TOO_FEW_SHARDS
    assert np.array_equal(st.cpu().numpy(), want)

    # the too-few blocks made whole: too few slots is what is left, where the call has slots and
    # the code can lose more data shards than that and still have k shards
    full = (1 << (k + m)) - 1
    healed = [full if w == fec.FEC_ERR_TOO_FEW_SHARDS else mask for mask, w in zip(masks, want)]
    want2 = rule(fec, healed, k, m, slots)
    slots_apply = bool(slots) and min(k, m) > slots
    assert (want2 == fec.FEC_ERR_INVALID_ARG).any() == slots_apply and not (want2 == fec.FEC_ERR_TOO_FEW_SHARDS).any()
    st = run(codec, torch, kernel, k, m, L, slots, healed, data, parity)
    assert codec.lib_sync_rc() == (fec.FEC_ERR_INVALID_ARG if slots_apply else fec.FEC_OK)
    assert codec.lib_sync_rc() == fec.FEC_OK          # reported once, then cleared
    assert np.array_equal(st.cpu().numpy(), want2)
