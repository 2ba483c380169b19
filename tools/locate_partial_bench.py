#!/usr/bin/env python3
"""Time fec_rs_locate_partial_batch beside fec_rs_locate_multi_batch on the same buffers: device-resident,
event-timed, one JSON line. The calls of a row are timed alternately in one process (warm-up, then
--reps rounds) and the medians reported, as tools/locate_multi_bench.py does.

    python tools/locate_partial_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

1202-byte shards in 1216-byte slots, --gib GiB of data slots per batch, RS(8,12), RS(20,30), RS(64,80),
max_bad = FEC_LOCATE_MAX_BAD. Four batches per code:
  full_clean      every mask full, no corrupt shard
  one_missing     one shard (data or parity, drawn per block) missing in every block, no corrupt shard
  one_missing_1pc the same masks, 1 % of the blocks with one corrupt present shard (one byte)
  half_missing_T  every block with e = m / 2 shards missing and T_b = (m - e) / 2 corrupt present shards
A missing shard's slot keeps its bytes: the old call reads it, the new call does not. Per batch a round
times the old call (all outputs), the new call (all outputs), the old call again: `multi_ms` and
`multi_again_ms` are the medians of the old call's two series and `multi_self` their ratio, the spread
of the yardstick against itself in this run; `partial_over_multi` is the new call's median over the
first. The old call reads k + m slots per block, the new one k + m - e. The tool sets no threshold.

For RS(8,12) the heal loop is timed on the one_missing_1pc batch: the new call, then
fec_rs_reconstruct_some_batch with the masks it wrote (`heal_ms`, the two calls together; before every
round, outside the timed window, the missing shards are zeroed and the errors planted again), and the
healed batch is compared with the original.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from locate_multi_bench import L, R, S, timed_round_robin  # noqa: E402


def code_rows(fec, torch, codec, k, m, gib, warmup, reps, heal):
    rng = np.random.default_rng(100 * k + m + 1)
    n = k + m
    W = fec.mask_words(n)
    B = max(2, int(gib * (1 << 30)) // (k * S))
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    truth_d, truth_p = data.clone(), parity.clone()
    old_bad = torch.zeros((B,), dtype=torch.int32, device="cuda")
    old_pm = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    old_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    bad = torch.zeros((B,), dtype=torch.int32, device="cuda")
    pm = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((3,), dtype=torch.int32, device="cuda")
    flat_d, flat_p = data.view(-1), parity.view(-1)
    perm = np.argsort(rng.random((B, n)), axis=1)        # per block: the missing shards first, then the corrupt
    blk = np.arange(B)[:, None]
    order = rng.permutation(B)
    one_pct = order[:max(1, B // 100)]
    e_half = m // 2
    T_half = min(fec.FEC_LOCATE_MAX_BAD, (m - e_half) // 2)

    def masks_of(e):
        bits = np.zeros((B, 32 * W), dtype=np.uint8)
        bits[:, :n] = 1
        np.put_along_axis(bits, perm[:, :e], 0, axis=1)
        return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(B, W)
                                .view(np.int32)).cuda()

    def planter(blocks, e, t):
        """xor one byte into shards perm[:, e:e + t] of the blocks (planting twice restores them)."""
        shard = perm[blocks, e:e + t]
        b = np.asarray(blocks)[:, None]
        pos = np.where(shard < k, (b * k + shard) * S, (b * m + shard - k) * S) + rng.integers(0, L, shard.shape)
        val = torch.from_numpy(rng.integers(1, 256, shard.shape).astype(np.uint8).reshape(-1)).cuda()
        d = torch.from_numpy((shard < k).reshape(-1)).cuda()
        p = torch.from_numpy(pos.reshape(-1)).cuda()

        def plant():
            flat_d[p[d]] ^= val[d]
            flat_p[p[~d]] ^= val[~d]
        return plant

    state = {}

    def multi():
        codec.rs_locate_multi_split(k, m, data, parity, old_bad, present_out=old_pm, counts=old_cnt, shard_len=L)

    def partial():
        codec.rs_locate_partial_split(k, m, data, parity, state["masks"], bad, present_out=pm, counts=cnt, shard_len=L)

    def some():
        codec.rs_reconstruct_some_split(k, m, data, parity, pm.view(-1), shard_len=L)

    rows = []
    base = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3)}
    plant_1pc = planter(one_pct, 1, 1)
    plant_all = planter(np.arange(B), e_half, T_half)
    steps = [("full_clean", 0, None, 0, 0), ("one_missing", 1, None, 0, 0), ("one_missing_1pc", 1, plant_1pc, one_pct.size, 1),
             ("half_missing_T", e_half, plant_all, B, T_half)]
    for name, e, plant, nbad, t in steps:
        state["masks"] = masks_of(e)
        if plant:
            plant()
        partial()
        codec.sync()
        want = np.zeros(B, dtype=np.int64)
        if plant:
            want[one_pct if nbad < B else np.arange(B)] = t
        assert np.array_equal(bad.cpu().numpy(), want), "the new call counts the planted shards"
        assert cnt.cpu().tolist() == [int((want > 0).sum()), 0, 0]
        if e == 0:
            multi()
            codec.sync()
            assert torch.equal(old_bad, bad) and torch.equal(old_pm, pm)
        o_ms, p_ms, o2_ms = timed_round_robin(torch, [multi, partial, multi], warmup, reps)
        row = dict(base, batch=name, missing=e, T_b=min(fec.FEC_LOCATE_MAX_BAD, (m - e) // 2),
                   corrupt_blocks=int((want > 0).sum()), corrupt_shards=t, multi_ms=round(o_ms, 4),
                   partial_ms=round(p_ms, 4), multi_again_ms=round(o2_ms, 4), partial_over_multi=round(p_ms / o_ms, 4),
                   multi_self=round(o2_ms / o_ms, 4), partial_minus_multi_us=round(1e3 * (p_ms - o_ms), 1),
                   multi_TBps=round(n * R * B / (o_ms * 1e-3) / 1e12, 4),
                   partial_TBps=round((n - e) * R * B / (p_ms * 1e-3) / 1e12, 4))
        if heal and name == "one_missing_1pc":
            miss = perm[:, 0]
            md = torch.from_numpy(np.flatnonzero(miss < k)).cuda(), torch.from_numpy(miss[miss < k]).cuda()
            mp = torch.from_numpy(np.flatnonzero(miss >= k)).cuda(), torch.from_numpy(miss[miss >= k] - k).cuda()

            def spoil(_):
                data[md[0], md[1]] = 0
                parity[mp[0], mp[1]] = 0
                plant()

            def locate_and_heal():
                partial()
                some()
            data[md[0], md[1]] = 0            # (the errors are planted already)
            parity[mp[0], mp[1]] = 0
            locate_and_heal()
            codec.sync()
            assert torch.equal(data[:, :, :L], truth_d[:, :, :L]) and torch.equal(parity[:, :, :L], truth_p[:, :, :L]), \
                "the heal loop restores the batch"
            h_ms, = timed_round_robin(torch, [locate_and_heal], warmup, reps, before=spoil)
            codec.sync()
            assert torch.equal(data[:, :, :L], truth_d[:, :, :L]) and torch.equal(parity[:, :, :L], truth_p[:, :, :L])
            row.update(heal_ms=round(h_ms, 4), heal_over_multi=round(h_ms / o_ms, 4))
        elif plant:
            plant()                           # restore the batch for the next step
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    fec = importlib.import_module("0xfec_amd")
    codec = fec.Codec(0).use_torch_stream()
    out = {"tool": "locate_partial_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "rows": []}
    for k, m, heal in [(8, 4, True), (20, 10, False), (64, 16, False)]:
        out["rows"] += code_rows(fec, torch, codec, k, m, a.gib, a.warmup, a.reps, heal)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
