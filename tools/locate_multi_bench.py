#!/usr/bin/env python3
"""Time fec_rs_locate_multi_batch beside fec_rs_locate_batch on the same buffers: device-resident,
event-timed, one JSON line. The calls of a row are timed alternately in one process (warm-up, then
--reps rounds) and the medians reported: separate processes disagree by several percent.

    python tools/locate_multi_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

1202-byte shards in 1216-byte slots, --gib GiB of data slots per batch, RS(8,12), RS(20,30), RS(64,80),
max_bad = FEC_LOCATE_MAX_BAD, so T = m / 2 = 2, 5, 8. Four batches per code: clean, 1 % of the blocks
with one corrupt shard, 1 % with T corrupt shards, every block with T corrupt shards (one byte of each
corrupt shard, data or parity, at a byte of its own). Per batch a round times the old call (verdicts,
masks and counts), the new call (counts, masks and counts), the old call again, and the new call with
bad_count as its only output: `locate_ms` and `locate_again_ms` are the medians of the two series of
the old call and their ratio `locate_self` is the spread of the yardstick against itself in this
run; `multi_over_locate` and `multi_bare_over_locate` are the new call's medians over the first.
`multi_minus_locate_us` is the difference in microseconds. All calls read k + m shard slots per
block: TBps = (k + m) * round_up(L, 16) * B / time. The tool sets no threshold.

For RS(8,12) the heal loop is timed on the batch with 1 % of the blocks at two corrupt shards: the
new call, then fec_rs_reconstruct_some_batch with the masks it wrote (`heal_ms`, the two calls
together; the batch is corrupted again before every round, outside the timed window), and the healed
batch is compared with the original.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, S = 1202, 1216
R = (L + 15) // 16 * 16


def timed_round_robin(torch, fns, warmup, reps, before=None):
    """Median ms of each function, timed alternately; before(i) runs ahead of fns[i], untimed."""
    def one(i, fn, timed):
        if before:
            before(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) if timed else 0.0
    for _ in range(warmup):
        for i, fn in enumerate(fns):
            one(i, fn, False)
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(one(i, fn, True))
    return [float(np.median(x)) for x in ms]


def code_rows(fec, torch, codec, k, m, gib, warmup, reps, heal):
    rng = np.random.default_rng(100 * k + m)
    n, T = k + m, min(fec.FEC_LOCATE_MAX_BAD, m // 2)
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
    cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")

    # T distinct shards per block, one corrupt byte each, planted by xor (planting twice restores it)
    shard = np.argsort(rng.random((B, n)), axis=1)[:, :T]
    blk = np.arange(B)[:, None]
    pos_np = np.where(shard < k, (blk * k + shard) * S, (blk * m + shard - k) * S) + rng.integers(0, L, (B, T))
    pos = torch.from_numpy(pos_np).cuda()
    val = torch.from_numpy(rng.integers(1, 256, (B, T)).astype(np.uint8)).cuda()
    in_data = torch.from_numpy(shard < k).cuda()
    flat_d, flat_p = data.view(-1), parity.view(-1)
    bits = np.zeros((B, T, 32 * W), dtype=np.uint8)
    np.put_along_axis(bits, shard[:, :, None], 1, axis=2)
    cum = np.cumsum(bits, axis=1)                     # the first t shards of each block as a bit set
    shard_words = torch.from_numpy(np.packbits(cum, axis=2, bitorder="little").view("<u4").reshape(B, T, W)
                                   .astype(np.int64)).cuda()
    full = torch.from_numpy(np.packbits((np.arange(32 * W) < n).astype(np.uint8), bitorder="little").view("<u4")
                            .astype(np.int64)).cuda()

    def plant(blocks, t0, t1):
        """Shards t0 .. t1 - 1 of the blocks' lists."""
        p, v, d = pos[blocks, t0:t1].reshape(-1), val[blocks, t0:t1].reshape(-1), in_data[blocks, t0:t1].reshape(-1)
        flat_d[p[d]] ^= v[d]
        flat_p[p[~d]] ^= v[~d]

    def locate():
        codec.rs_locate_split(k, m, data, parity, old_bad, old_pm, old_cnt, shard_len=L)

    def multi():
        codec.rs_locate_multi_split(k, m, data, parity, bad, present_out=pm, counts=cnt, shard_len=L)

    def multi_bare():   # bad_count alone: no counts to clear
        codec.rs_locate_multi_split(k, m, data, parity, bad, shard_len=L)

    def some():
        codec.rs_reconstruct_some_split(k, m, data, parity, pm.view(-1), shard_len=L)

    order = torch.from_numpy(rng.permutation(B)).cuda()
    one_pct = order[:max(1, B // 100)]
    rest = order[one_pct.numel():]
    rows = []
    base = {"code": "RS(%d,%d)" % (k, n), "T": T, "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3)}
    weight = torch.zeros((B,), dtype=torch.int64, device="cuda")   # corrupt shards of each block now
    steps = [("clean", None, 0, 0), ("one_percent_1", one_pct, 0, 1), ("one_percent_T", one_pct, 1, T),
             ("all_T", rest, 0, T)]
    for name, add, t0, t1 in steps:
        if add is not None and t1 > t0:
            plant(add, t0, t1)
            weight[add] += t1 - t0
        multi()
        locate()
        codec.sync()
        assert torch.equal(bad.long(), weight), "the new call counts the planted shards"
        assert cnt.cpu().tolist() == [int((weight > 0).sum()), 0]
        want_pm = torch.where((weight > 0)[:, None], full[None, :] & ~shard_words[torch.arange(B), (weight - 1).clamp(min=0)],
                              full[None, :].expand(B, W))
        assert torch.equal(pm.long() & 0xFFFFFFFF, want_pm), "and clears their bits"
        single = weight == 1
        assert torch.equal(old_bad[single].long(), torch.from_numpy(shard[:, 0]).cuda()[single]), "the old call names one"
        o_ms, m_ms, o2_ms, b_ms = timed_round_robin(torch, [locate, multi, locate, multi_bare], warmup, reps)
        row = dict(base, batch=name, corrupt_blocks=int((weight > 0).sum()), locate_ms=round(o_ms, 4),
                   multi_ms=round(m_ms, 4), locate_again_ms=round(o2_ms, 4), multi_bare_ms=round(b_ms, 4),
                   multi_over_locate=round(m_ms / o_ms, 4), multi_bare_over_locate=round(b_ms / o_ms, 4),
                   locate_self=round(o2_ms / o_ms, 4), multi_minus_locate_us=round(1e3 * (m_ms - o_ms), 1),
                   locate_TBps=round(n * R * B / (o_ms * 1e-3) / 1e12, 4),
                   multi_TBps=round(n * R * B / (m_ms * 1e-3) / 1e12, 4))
        if heal and name == "one_percent_T":
            def locate_and_heal():
                multi()
                some()
            locate_and_heal()
            codec.sync()
            assert torch.equal(data[:, :, :L], truth_d[:, :, :L]) and torch.equal(parity[:, :, :L], truth_p[:, :, :L]), \
                "the heal loop restores the batch"
            # the batch is whole now: each round plants the errors again first
            h_ms, = timed_round_robin(torch, [locate_and_heal], warmup, reps, before=lambda i: plant(one_pct, 0, T))
            codec.sync()
            assert torch.equal(data[:, :, :L], truth_d[:, :, :L]) and torch.equal(parity[:, :, :L], truth_p[:, :, :L])
            plant(one_pct, 0, T)
            row.update(heal_ms=round(h_ms, 4), heal_over_locate=round(h_ms / o_ms, 4))
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
    out = {"tool": "locate_multi_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "rows": []}
    for k, m, heal in [(8, 4, True), (20, 10, False), (64, 16, False)]:
        out["rows"] += code_rows(fec, torch, codec, k, m, a.gib, a.warmup, a.reps, heal)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
