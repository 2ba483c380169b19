#!/usr/bin/env python3
"""Time fec_rs_locate_batch beside fec_rs_verify_batch on the same buffers: device-resident,
event-timed, one JSON line. The calls of a row are timed alternately in one process (warm-up, then
--reps rounds) and the medians reported: separate processes disagree by several percent.

    python tools/locate_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

1202-byte shards in 1216-byte slots, --gib GiB of data slots per batch, RS(8,12), RS(20,30), RS(64,80).
Three batches per code: clean, 1 % of the blocks with one corrupt shard (one byte of a data or parity
shard), every block with one. Per batch a round times verify, locate (with present_out and counts),
verify again, and locate with the verdicts as its only output (no finalize kernel): `verify_ms` and
`verify_again_ms` are the medians of the two verify series, and their ratio `verify_self` is the
spread of the yardstick against itself in this run; `locate_over_verify` and
`locate_bare_over_verify` are the two locates' medians over the first. All of them read k + m shard
slots per block: TBps = (k + m) * round_up(L, 16) * B / time. The tool sets no threshold.

For RS(8,12) the heal loop is timed too, on the 1 % and the all-corrupt batch: locate, then
fec_rs_reconstruct_some_batch with the masks locate wrote (`heal_ms`, the two calls together; the
batch is corrupted again before every round, outside the timed window), and the healed batch is
compared with the original.
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
    n = k + m
    B = max(2, int(gib * (1 << 30)) // (k * S))
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    truth_d, truth_p = data.clone(), parity.clone()
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    vcnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    bad = torch.zeros((B,), dtype=torch.int32, device="cuda")
    pm = torch.zeros((B, fec.mask_words(n)), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")

    # one corrupt byte per block, planted by xor (planting twice restores the block)
    shard = rng.integers(0, n, B)
    flat_d, flat_p = data.view(-1), parity.view(-1)
    pos = torch.from_numpy(np.where(shard < k, (np.arange(B) * k + shard) * S,
                                    (np.arange(B) * m + shard - k) * S) + rng.integers(0, L, B)).cuda()
    val = torch.from_numpy(rng.integers(1, 256, B).astype(np.uint8)).cuda()
    in_data = torch.from_numpy(shard < k).cuda()
    shard_t = torch.from_numpy(shard.astype(np.int32)).cuda()

    def plant(blocks):
        d, p = blocks[in_data[blocks]], blocks[~in_data[blocks]]
        flat_d[pos[d]] ^= val[d]
        flat_p[pos[p]] ^= val[p]

    def verify():
        codec.rs_verify_split(k, m, data, parity, st, vcnt, shard_len=L)

    def locate():
        codec.rs_locate_split(k, m, data, parity, bad, pm, cnt, shard_len=L)

    def locate_bare():   # verdicts alone: no finalize kernel, no counts to clear
        codec.rs_locate_split(k, m, data, parity, bad, shard_len=L)

    def some():
        codec.rs_reconstruct_some_split(k, m, data, parity, pm.view(-1), shard_len=L)

    order = torch.from_numpy(rng.permutation(B)).cuda()
    one_pct = order[:max(1, B // 100)]
    rows = []
    base = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3)}
    for name, add in [("clean", None), ("one_percent", one_pct), ("all", order[one_pct.numel():])]:
        if add is not None:
            plant(add)
        corrupt = torch.zeros((B,), dtype=torch.bool, device="cuda")
        if name != "clean":
            corrupt[one_pct if name == "one_percent" else order] = True
        locate()
        verify()
        codec.sync()
        want = torch.where(corrupt, shard_t, torch.full_like(shard_t, fec.FEC_LOCATE_CLEAN))
        assert torch.equal(bad, want), "locate names the planted shards"
        assert cnt.cpu().tolist() == [int(corrupt.sum()), 0] and int(vcnt.cpu()[0]) == int(corrupt.sum())
        v_ms, l_ms, v2_ms, b_ms = timed_round_robin(torch, [verify, locate, verify, locate_bare], warmup, reps)
        row = dict(base, batch=name, corrupt_blocks=int(corrupt.sum()), verify_ms=round(v_ms, 4),
                   locate_ms=round(l_ms, 4), verify_again_ms=round(v2_ms, 4), locate_bare_ms=round(b_ms, 4),
                   locate_bare_over_verify=round(b_ms / v_ms, 4),
                   locate_over_verify=round(l_ms / v_ms, 4), verify_self=round(v2_ms / v_ms, 4),
                   verify_TBps=round(n * R * B / (v_ms * 1e-3) / 1e12, 4),
                   locate_TBps=round(n * R * B / (l_ms * 1e-3) / 1e12, 4))
        if heal and name != "clean":
            blocks = one_pct if name == "one_percent" else order

            def locate_and_heal():
                locate()
                some()
            locate_and_heal()
            codec.sync()
            assert torch.equal(data[:, :, :L], truth_d[:, :, :L]) and torch.equal(parity[:, :, :L], truth_p[:, :, :L]), \
                "the heal loop restores the batch"
            # the batch is whole now: each round plants the errors again first
            h_ms, = timed_round_robin(torch, [locate_and_heal], warmup, reps, before=lambda i: plant(blocks))
            codec.sync()
            assert torch.equal(data[:, :, :L], truth_d[:, :, :L]) and torch.equal(parity[:, :, :L], truth_p[:, :, :L])
            plant(blocks)
            row.update(heal_ms=round(h_ms, 4), heal_over_verify=round(h_ms / v_ms, 4))
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
    out = {"tool": "locate_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "rows": []}
    for k, m, heal in [(8, 4, True), (20, 10, False), (64, 16, False)]:
        out["rows"] += code_rows(fec, torch, codec, k, m, a.gib, a.warmup, a.reps, heal)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
