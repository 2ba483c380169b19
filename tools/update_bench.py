#!/usr/bin/env python3
"""Time fec_rs_encode_idx_batch and fec_rs_update_batch beside the full encode of the same code, on
the same buffers: device-resident, event-timed, one JSON line. All cases of a code are timed
alternately in one process (warm-up, then --reps rounds) and the medians reported: separate
processes disagree by several percent.

    python tools/update_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

1200-byte shards, --gib GiB of data slots per batch (and as much again of new data). For each of
k = 8, m = 4 (RS(8,12)), k = 20, m = 10 (RS(20,30)) and k = 100, m = 4:
  encode            fec_rs_encode_batch: k + m shard slots per block
  encode_idx c      c = 1 and c = k columns per block (a random set per block)
  update c          c = 1, 2 and k / 2 changed columns per block
Each case moves (c*s + 2m) * round_up(L, 16) bytes per block (s = 1 for encode-idx, 2 for update:
the masked columns read, every parity slot read and written). TBps is that over the time;
`yardstick_ms` is the encode's time on these buffers scaled by the traffic ratio (c*s + 2m) / (k + m),
and `over_yardstick` the case's time over it. The tool sets no threshold.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = S = 1200
R = (L + 15) // 16 * 16


def timed_round_robin(torch, fns, warmup, reps):
    """Median ms of each function, timed alternately."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [float(np.median(x)) for x in ms]


def column_masks(fec, torch, rng, B, k, c):
    """uint32 [B, W] device masks with c random columns per block."""
    order = np.argsort(rng.random((B, k)), axis=1)
    return torch.from_numpy(fec.wide_masks(order < c).view(np.int32)).cuda()


def code_rows(fec, torch, codec, k, m, gib, warmup, reps):
    rng = np.random.default_rng(100 * k + m)
    B = max(2, int(gib * (1 << 30)) // (k * S))
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    new = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")

    # every column into zeroed parity is the encode
    codec.rs_encode_idx_split(k, m, data, parity, column_masks(fec, torch, rng, B, k, k), shard_len=L)
    acc = parity.clone()
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    assert torch.equal(acc, parity), "encode-idx of every column must equal the encode"

    cases = [("encode", 0, 0, lambda: codec.rs_encode_split(k, m, data, parity, shard_len=L))]
    for c in (1, k):
        mk = column_masks(fec, torch, rng, B, k, c)
        cases.append(("encode_idx", c, 1,
                      lambda mk=mk: codec.rs_encode_idx_split(k, m, data, parity, mk, shard_len=L)))
    for c in (1, 2, k // 2):
        mk = column_masks(fec, torch, rng, B, k, c)
        cases.append(("update", c, 2,
                      lambda mk=mk: codec.rs_update_split(k, m, data, new, parity, mk, shard_len=L)))
    ms = timed_round_robin(torch, [f for _, _, _, f in cases], warmup, reps)
    codec.sync()
    enc_ms = ms[0]
    rows = []
    for (name, c, s, _), t in zip(cases, ms):
        slots = (k + m) if name == "encode" else c * s + 2 * m
        row = {"code": "k=%d,m=%d" % (k, m), "blocks": B, "case": name, "columns": c, "ms": round(t, 4),
               "bytes_per_block": slots * R, "TBps": round(slots * R * B / (t * 1e-3) / 1e12, 4)}
        if name != "encode":
            y = enc_ms * slots / (k + m)
            row.update(yardstick_ms=round(y, 4), over_yardstick=round(t / y, 3))
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
    out = {"tool": "update_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "rows": []}
    for k, m in [(8, 4), (20, 10), (100, 4)]:
        out["rows"] += code_rows(fec, torch, codec, k, m, a.gib, a.warmup, a.reps)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
