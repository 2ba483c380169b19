#!/usr/bin/env python3
"""Time wide reconstruct-some (fec_rs_reconstruct_some_wide_batch) beside the calls that did its work
before it existed, on the same buffers: device-resident, event-timed, warm-up then --reps timed runs,
one JSON line (kept as profiles/wide/some_wide_bench.log).

    python tools/some_wide_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

Per code, RS(32,48), RS(64,80) and RS(128,256), 1202-byte shards in 1216-byte slots, --gib GiB of data
shards per batch:
  (a) data-only want mask beside fec_rs_reconstruct_wide_batch, the losses of tools/wide_bench.py
      (U{1..16}, 16 and 32 erased data shards per block). Both run the same rebuild kernel over records
      of the same size, so a difference is the plan kernel's. The old call is timed twice, before and
      after the new one: the run's spread.
  (b) data intact, every parity shard lost, want = NULL, beside fec_rs_encode_batch(k, m).
  (c) one parity shard lost in 1 % of the blocks, and in every block, beside a full fec_rs_encode_batch,
      which was the only way to put a parity shard of such a code back.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from wide_bench import L, S, timed  # noqa: E402


def dev_words(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def shape_case(fec, torch, codec, k, m, emin, emax, gib, warmup, reps):
    rng = np.random.default_rng(100 * k + m)
    B = max(1, int(gib * (1 << 30)) // (k * S))
    n = k + m
    data = torch.zeros((B, k, S), dtype=torch.uint8, device="cuda")
    data[:, :, :L] = torch.randint(0, 256, (B, k, L), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    ref_parity = parity.clone()
    work = data.clone()

    def r3(x):
        return round(x, 3)

    def pair(new, old, check):
        """median ms of old, new, old again; check() after the first run of each."""
        for fn in (new, old):
            fn()
            assert codec.lib_sync_rc() == fec.FEC_OK
            check()
        o1, _ = timed(torch, old, warmup, reps)
        nw, nw_min = timed(torch, new, warmup, reps)
        o2, _ = timed(torch, old, warmup, reps)
        old_ms = (o1 + o2) / 2
        return {"new_ms": r3(nw), "new_min_ms": r3(nw_min), "old_ms": r3(old_ms), "old_runs_ms": [r3(o1), r3(o2)],
                "old_spread": r3(abs(o1 - o2) / old_ms), "new_over_old": r3(nw / old_ms)}

    def intact():
        assert torch.equal(work, data) and torch.equal(parity, ref_parity), "the batch was not put back"

    res = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3)}

    # (a) erased data shards, data-only want mask, beside the wide reconstruct
    e = rng.integers(emin, emax + 1, B)
    order = np.argsort(rng.random((B, k)), axis=1)
    present = np.ones((B, n), dtype=bool)
    present[:, :k] = order >= e[:, None]
    want = np.zeros((B, n), dtype=bool)
    want[:, :k] = True
    dm, dw = dev_words(torch, fec.wide_masks(present)), dev_words(torch, fec.wide_masks(want))
    res["a_data_only"] = dict(
        losses="U{%d..%d}" % (emin, emax) if emin != emax else str(emax), mean_rows=round(float(e.mean()), 2),
        **pair(lambda: codec.rs_reconstruct_some_wide_split(k, m, work, parity, dm, want=dw, shard_len=L),
               lambda: codec.rs_reconstruct_wide_split(k, m, work, parity, dm, shard_len=L), intact))

    # (b) every parity shard lost, beside the encode
    present = np.zeros((B, n), dtype=bool)
    present[:, :k] = True
    dm_b = dev_words(torch, fec.wide_masks(present))
    res["b_all_parity"] = dict(
        rows=m, **pair(lambda: codec.rs_reconstruct_some_wide_split(k, m, work, parity, dm_b, shard_len=L),
                       lambda: codec.rs_encode_split(k, m, work, parity, shard_len=L), intact))

    # (c) one parity shard lost in 1 % of the blocks / in every block, beside a full encode
    for name, frac in (("c_one_parity_1pct", 0.01), ("c_one_parity_every_block", 1.0)):
        hit = rng.random(B) < frac
        present = np.ones((B, n), dtype=bool)
        present[hit, k + rng.integers(0, m, int(hit.sum()))] = False
        dm_c = dev_words(torch, fec.wide_masks(present))
        res[name] = dict(
            blocks_hit=int(hit.sum()),
            **pair(lambda: codec.rs_reconstruct_some_wide_split(k, m, work, parity, dm_c, shard_len=L),
                   lambda: codec.rs_encode_split(k, m, work, parity, shard_len=L), intact))
    codec.sync()
    del data, parity, work, ref_parity
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    fec = importlib.import_module("0xfec_amd")
    codec = fec.Codec(0).use_torch_stream()
    out = {"tool": "some_wide_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "shapes": []}
    for k, m, emin, emax in [(32, 16, 1, 16), (64, 16, 16, 16), (128, 128, 32, 32)]:
        out["shapes"].append(shape_case(fec, torch, codec, k, m, emin, emax, a.gib, a.warmup, a.reps))
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
