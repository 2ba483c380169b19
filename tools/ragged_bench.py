#!/usr/bin/env python3
"""Time the ragged RS calls (a shard length per block) beside the uniform calls at the longest
length on the same buffers: device-resident, event-timed, one JSON line. The two calls of a pair are
timed alternately in one process (warm-up, then --reps rounds of ragged, uniform) and the medians
reported: separate processes disagree by several percent.

    python tools/ragged_bench.py [--reps 20] [--warmup 3] [--gib 1.0] [--rag-g N] [--codes 8,4 20,10]

--rag-g forces the blocks per tile of both ragged kernels (the test-only knob rag_g; 0: the default).

Codes RS(8,12) and RS(20,30), 1216-byte slots, --gib GiB of data slots per batch. Length
distributions: (a) every block 1202 bytes, (b) 1202 and 50 alternating, (c) U{1..1202}. Calls: encode,
recover with one erased data shard per block (one out slot), recover with U{1..m} erased (m out
slots). `ragged_TBps` is sum over blocks of (shards read + shards written) * round_up(len_b, 16) over
the ragged call's time; `len_fraction` is mean round_up(len_b, 16) / 1216; `cross_fraction` (from case
a) is uniform / ragged time at full length: the mean-length fraction below which the ragged call
should win if its time follows the bytes it moves.
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


def timed_pair(torch, fa, fb, warmup, reps):
    """Median ms of fa and of fb, timed alternately."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return float(np.median(ms[0])), float(np.median(ms[1]))


def lengths(dist, B, rng):
    if dist == "a":
        return np.full(B, L, dtype=np.uint32)
    if dist == "b":
        return np.where(np.arange(B) % 2 == 0, L, 50).astype(np.uint32)
    return rng.integers(1, L + 1, B).astype(np.uint32)


def code_case(fec, torch, codec, k, m, gib, warmup, reps):
    rng = np.random.default_rng(100 * k + m)
    B = max(2, int(gib * (1 << 30)) // (k * S))
    n = k + m
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")    # parity of the timed encodes
    out = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    out2 = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    order = np.argsort(rng.random((B, k)), axis=1)   # a random permutation of the data shards per block

    def masks_for(e):
        present = np.ones((B, n), dtype=bool)
        present[:, :k] = order >= e[:, None]
        bits = (present * (1 << np.arange(n, dtype=np.uint64))[None, :]).sum(axis=1)
        return torch.from_numpy(bits.astype(np.uint32).view(np.int32)).cuda()

    e_one = np.ones(B, dtype=np.int64)
    e_multi = rng.integers(1, m + 1, B)
    calls = [("encode", None, 0), ("recover_1", e_one, 1), ("recover_U1..m", e_multi, m)]
    res = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3), "cases": []}
    cross = {}
    for dist in ("a", "b", "c"):
        lens = lengths(dist, B, rng)
        r16 = (lens.astype(np.int64) + 15) // 16 * 16
        dl = torch.from_numpy(lens.view(np.int32)).cuda()
        for name, e, slots in calls:
            if e is None:
                def ragged():
                    codec.rs_encode_ragged_split(k, m, data, scratch, dl, max_shard_len=L)

                def uniform():
                    codec.rs_encode_split(k, m, data, scratch, shard_len=L)
                moved = int((r16 * n).sum())
            else:
                dm = masks_for(e)
                o_r, o_u = out[:, :slots], out2[:, :slots]
                if slots != m:
                    o_r, o_u = out[:, :slots].contiguous(), out2[:, :slots].contiguous()

                def ragged(dm=dm, o_r=o_r):
                    codec.rs_recover_ragged_split(k, m, data, parity, dm, dl, o_r, max_shard_len=L)

                def uniform(dm=dm, o_u=o_u):
                    codec.rs_recover_split(k, m, data, parity, dm, o_u, shard_len=L)
                moved = int((r16 * (k + e)).sum())
            ragged()
            assert codec.lib_sync_rc() == fec.FEC_OK
            if dist == "a":   # same lengths: the two calls must leave the same bytes
                if e is None:
                    assert torch.equal(scratch, parity), "ragged encode differs from the uniform encode"
                    scratch.zero_()
                else:
                    uniform()
                    assert codec.lib_sync_rc() == fec.FEC_OK
                    assert torch.equal(o_r, o_u), "ragged and uniform %s disagree" % name
            r_ms, u_ms = timed_pair(torch, ragged, uniform, warmup, reps)
            codec.sync()
            if dist == "a":
                cross[name] = u_ms / r_ms
            res["cases"].append({"lengths": dist, "call": name, "len_fraction": round(float(r16.mean()) / S, 4),
                                 "ragged_ms": round(r_ms, 4), "uniform_ms": round(u_ms, 4),
                                 "ragged_over_uniform": round(r_ms / u_ms, 4),
                                 "ragged_TBps": round(moved / (r_ms * 1e-3) / 1e12, 4),
                                 "cross_fraction": round(cross[name], 4)})
    del data, parity, scratch, out, out2
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--rag-g", type=int, default=0)
    ap.add_argument("--codes", nargs="*", default=["8,4", "20,10"], help="k,m pairs")
    a = ap.parse_args()
    import torch
    fec = importlib.import_module("0xfec_amd")
    codec = fec.Codec(0).use_torch_stream()
    out = {"tool": "ragged_bench", "device": torch.cuda.get_device_name(0), "max_shard_len": L, "slot": S,
           "reps": a.reps, "rag_g": a.rag_g, "codes": []}
    codec.set_tuning(rag_g=a.rag_g)
    for k, m in [tuple(int(v) for v in c.split(",")) for c in a.codes]:
        out["codes"].append(code_case(fec, torch, codec, k, m, a.gib, a.warmup, a.reps))
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
