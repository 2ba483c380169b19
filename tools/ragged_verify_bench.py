#!/usr/bin/env python3
"""Time the ragged verify and the ragged reconstruct-some (include/fec_hip_ragged.h) beside their
uniform calls at the longest length on the same buffers: device-resident, event-timed, one JSON line.
The sibling of tools/ragged_bench.py, whose pairing and length distributions it takes: the two calls of
a pair are timed alternately in one process (warm-up, then --reps rounds of ragged, uniform) and the
medians reported, each with its spread over the repetitions (`*_spread_ms`: minimum, lower quartile,
median, upper quartile, maximum).

    python tools/ragged_verify_bench.py [--reps 20] [--warmup 3] [--gib 1.0] [--rag-g N] [--codes 8,4 20,10]

Codes RS(8,12) and RS(20,30), 1216-byte slots, --gib GiB of data slots per batch. Length
distributions: (a) every block 1202 bytes, (b) 1202 and 50 alternating, (c) U{1..1202}. Calls: verify
of a clean batch (no atomics) with a count, and reconstruct-some with one data and one parity shard
missing per block (every shard wanted); the ragged calls on parity encoded at each block's own
length, the uniform calls on parity encoded at the full length, over the same data.
`traffic_fraction` is the sum of the blocks' chunk counts over nblocks * the chunks of a full-length
shard; `scaled_uniform_ms` is the uniform call's time times it: what the ragged call takes if its
time follows the bytes it moves.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ragged_bench import L, S, lengths  # noqa: E402


def timed_pair(torch, fa, fb, warmup, reps):
    """ms of fa and of fb, timed alternately: two lists of `reps` samples."""
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
    return ms


def spread(ms):
    """[min, lower quartile, median, upper quartile, max] of the samples."""
    return [round(float(v), 4) for v in np.percentile(ms, [0, 25, 50, 75, 100])]


def code_case(fec, torch, codec, k, m, gib, warmup, reps):
    rng = np.random.default_rng(100 * k + m)
    B = max(2, int(gib * (1 << 30)) // (k * S))
    n = k + m
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")        # of the ragged calls
    parity_full = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")   # of the uniform calls
    codec.rs_encode_split(k, m, data, parity_full, shard_len=L)
    st_r = torch.zeros(B, dtype=torch.int32, device="cuda")
    st_u = torch.zeros(B, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    lost_d, lost_p = rng.integers(0, k, B), k + rng.integers(0, m, B)
    bits = ((1 << n) - 1) & ~((1 << lost_d) | (1 << lost_p))
    dm = torch.from_numpy(bits.astype(np.uint32).view(np.int32)).cuda()
    res = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3), "cases": []}
    for dist in ("a", "b", "c"):
        lens = lengths(dist, B, rng)
        r16 = (lens.astype(np.int64) + 15) // 16 * 16
        frac = float(r16.sum()) / (B * S)
        dl = torch.from_numpy(lens.view(np.int32)).cuda()
        # parity that is right at each block's own length (and so, in case a, at the uniform length)
        codec.rs_encode_ragged_split(k, m, data, parity, dl, max_shard_len=L)
        codec.sync()
        pairs = {
            "verify": (lambda: codec.rs_verify_ragged_split(k, m, data, parity, dl, st_r, cnt, max_shard_len=L),
                       lambda: codec.rs_verify_split(k, m, data, parity_full, st_u, cnt, shard_len=L), n),
            "reconstruct_some": (lambda: codec.rs_reconstruct_some_ragged_split(k, m, data, parity, dm, dl,
                                                                                status=st_r, max_shard_len=L),
                                 lambda: codec.rs_reconstruct_some_split(k, m, data, parity_full, dm, status=st_u,
                                                                         shard_len=L), k + 2),
        }
        for name, (ragged, uniform, shards_moved) in pairs.items():
            # (the ragged rebuild zeroes a data shard's bytes up to round_up(len, 16); the uniform one,
            # which comes last in every round, puts the full-length shard back)
            ragged()
            assert codec.lib_sync_rc() == fec.FEC_OK
            if name == "verify":
                assert bool((st_r == 1).all()) and int(cnt[0]) == 0, "the ragged verify finds a clean batch bad"
            r_all, u_all = timed_pair(torch, ragged, uniform, warmup, reps)
            r_ms, u_ms = float(np.median(r_all)), float(np.median(u_all))
            assert codec.lib_sync_rc() == fec.FEC_OK
            assert torch.equal(st_r, st_u), "ragged and uniform %s disagree" % name
            res["cases"].append({"lengths": dist, "call": name, "traffic_fraction": round(frac, 4),
                                 "ragged_ms": round(r_ms, 4), "uniform_ms": round(u_ms, 4),
                                 "ragged_spread_ms": spread(r_all), "uniform_spread_ms": spread(u_all),
                                 "scaled_uniform_ms": round(u_ms * frac, 4),
                                 "ragged_over_uniform": round(r_ms / u_ms, 4),
                                 "ragged_over_scaled": round(r_ms / (u_ms * frac), 4),
                                 "ragged_TBps": round(int(r16.sum()) * shards_moved / (r_ms * 1e-3) / 1e12, 4)})
    del data, parity, parity_full
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
    out = {"tool": "ragged_verify_bench", "device": torch.cuda.get_device_name(0), "max_shard_len": L, "slot": S,
           "reps": a.reps, "rag_g": a.rag_g, "codes": []}
    codec.set_tuning(rag_g=a.rag_g)
    for k, m in [tuple(int(v) for v in c.split(",")) for c in a.codes]:
        out["codes"].append(code_case(fec, torch, codec, k, m, a.gib, a.warmup, a.reps))
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
