#!/usr/bin/env python3
"""Time fec_rs_verify_batch and fec_rs_reconstruct_some_batch beside the call each would otherwise
be composed from, on the same buffers: device-resident, event-timed, one JSON line. The two calls of
a pair are timed alternately in one process (warm-up, then --reps rounds) and the medians reported:
separate processes disagree by several percent.

    python tools/verify_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

1200-byte shards, --gib GiB of data slots per batch. Rows:
  verify            RS(8,12), RS(20,30), RS(64,80): verify of a clean batch beside the encode of the
                    same code. Both move k + m shard slots per block (verify reads them all, the
                    encode reads k and writes m): TBps = (k + m) * round_up(L, 16) * B / time.
  some_data         reconstruct-some with a data-only want mask beside fec_rs_reconstruct_batch on the
                    same masks: RS(8,12) with one erased data shard per block, RS(20,30) with U{1..10}.
                    The gap is the price of the plain route (no sorted plans, wave or compile-time-k
                    rebuilds, direct body). TBps = (k + e) shard slots per block over the time.
  some_all_parity   reconstruct-some of a batch whose parity is all lost (want = NULL) beside the
                    encode: RS(8,12), RS(20,30). TBps as for the encode.
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


def tbps(slots, ms):
    return round(slots * S / (ms * 1e-3) / 1e12, 4)


def code_rows(fec, torch, codec, k, m, gib, warmup, reps, some):
    rng = np.random.default_rng(100 * k + m)
    B = max(2, int(gib * (1 << 30)) // (k * S))
    n = k + m
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    truth_d, truth_p = data.clone(), parity.clone()
    rows = []
    base = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3)}

    def encode():
        codec.rs_encode_split(k, m, data, parity, shard_len=L)

    def verify():
        codec.rs_verify_split(k, m, data, parity, st, cnt, shard_len=L)

    verify()
    codec.sync()
    assert int(cnt.cpu()[0]) == 0 and bool((st == 1).all()), "a clean batch must verify"
    v_ms, e_ms = timed_pair(torch, verify, encode, warmup, reps)
    rows.append(dict(base, row="verify", verify_ms=round(v_ms, 4), encode_ms=round(e_ms, 4),
                     verify_over_encode=round(v_ms / e_ms, 4), verify_TBps=tbps(B * n, v_ms),
                     encode_TBps=tbps(B * n, e_ms)))
    if not some:
        return rows

    # data-only want mask beside ReconstructData: e erased data shards per block
    e = np.ones(B, dtype=np.int64) if k == 8 else rng.integers(1, m + 1, B)
    order = np.argsort(rng.random((B, k)), axis=1)
    present = np.ones((B, n), dtype=bool)
    present[:, :k] = order >= e[:, None]
    bits = (present * (1 << np.arange(n, dtype=np.uint64))[None, :]).sum(axis=1)
    dm = torch.from_numpy(bits.astype(np.uint32).view(np.int32)).cuda()
    want = torch.full((B,), (1 << k) - 1, dtype=torch.int32, device="cuda")
    data[torch.from_numpy(~present[:, :k]).cuda()] = 0x5A

    def some_data():
        codec.rs_reconstruct_some_split(k, m, data, parity, dm, want=want, status=st, shard_len=L)

    def recon():
        codec.rs_reconstruct_split(k, m, data, parity, dm, status=st, shard_len=L)

    some_data()
    assert codec.lib_sync_rc() == fec.FEC_OK and torch.equal(data, truth_d), "reconstruct-some (data) is wrong"
    s_ms, r_ms = timed_pair(torch, some_data, recon, warmup, reps)
    assert torch.equal(data, truth_d)
    moved = int((k + e).sum())
    rows.append(dict(base, row="some_data", erased="1" if k == 8 else "U{1..%d}" % m, some_ms=round(s_ms, 4),
                     reconstruct_ms=round(r_ms, 4), some_over_reconstruct=round(s_ms / r_ms, 4),
                     some_TBps=tbps(moved, s_ms), reconstruct_TBps=tbps(moved, r_ms)))

    # all parity lost, want = NULL, beside the encode
    dm2 = torch.full((B,), (1 << k) - 1, dtype=torch.int32, device="cuda")
    parity.fill_(0x5A)

    def some_par():
        codec.rs_reconstruct_some_split(k, m, data, parity, dm2, status=st, shard_len=L)

    some_par()
    assert codec.lib_sync_rc() == fec.FEC_OK and torch.equal(parity, truth_p), "reconstruct-some (parity) is wrong"
    p_ms, e_ms = timed_pair(torch, some_par, encode, warmup, reps)
    rows.append(dict(base, row="some_all_parity", some_ms=round(p_ms, 4), encode_ms=round(e_ms, 4),
                     some_over_encode=round(p_ms / e_ms, 4), some_TBps=tbps(B * n, p_ms),
                     encode_TBps=tbps(B * n, e_ms)))
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
    out = {"tool": "verify_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "rows": []}
    for k, m, some in [(8, 4, True), (20, 10, True), (64, 16, False)]:
        out["rows"] += code_rows(fec, torch, codec, k, m, a.gib, a.warmup, a.reps, some)
        torch.cuda.empty_cache()
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
