#!/usr/bin/env python3
"""Time the wide RS reconstruct (fec_rs_reconstruct_wide_batch) beside the library's own generic
encode on the same buffers: device-resident, event-timed, warm-up then --reps timed runs, one JSON
line. The encode fec_rs_encode_batch(k, e_max) does the same e x k products per chunk with its
tables expanded once per launch; the wide rebuild adds a plan-record read per block, the table
expansion per block and the input gather.

    python tools/wide_bench.py [--reps 20] [--warmup 3] [--gib 1.0]

Shapes: RS(32,48) with U{1..16} erased data shards per block, RS(64,80) with exactly 16, RS(128,256)
with exactly 32; and RS(20,30) with U{1..10} through the wide kernels (two mask words) beside the
narrow call (what the tuned narrow path is worth). 1202-byte shards in 1216-byte slots, --gib GiB of
data shards per batch.
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


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def shape_case(fec, torch, codec, k, m, emin, emax, gib, warmup, reps, narrow=False):
    rng = np.random.default_rng(100 * k + m)
    B = max(1, int(gib * (1 << 30)) // (k * S))
    n = k + m
    data = torch.zeros((B, k, S), dtype=torch.uint8, device="cuda")
    data[:, :, :L] = torch.randint(0, 256, (B, k, L), dtype=torch.uint8, device="cuda")
    parity = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, data, parity, shard_len=L)
    codec.sync()
    e = rng.integers(emin, emax + 1, B)
    order = np.argsort(rng.random((B, k)), axis=1)           # a random permutation of the data shards per block
    present = np.ones((B, n), dtype=bool)
    present[:, :k] = order >= e[:, None]                      # e of them erased
    W = max(2, fec.mask_words(n))                             # two words at least: the wide kernels
    masks = np.zeros((B, W), dtype=np.uint32)
    masks[:, :fec.mask_words(n)] = fec.wide_masks(present)
    dm = torch.from_numpy(masks.view(np.int32)).cuda()
    work = data.clone()
    scratch = torch.zeros((B, emax, S), dtype=torch.uint8, device="cuda")

    def decode():
        codec.rs_reconstruct_wide_split(k, m, work, parity, dm, shard_len=L)

    def encode():
        codec.rs_encode_split(k, emax, data, scratch, shard_len=L)

    decode()
    assert codec.lib_sync_rc() == fec.FEC_OK
    assert torch.equal(work, data), "wide reconstruct did not give the data back"
    dec_ms, dec_min = timed(torch, decode, warmup, reps)
    enc_ms, enc_min = timed(torch, encode, warmup, reps)
    codec.sync()
    res = {"code": "RS(%d,%d)" % (k, n), "losses": "U{%d..%d}" % (emin, emax) if emin != emax else str(emax),
           "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3), "mean_rows": round(float(e.mean()), 2),
           "decode_ms": round(dec_ms, 3), "decode_min_ms": round(dec_min, 3),
           "encode_rows": emax, "encode_ms": round(enc_ms, 3), "encode_min_ms": round(enc_min, 3),
           "decode_over_encode": round(dec_ms / enc_ms, 3)}
    if narrow:
        dm1 = torch.from_numpy(np.ascontiguousarray(masks[:, 0]).view(np.int32)).cuda()

        def decode_narrow():
            codec.rs_reconstruct_split(k, m, work, parity, dm1, shard_len=L)

        decode_narrow()
        assert codec.lib_sync_rc() == fec.FEC_OK and torch.equal(work, data)
        nar_ms, nar_min = timed(torch, decode_narrow, warmup, reps)
        res.update(narrow_ms=round(nar_ms, 3), narrow_min_ms=round(nar_min, 3),
                   wide_over_narrow=round(dec_ms / nar_ms, 3))
    del data, parity, work, scratch
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
    out = {"tool": "wide_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S, "reps": a.reps,
           "shapes": []}
    for k, m, emin, emax, narrow in [(32, 16, 1, 16, False), (64, 16, 16, 16, False), (128, 128, 32, 32, False),
                                     (20, 10, 1, 10, True)]:
        out["shapes"].append(shape_case(fec, torch, codec, k, m, emin, emax, a.gib, a.warmup, a.reps, narrow))
    codec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
