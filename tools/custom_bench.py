#!/usr/bin/env python3
"""Time the RS calls under a custom matrix (fec_hip_matrix.h fec_ctx_set_custom_matrix, kind 2) beside
the default matrix (kind 0), on the same buffers: device-resident, event-timed. The custom matrix is
the default matrix's own parity rows (rs_matrix(k, m)[k:]) registered as a custom code, so both kinds
compute the same bytes and every difference in time is the route: the generic fold against the
fixed-shape encodes, and the elimination plan (fec_plan_solve.hip) against the Lagrange plans; the
rebuild kernels are the same under both. The two kinds of a call are timed alternately in one process
on one ctx (fec_ctx_set_matrix between the calls; warm-up, then --reps rounds) and the medians
reported: separate processes disagree by several percent.

    python tools/custom_bench.py [--reps 20] [--warmup 3] [--gib 0.5] [--out profiles/custom/custom_bench.log]

1202-byte shards in 1216-byte slots, --gib GiB of data slots per batch. Per code (RS(8,12), RS(16,24),
RS(20,30)) four rows:
  encode          data -> a parity region of its own
  recover_1       one erased data shard per block, rebuilt into one out slot
  recover_multi   e ~ U{1..m} erased shards per block over all n, the erased data shards rebuilt into
                  min(k, m) out slots
  verify          a clean batch
Each row reports the two medians in ms and their ratio custom / default; no ratio is judged here.
The JSON line is printed and written to --out.
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
CODES = [(8, 4), (16, 8), (20, 10)]
KINDS = ("vandermonde", "custom")


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


def code_rows(fec, torch, codec, k, m, gib, warmup, reps):
    rng = np.random.default_rng(100 * k + m)
    B = max(2, int(gib * (1 << 30)) // (k * S))
    n = k + m
    data = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda")
    data[:, :, L:] = 0
    par = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros((B, m, S), dtype=torch.uint8, device="cuda")
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    codec.set_custom_matrix(k, m, fec.rs_matrix(k, m)[k:])     # the ctx is now under kind custom
    codec.set_matrix("vandermonde")
    codec.rs_encode_split(k, m, data, par, shard_len=L)
    codec.sync()
    base = {"code": "RS(%d,%d)" % (k, n), "blocks": B, "data_GiB": round(B * k * S / (1 << 30), 3)}
    rows = []

    def pair(row, call, check, **extra):
        """call() under each kind, alternately; check() after one call of each."""
        def under(i):
            def fn():
                codec.set_matrix(KINDS[i])
                call()
            return fn
        for i in range(2):
            under(i)()
            assert codec.lib_sync_rc() == fec.FEC_OK, (row, KINDS[i])
            check(KINDS[i])
        d_ms, c_ms = timed_pair(torch, under(0), under(1), warmup, reps)
        rows.append(dict(base, row=row, default_ms=round(d_ms, 4), custom_ms=round(c_ms, 4),
                         custom_over_default=round(c_ms / d_ms, 4), **extra))

    def encoded(kind):
        assert torch.equal(scratch, par), "encode under %s differs from the default matrix's parity" % kind
        scratch.zero_()

    pair("encode", lambda: codec.rs_encode_split(k, m, data, scratch, shard_len=L), encoded)

    def clean(kind):
        assert int(cnt.cpu()[0]) == 0 and bool((st == 1).all()), "a clean batch must verify (%s)" % kind

    pair("verify", lambda: codec.rs_verify_split(k, m, data, par, st, cnt, shard_len=L), clean)

    for row, counts, among, slots in (("recover_1", np.ones(B, dtype=np.int64), k, 1),
                                      ("recover_multi", rng.integers(1, m + 1, B), n, min(k, m))):
        order = np.argsort(rng.random((B, among)), axis=1)
        present = np.ones((B, n), dtype=bool)
        present[:, :among] = order >= counts[:, None]
        bits = (present * (1 << np.arange(n, dtype=np.uint64))[None, :]).sum(axis=1)
        dm = torch.from_numpy(bits.astype(np.uint32).view(np.int32)).cuda()
        out = torch.zeros((B, slots, S), dtype=torch.uint8, device="cuda")
        lost = torch.from_numpy(~present[:, :k]).cuda()
        # the bytes a correct recover writes: the lost data shards in ascending order, slot by slot
        rank = torch.cumsum(lost.to(torch.int64), dim=1) - 1
        bi, ji = torch.nonzero(lost, as_tuple=True)
        want = torch.zeros_like(out)
        want[bi, rank[bi, ji]] = data[bi, ji]

        def recover(dm=dm, out=out):
            codec.rs_recover_split(k, m, data, par, dm, out, status=st, shard_len=L)

        def right(kind, out=out, want=want, row=row):
            assert torch.equal(out, want), "%s is wrong under %s" % (row, kind)
            out.zero_()

        pair(row, recover, right, erased="1 data" if slots == 1 else "U{1..%d} of n" % m)
        del out, want
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "custom", "custom_bench.log"))
    a = ap.parse_args()
    import torch
    fec = importlib.import_module("0xfec_amd")
    codec = fec.Codec(0).use_torch_stream()
    res = {"tool": "custom_bench", "device": torch.cuda.get_device_name(0), "shard_len": L, "slot": S,
           "reps": a.reps, "warmup": a.warmup, "rows": []}
    for k, m in CODES:
        res["rows"] += code_rows(fec, torch, codec, k, m, a.gib, a.warmup, a.reps)
        torch.cuda.empty_cache()
    codec.set_matrix("vandermonde")
    codec.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
