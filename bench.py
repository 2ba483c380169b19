#!/usr/bin/env python3
"""bench.py — device-resident FEC encode+decode throughput on MI355X.

Metric (BASELINE.json): device-resident FEC encode+decode GiB/s, 1200B symbols, RS k=8 n=12.
Workload (configs[2]): RS(k=8, n=12), 2^20 blocks per GPU, 1200-byte payloads framed as
1202-byte shards (payload | big-endian uint16 length, internal/fec/reed_solomon.go:70-89),
random single data-shard erasure per block.

One step = one pass of the hot path over the resident batch:
    encode  fec_rs_encode_batch   (klauspost Encode, reed_solomon.go:51): data -> parity
    decode  fec_rs_recover_batch  (ReconstructData + copy-out of recoverSymbolPayloads,
            reed_solomon.go:92-136): the erased data shard of every block rebuilt from the
            first k present shards into a recovered-shard buffer
The in-place form (fec_rs_reconstruct_batch) is timed separately and reported beside it.
Inputs are resident in HBM before timing starts. value = payload GiB/s over all ranks
= N * B * k * 1200 / 2^30 / step time (max over ranks). Multi-GPU: every rank owns its own
2^20 contiguous blocks (weak scaling), no collective on the data path.

Run:  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
      torchrun --nproc-per-node N bench.py --gpus N ...   (N > 1)
A plain run does what the headline figure needs and no more: it generates the batch, runs W
warm-up steps, times K steps and prints the result line (metric, value, ms_per_step and the
per-kernel event times of those same K steps). --dump-outputs DIR also writes what the last
timed step computed (dump_outputs below). --full adds everything else the benchmark measures or
checks, each in runs of its own after the timed steps: the full-batch round-trip check, the
in-place reconstruct, the traffic twins and the roofline figures, the host-resident (PCIe)
path, the oracle spot-check and the CPU baseline.

`python bench.py --gpus N` with N > 1 and no torchrun environment starts torchrun itself, as a
child process, before anything touches the GPU, and exits with its status; it refuses (exit 2)
when fewer than N devices are visible. Under torchrun, a WORLD_SIZE different from --gpus is
refused as well, so an N-GPU request never comes back as a 1-GPU number.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PAYLOAD = 1200
SHARD_LEN = PAYLOAD + 2          # + big-endian uint16 length trailer
SHARD_STRIDE = 1216              # 16-byte aligned device slot per shard
HBM_PEAK = 8.0e12                # MI355X HBM3E spec, bytes/s (MI355X_MICROARCH.md)
# traffic-twin ceiling search (best_twin): resident workgroups per CU (0: as many as fit) and
# offsets of the twin's output from its buffer's start (the output buffers carry TWIN_SLACK spare
# bytes for them; the codec kernels always write at offset 0)
TWIN_WPC = (1, 2, 3, 4, 5, 0)
TWIN_OFFSETS = (0, 4160, 65600)
TWIN_SLACK = 1 << 17
# rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of this bench (separate passes, tools/pmc_traffic.py,
# gfx950 FETCH_SIZE x2 correction): HBM bytes per launch of each codec kernel, with the hash of
# the kernel's machine code at profiling time (tools/gpu_round.sh pmc refreshes it)
TRAFFIC_JSON = os.path.join(ROOT, "profiles", "pmc_traffic_latest.json")


def encode_kernel_name(k, m):
    """The kernel fec_rs_encode_batch runs for (k, m) at the library's default tuning
    (fec_encode.hip launch_rs_encode_fixed: RS(8,12) the dyadic fixed-shape kernel, RS(2,3) its
    parity-row kernel, RS(16,24) / RS(20,30) the bit-sliced one, other shapes the generic kernel)."""
    if (k, m) == (8, 4):
        return "rs_encode_fixed_kernel<8, 4"
    if (k, m) == (2, 1):
        return "rs_encode23_kernel<"
    if (k, m) in ((16, 8), (20, 10)):
        return "rs_encode_bits_kernel<%d, %d" % (k, m)
    return "rs_encode_kernel<"


def committed_traffic(kernel_prefix, tu):
    """HBM bytes per launch of the kernel from the committed PMC profile, or None when there is
    none or when the profile describes another kernel than the one built now: its recorded hash
    of the kernel's machine code (or, for older profiles, of its translation unit's sources)
    differs from the built library's."""
    sys.path.insert(0, os.path.join(ROOT, "0xfec_amd"))
    try:
        import _build
        now_src = _build.source_hash(tu)
        now_code = _build.kernel_code_hashes()
    finally:
        sys.path.pop(0)
    try:
        with open(TRAFFIC_JSON) as fh:
            prof = json.load(fh)
    except (OSError, ValueError):
        return None, {"source": None, "note": "no PMC profile committed"}
    for name, rec in prof.items():
        if kernel_prefix in name and rec.get("traffic_bytes"):
            info = {"source": os.path.relpath(TRAFFIC_JSON, ROOT), "kernel": name}
            if rec.get("code_hash"):
                info.update(profile_code_hash=rec["code_hash"], built_code_hash=now_code.get(name))
                same = rec["code_hash"] == now_code.get(name)
            else:
                info.update(profile_source_hash=rec.get("source_hash"), built_source_hash=now_src)
                same = rec.get("source_hash") == now_src
            if not same:
                info["note"] = "stale: the kernel changed since this profile; traffic not reported"
                return None, info
            return rec["traffic_bytes"], info
    return None, {"source": os.path.relpath(TRAFFIC_JSON, ROOT), "note": "kernel not in the profile"}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--m", type=int, default=4)
    p.add_argument("--blocks", type=int, default=1 << 20, help="blocks per GPU")
    p.add_argument("--seed", type=int, default=0x0FEC)
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the checks and the side measurements (round trip, "
                        "in-place reconstruct, traffic twins / roofline, host-resident path, CPU baseline)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the outputs of the last timed step to DIR/<name>.npy (float32; see dump_outputs)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline leg")
    p.add_argument("--cpu-sample-blocks", type=int, default=1 << 15)
    p.add_argument("--host-blocks", type=int, default=1 << 17,
                   help="blocks of the host-resident (PCIe-inclusive) measurement, rank 0 at N=1; 0: skip")
    p.add_argument("--rehearse-one-gpu", action="store_true",
                   help="diagnostics only: every torchrun rank on cuda:0 with gloo (RCCL refuses two ranks "
                        "on one device), to exercise the N>1 code path on a one-GPU box; its timings are "
                        "contended and never a result")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    return args


DUMP_SAMPLE_BLOCKS = 1024


def dump_outputs(torch, batch, out_dir, seed):
    """--dump-outputs: what the last timed step left in the buffers a caller of the hot path
    receives, as float32 .npy files (byte values 0..255 and sums of them below 2^24, so exact):
      parity.npy             [n, m, 1202]  parity shards (fec_rs_encode_batch) of n sampled blocks
      recovered.npy          [n, 1202]     recovered shards (fec_rs_recover_batch) of the same blocks
      sample_blocks.npy      [n]           the sampled block indices within this rank's batch (float64)
      parity_block_sums.npy  [B]           sum of the m x 1202 parity bytes of every block
      recovered_block_sums.npy [B]         sum of the 1202 recovered bytes of every block
    n = min(B, 1024) blocks drawn once from numpy's default_rng(seed), ascending; the sums cover
    the whole batch. About 33 MB at the default 2^20 blocks. Inputs come from the device generator
    keyed by --seed, so two runs with the same arguments write the same files."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    B = batch.B
    pick = np.sort(np.random.default_rng(seed).choice(B, min(B, DUMP_SAMPLE_BLOCKS), replace=False))
    idx = torch.from_numpy(pick).to(batch.parity.device)
    arrays = {
        "parity": batch.parity[idx][:, :, :SHARD_LEN].float(),
        "recovered": batch.recovered[idx][:, 0, :SHARD_LEN].float(),
        "sample_blocks": idx.double(),
        "parity_block_sums": batch.parity[:, :, :SHARD_LEN].sum(dim=(1, 2), dtype=torch.int32).float(),
        "recovered_block_sums": batch.recovered[:, 0, :SHARD_LEN].sum(dim=1, dtype=torch.int32).float(),
    }
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())


def padded(torch, shape, dev):
    """A zeroed device tensor of `shape` at the start of a buffer TWIN_SLACK bytes longer (room for
    the traffic twins' output offsets, best_twin)."""
    n = 1
    for d in shape:
        n *= d
    return torch.zeros(n + TWIN_SLACK, dtype=torch.uint8, device=dev)[:n].view(*shape)


class RankBatch:
    """One rank's slice of the global batch, resident in HBM: data shards [B, k, 1216] and
    parity shards [B, m, 1216] in separate buffers, one erased data shard per block (masks),
    the recovered-shard buffer [B, 1, 1216]. Data and erasures come from the device generator
    (include/fec_synth.h: splitmix64 keyed by (seed, global block, shard, word), BASELINE.md
    §2), so any split over ranks codes the same global batch."""

    def __init__(self, torch, codec, dev, B, k, m, seed, first_block):
        self.B, self.k, self.m, self.first = B, k, m, first_block
        self.data = torch.empty((B, k, SHARD_STRIDE), dtype=torch.uint8, device=dev)
        codec.synth_data(seed, first_block, B, k, PAYLOAD, self.data.data_ptr(), k * SHARD_STRIDE, SHARD_STRIDE)
        self.parity = padded(torch, (B, m, SHARD_STRIDE), dev)
        self.masks = torch.empty((B,), dtype=torch.int32, device=dev)
        self.erased = torch.empty((B,), dtype=torch.int32, device=dev)
        codec.synth_single_erasures(seed, first_block, B, k, m, self.masks.data_ptr(), self.erased.data_ptr())
        self.recovered = padded(torch, (B, 1, SHARD_STRIDE), dev)


class RankStep:
    """The hot path over one RankBatch: encode (fec_rs_encode_batch, reed_solomon.go:51) and
    decode (fec_rs_recover_batch: ReconstructData + the copy-out of recoverSymbolPayloads,
    reed_solomon.go:92-136), plus the in-place form (fec_rs_reconstruct_batch) timed beside."""

    def __init__(self, fec, codec, batch):
        self.fec, self.codec, self.b = fec, codec, batch

    def encode(self):
        b = self.b
        self.codec.rs_encode_raw(b.k, b.m, SHARD_LEN, b.B, b.data.data_ptr(), b.k * SHARD_STRIDE,
                                 b.parity.data_ptr(), b.m * SHARD_STRIDE, SHARD_STRIDE, self.fec.FEC_DEVICE)

    def decode(self):
        b = self.b
        rc = self.codec.rs_recover_raw(b.k, b.m, SHARD_LEN, b.B, b.data.data_ptr(), b.k * SHARD_STRIDE,
                                       b.parity.data_ptr(), b.m * SHARD_STRIDE, SHARD_STRIDE, b.masks.data_ptr(),
                                       b.recovered.data_ptr(), SHARD_STRIDE, 1, None)
        if rc != 0:
            raise self.fec.FecError(rc, "decode")

    def decode_inplace(self):
        b = self.b
        rc = self.codec.rs_reconstruct_raw(b.k, b.m, SHARD_LEN, b.B, b.data.data_ptr(), b.k * SHARD_STRIDE,
                                           b.parity.data_ptr(), b.m * SHARD_STRIDE, SHARD_STRIDE,
                                           b.masks.data_ptr(), None, self.fec.FEC_DEVICE)
        if rc != 0:
            raise self.fec.FecError(rc, "decode_inplace")

    def check_full(self, torch):
        """Outside the timed region: every recovered shard equals the erased original; then
        wipe every erased shard, rebuild in place, compare the whole batch."""
        b = self.b
        rows = torch.arange(b.B, device=b.data.device)
        er = b.erased.long()
        ok = bool(torch.equal(b.recovered[:, 0, :SHARD_LEN], b.data[rows, er, :SHARD_LEN]))
        ref = b.data[:, :, :SHARD_LEN].clone()
        b.data[rows, er, :] = 0
        self.decode_inplace()
        self.codec.sync()
        ok = ok and bool(torch.equal(b.data[:, :, :SHARD_LEN], ref))
        del ref
        torch.cuda.empty_cache()
        return ok


def host_threads():
    """Threads for the CPU baseline: OMP_NUM_THREADS if set (16 on the GPU box, its CPU
    share), else the CPUs this process may run on."""
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit() and int(env) > 0:
        return int(env)
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def oracle_spot_check(k, m, sample):
    """cpu_baseline leg, the checker half: the parity of 64 blocks the device encoded equals the
    CPU oracle's (oracle/oracle.py, the reference's buildMatrix and mulTable restated). None when
    the oracle cannot run (never a truthy string)."""
    try:
        import numpy as np
        from oracle import oracle as orc
        want = sample[:, :, :SHARD_LEN].copy()
        orc.rs_encode(k, m, want)
        return bool(np.array_equal(sample[:, :, :SHARD_LEN], want))
    except Exception as exc:  # oracle unavailable: report, do not hide
        print("bench.py: oracle spot-check not run: %s" % exc, file=sys.stderr, flush=True)
        return None


def cpu_baseline(k, m, blocks, seed, budget_s=12.0):
    """The CPU restatement of klauspost's kernels (oracle/fec_simd.c: AVX2 PSHUFB nibble tables,
    GFNI affine forms; the method the reference's calls at reed_solomon.go:51,124 run on x86),
    OpenMP over the host's cores, on a bounded sample of the same workload: encode + single-
    erasure ReconstructData of `blocks` blocks. Every ISA the host supports is tried and the
    fastest reported (the baseline most favourable to the CPU); the scalar mulTable form of the
    pure-Go path (fec_oracle.c) is reported beside it."""
    import numpy as np
    from oracle import oracle as orc
    orc.build()
    n = k + m
    rng = np.random.default_rng(seed)
    sh = np.zeros((blocks, n, SHARD_LEN), dtype=np.uint8)
    sh[:, :k, :PAYLOAD] = rng.integers(0, 256, (blocks, k, PAYLOAD), dtype=np.uint8)
    sh[:, :k, PAYLOAD] = PAYLOAD >> 8
    sh[:, :k, PAYLOAD + 1] = PAYLOAD & 0xFF
    erased = rng.integers(0, k, blocks)
    masks = (((1 << n) - 1) & ~(1 << erased)).astype(np.uint32)
    threads = host_threads()
    gib = blocks * k * PAYLOAD / 2**30

    def rate(isa, reps_max, seconds):
        orc.rs_encode_simd(k, m, sh, isa, threads=threads)    # warm (page in, OpenMP pool)
        reps, t = 0, 0.0
        while (reps == 0 or t < seconds) and reps < reps_max:
            t0 = time.perf_counter()
            orc.rs_encode_simd(k, m, sh, isa, threads=threads)
            orc.rs_reconstruct_simd(k, m, sh, masks, isa, threads=threads)
            t += time.perf_counter() - t0
            reps += 1
        return reps * gib / t, reps

    isas = [i for i in (orc.ISA_AVX2, orc.ISA_GFNI_AVX2, orc.ISA_GFNI_AVX512) if orc.isa_supported(i)]
    trial = {i: rate(i, 2, 0.0)[0] for i in isas}
    best = max(trial, key=trial.get) if trial else orc.ISA_SCALAR
    value, reps = rate(best, 200, budget_s)
    scalar, sreps = rate(orc.ISA_SCALAR, 3, 0.0)

    def one_core(kk, mm, nb=4096):
        """One thread's per-block time (us) for encode and single-erasure ReconstructData, the
        fastest ISA, amortised over nb blocks: what one connection's run loop would spend coding
        a block itself (the yardstick of the receive-side burst stall)."""
        nn = kk + mm
        s1 = np.zeros((nb, nn, SHARD_LEN), dtype=np.uint8)
        s1[:, :kk] = rng.integers(0, 256, (nb, kk, SHARD_LEN), dtype=np.uint8)
        m1 = np.full(nb, ((1 << nn) - 1) & ~1, dtype=np.uint32)
        out = None
        for isa in isas or [orc.ISA_SCALAR]:
            orc.rs_encode_simd(kk, mm, s1, isa, threads=1)
            te, td = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                orc.rs_encode_simd(kk, mm, s1, isa, threads=1)
                t1 = time.perf_counter()
                orc.rs_reconstruct_simd(kk, mm, s1, m1, isa, threads=1)
                te.append(t1 - t0)
                td.append(time.perf_counter() - t1)
            cand = (min(te) / nb * 1e6, min(td) / nb * 1e6, orc.isa_name(isa))
            if out is None or cand[0] + cand[1] < out[0] + out[1]:
                out = cand
        return {"encode_us": round(out[0], 3), "reconstruct_1_erasure_us": round(out[1], 3), "isa": out[2]}

    return {"value": round(value, 3), "unit": "GiB/s", "cores": threads, "kind": "port",
            "single_core": {"RS(%d,%d)" % (kk, kk + mm): one_core(kk, mm) for kk, mm in ((k, m), (20, 10))},
            "isa": orc.isa_name(best),
            "sample": "%d reps x %d blocks RS(%d,%d) 1202-B shards, encode + 1-erasure ReconstructData, "
                      "oracle/fec_simd.c (klauspost kernel method restated, bit-exact vs the scalar oracle), "
                      "OpenMP %d threads; fastest of %s" % (reps, blocks, k, n, threads,
                                                           ", ".join(orc.isa_name(i) for i in isas)),
            "scalar_value": round(scalar, 3),
            "scalar_sample": "%d reps, pure-Go mulTable form (oracle/fec_oracle.c)" % sreps}


def host_resident(torch, fec, codec, k, m, blocks, seed, reps=6):
    """The path as the reference runs it, from host packet buffers to host packet buffers:
    fec_rs_encode_batch + single-erasure fec_rs_reconstruct_batch on host memory, PCIe copies
    included (pinned hipMemcpyAsync on three streams, three staging sets overlapping chunks); the
    best of `reps` steps, each ~50-60 ms (a shared host's CPU share comes and goes). Two forms: buffers the
    caller pinned (FEC_HOST_PINNED: direct 2D DMA) and pageable buffers (FEC_HOST: staged by the
    library). Packed host layout, stride = shard length. Reported beside the device-resident
    value, never as it."""
    import numpy as np
    n, L = k + m, SHARD_LEN
    shard = importlib.import_module("0xfec_amd.shard")
    rng = np.random.default_rng(seed)
    src = np.zeros((blocks, k, L), dtype=np.uint8)
    src[:, :, :PAYLOAD] = rng.integers(0, 256, (blocks, k, PAYLOAD), dtype=np.uint8)
    src[:, :, PAYLOAD] = PAYLOAD >> 8
    src[:, :, PAYLOAD + 1] = PAYLOAD & 0xFF
    erased = shard.synth_single_erasures(seed, 0, blocks, k)
    masks = (((1 << n) - 1) & ~(1 << erased)).astype(np.uint32)
    # PCIe bytes of a step: encode k up + m down; reconstruct the k data shards up (one linear DMA
    # of the span), the one parity plane each block reads (pageable: staged by the host; pinned:
    # one 2D DMA of the plane, which every block reads here), the rebuilt shard down
    up_bytes, down_bytes = blocks * (k + k + 1) * L, blocks * (m + 1) * L
    # the link as the host path drives it (include/fec_probe.h fec_probe_link: pinned hipMemcpyAsync,
    # H2D, D2H, both at once on two streams; tools/pcie_duplex_probe.hip measures more shapes)
    link = codec.probe_link()
    # the link's bound for the step: while both directions run, each at the duplex rate; the rest
    # of the up direction (the larger one) alone at the H2D rate
    both = min(up_bytes, down_bytes)
    bound_s = both / (link["duplex_each_GBps"] * 1e9) + (up_bytes - both) / (link["h2d_GBps"] * 1e9) \
        + (down_bytes - both) / (link["d2h_GBps"] * 1e9)
    out = {"blocks": blocks, "layout": "packed host [B][k][1202] + [B][m][1202]",
           "pcie_bytes_per_step": up_bytes + down_bytes, "pcie_up_bytes": up_bytes, "pcie_down_bytes": down_bytes,
           "pcie_bytes_note": "up k+k+1 shards per block (encode data; reconstruct data span + the parity plane each "
                              "block reads), down m+1 (parity; the rebuilt shard), in both forms",
           "link_probe": link, "link_bound_ms": round(bound_s * 1e3, 2),
           "link_bound_GiBps": round(blocks * k * PAYLOAD / 2**30 / bound_s, 2)}
    for form in ("pinned", "pageable"):
        if form == "pinned":
            data = torch.from_numpy(src.copy()).pin_memory()
            par = torch.zeros((blocks, m, L), dtype=torch.uint8).pin_memory()
            dnp, pnp = data.numpy(), par.numpy()
            flags, dp, pp = fec.FEC_HOST_PINNED, data.data_ptr(), par.data_ptr()
        else:
            dnp, pnp = src.copy(), np.zeros((blocks, m, L), dtype=np.uint8)
            flags, dp, pp = fec.FEC_HOST, dnp.ctypes.data, pnp.ctypes.data
        rows = np.arange(blocks)

        def step():
            codec.rs_encode_raw(k, m, L, blocks, dp, k * L, pp, m * L, L, flags)
            rc = codec.rs_reconstruct_raw(k, m, L, blocks, dp, k * L, pp, m * L, L, masks.ctypes.data, None, flags)
            if rc:
                raise fec.FecError(rc, "host reconstruct")

        codec.rs_encode_raw(k, m, L, blocks, dp, k * L, pp, m * L, L, flags)
        dnp[rows, erased] = 0                       # the erased shards, wiped once (checked below)
        rc = codec.rs_reconstruct_raw(k, m, L, blocks, dp, k * L, pp, m * L, L, masks.ctypes.data, None, flags)
        ok = rc == 0 and bool(np.array_equal(dnp, src))
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            step()
            t.append(time.perf_counter() - t0)
        best = min(t)
        out[form] = {"value": round(blocks * k * PAYLOAD / 2**30 / best, 2), "unit": "GiB/s",
                     "ms_per_step": round(best * 1e3, 2), "pcie_GBps": round(out["pcie_bytes_per_step"] / best / 1e9, 2),
                     "up_GBps": round(up_bytes / best / 1e9, 2), "down_GBps": round(down_bytes / best / 1e9, 2),
                     "frac_of_probe": round(bound_s / best, 4),
                     "check": ok and bool(np.array_equal(pnp[:64], device_parity(torch, fec, codec, k, m, src[:64])))}
    return out


def timed_bursts(torch, stream, fn, bursts=3, min_burst_ms=6.0):
    """ms per launch of fn: the median over `bursts` bursts of back-to-back launches, each burst
    at least min_burst_ms long (a 40-us RS(2,3) launch timed in bursts of 3 sees launch gaps)."""
    def one(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    burst = max(3, int(min_burst_ms / max(one(1), 1e-3)) + 1)
    return sorted(one(burst) for _ in range(bursts))[bursts // 2]


def best_twin(torch, stream, twin, nbytes, offsets=TWIN_OFFSETS, wpcs=TWIN_WPC):
    """The box's ceiling for an access shape: twin(wpc, off) (a traffic twin at `wpc` resident
    workgroups per CU, output `off` bytes into its buffer) timed at every residency and output
    offset; returns the best TB/s with its (wpc, off) and every rate measured."""
    rates, fns = {}, {}
    for off in offsets:
        for w in wpcs:
            key = "wpc%d off%d" % (w, off)
            fns[key] = lambda w=w, off=off: twin(w, off)
            fns[key]()
            rates[key] = round(nbytes / timed_bursts(torch, stream, fns[key]) / 1e9, 3)
    best = max(rates, key=rates.get)
    best0 = max((kk for kk in rates if kk.endswith(" off0")), key=rates.get)
    # the max over the sweep's noisy medians reads high: the winner (and the best at offset 0, the
    # kernels' own output placement) are timed again in fresh interleaved bursts, and those rates
    # are the ones reported
    again = {kk: [] for kk in dict.fromkeys((best, best0))}
    for _ in range(3):
        for kk in again:
            again[kk].append(timed_bursts(torch, stream, fns[kk]))
    re_rate = {kk: round(nbytes / sorted(v)[1] / 1e9, 3) for kk, v in again.items()}
    return {"probe_best_TBps": re_rate[best], "probe_best_at": best, "probe_best_off0_TBps": re_rate[best0],
            "probe_best_off0_at": best0, "sweep_TBps": rates,
            "sweep_note": "probe_best_* re-timed after the sweep in 3 interleaved rounds (median); sweep_TBps "
                          "holds each setting's first median"}


def box_probe(torch, codec, b, step, stream, enc_bytes, dec_bytes, rounds=5, burst=4):
    """Times the traffic twin of the encode and of the direct decode (fec_probe.hip: the same bytes,
    launch shape, residency and cache policy, no field arithmetic) in bursts interleaved with bursts
    of the kernels themselves. Returns per kernel the twin's TB/s at the kernel's own residency
    (the same-shape figure), the kernel's TB/s in the same interleaved bursts, and their ratio; then
    each twin's best over residency and output placement (probe_best_TBps, best_twin), and the
    shape-independent reference: the block's k data shards read whole plus one store per block
    (fec_probe_stream_traffic), at its best residency."""
    L, S = SHARD_LEN, SHARD_STRIDE

    def enc_twin(wpc=-1, off=0):
        codec.probe_encode_traffic_raw(b.k, b.m, L, b.B, b.data.data_ptr(), b.k * S, b.parity.data_ptr() + off,
                                       b.m * S, S, wpc)

    def dec_twin(wpc=-1, off=0):
        codec.probe_recover_traffic_raw(b.k, b.m, L, b.B, b.data.data_ptr(), b.k * S, b.parity.data_ptr(), b.m * S, S,
                                        b.masks.data_ptr(), b.recovered.data_ptr() + off, S, wpc)

    def stream_ref(wpc=0, off=0):
        codec.probe_stream_traffic_raw(b.k, L, b.B, b.data.data_ptr(), b.k * S, b.recovered.data_ptr() + off, S, S,
                                       wpc)

    def timed_burst(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(burst):
            fn()
        e1.record(stream)
        return e0, e1

    out = {}
    for name, twin, kern, nbytes in (("encode", enc_twin, step.encode, enc_bytes),
                                     ("decode", dec_twin, step.decode, dec_bytes)):
        twin()
        kern()
        ev = []
        for _ in range(rounds):   # twin first: the kernel then rewrites what the twin wrote
            ev.append((timed_burst(twin), timed_burst(kern)))
        codec.sync()
        tw = sum(a[0].elapsed_time(a[1]) for a, _ in ev) / (rounds * burst)
        kt = sum(c[0].elapsed_time(c[1]) for _, c in ev) / (rounds * burst)
        out[name] = {"probe_ms": round(tw, 4), "probe_TBps": round(nbytes / tw / 1e9, 3),
                     "kernel_ms_interleaved": round(kt, 4), "kernel_TBps_interleaved": round(nbytes / kt / 1e9, 3),
                     "kernel_frac_of_probe_interleaved": round(tw / kt, 4)}
        out[name].update(best_twin(torch, stream, twin, nbytes))
        if out[name]["probe_TBps"] > out[name]["probe_best_TBps"]:   # the interleaved same-shape run won
            out[name]["probe_best_TBps"] = out[name]["probe_TBps"]
            out[name]["probe_best_at"] = "own residency, interleaved with the kernel"
    # the reference moves k reads + 1 write per block, as the decode does
    out["stream_reference"] = {"shape": "%d contiguous data shards read + 1 store per block" % b.k,
                               **best_twin(torch, stream, stream_ref, dec_bytes)}
    return out


def device_parity(torch, fec, codec, k, m, data):
    """Parity of host data blocks [B, k, L] by the device-resident encode (FEC_DEVICE, the kernel
    the oracle checks in tests/ and in the cpu_baseline leg): the host-resident forms must give
    the same bytes."""
    b, _, ln = data.shape
    st = (ln + 15) // 16 * 16
    d = torch.zeros((b, k, st), dtype=torch.uint8, device="cuda")
    d[:, :, :ln] = torch.from_numpy(data).cuda()
    p = torch.zeros((b, m, st), dtype=torch.uint8, device="cuda")
    codec.rs_encode_raw(k, m, ln, b, d.data_ptr(), k * st, p.data_ptr(), m * st, st, fec.FEC_DEVICE)
    codec.sync()
    return p[:, :, :ln].cpu().numpy()


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(args):
    """--gpus N > 1 without a torchrun environment: run torchrun with N ranks as a child process
    (this process has not touched the GPU: torch.cuda.device_count() does not initialise it on
    this image) and return its exit status. Rank 0 prints the JSON line."""
    import subprocess
    import torch
    have = torch.cuda.device_count()
    if args.gpus > have and not args.rehearse_one_gpu:
        print("bench.py: --gpus %d requested but only %d HIP device(s) are visible; refusing to report "
              "a smaller run as an %d-GPU number" % (args.gpus, have, args.gpus), file=sys.stderr, flush=True)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def main():
    args = parse()
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        sys.exit(launch_ranks(args))
    if world_env is not None and int(world_env) != args.gpus:
        print("bench.py: WORLD_SIZE=%s but --gpus %d; refusing to mislabel the run" % (world_env, args.gpus),
              file=sys.stderr, flush=True)
        sys.exit(2)
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.rehearse_one_gpu:
        local = 0
    # under torchrun the process group is always formed, a single rank included: then
    # `torchrun --nproc-per-node 1 bench.py` runs the RCCL init, barriers and reductions of the
    # N-GPU path on a one-GPU box
    distributed = world_env is not None
    if distributed:
        if args.rehearse_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    fec = importlib.import_module("0xfec_amd")

    shard = importlib.import_module("0xfec_amd.shard")
    k, m, B = args.k, args.m, args.blocks
    n = k + m
    g_lo, g_hi = shard.block_range(B * world, rank, world)   # this rank's slice of the global batch
    codec = fec.Codec(local)
    codec.prepare(k, m)
    codec.use_torch_stream()
    stream = torch.cuda.current_stream(dev)

    batch = RankBatch(torch, codec, dev, B, k, m, args.seed, g_lo)
    step = RankStep(fec, codec, batch)
    encode, decode, decode_inplace = step.encode, step.decode, step.decode_inplace
    full = args.full
    ok_roundtrip = None
    if full:
        encode()
        decode()
        codec.sync()
        ok_roundtrip = step.check_full(torch)

    for _ in range(args.warmup):
        encode()
        decode()
    codec.sync()

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True),
           torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record(stream)
        encode()
        ev[i][1].record(stream)
        decode()
        ev[i][2].record(stream)
    codec.sync()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    wall = time.perf_counter() - t0
    enc_ms = sum(e[0].elapsed_time(e[1]) for e in ev) / args.steps
    dec_ms = sum(e[1].elapsed_time(e[2]) for e in ev) / args.steps
    step_ms = wall * 1000.0 / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(torch, batch, args.dump_outputs, args.seed)
    inplace_ms = 0.0
    if full:
        # in-place reconstruct, timed on its own (not part of the step)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(3, args.steps // 2)
        e0.record(stream)
        for _ in range(reps):
            decode_inplace()
        e1.record(stream)
        codec.sync()
        inplace_ms = e0.elapsed_time(e1) / reps
    rank_step_ms = [step_ms]
    ranks_seen = 1
    if distributed:
        rdev = "cpu" if args.rehearse_one_gpu else dev   # gloo reduces host tensors
        ranks_seen = dist.get_world_size()
        per = [torch.zeros(1, device=rdev, dtype=torch.float64) for _ in range(ranks_seen)]
        dist.all_gather(per, torch.tensor([step_ms], device=rdev, dtype=torch.float64))
        rank_step_ms = [float(x.item()) for x in per]
        t = torch.tensor([step_ms, enc_ms, dec_ms, inplace_ms], device=rdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        step_ms, enc_ms, dec_ms, inplace_ms = t.tolist()
        if full:
            okt = torch.tensor([1 if ok_roundtrip else 0], device=rdev)
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            ok_roundtrip = bool(okt.item())

    L = SHARD_LEN
    enc_bytes = B * (k + m) * L                  # read k shards, write m shards
    dec_bytes = B * (k + 1) * L                  # read first k present, write 1 erased data shard
    value = shard.aggregate_gibps([B] * world, k, PAYLOAD, step_ms / 1000.0)
    enc_bw = enc_bytes / (enc_ms / 1000.0)
    dec_bw = dec_bytes / (dec_ms / 1000.0)

    # what both forms of the result line share: the headline figure and its workload
    head = {
        "metric": "device-resident FEC encode+decode GiB/s, 1200B symbols, RS k=%d n=%d" % (k, n),
        "value": round(value, 2),
        "unit": "GiB/s",
        "n_gpus": world,
        "ranks_seen": ranks_seen,
        "rank_ms_per_step": [round(x, 4) for x in rank_step_ms],
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(step_ms, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "full": full,
        "outputs_dumped": args.dump_outputs,
        "data": "synthetic: splitmix64 bytes keyed by (seed 0x%04X, global block, shard, word), "
                "generated in HBM (include/fec_synth.h, BASELINE.md 2)" % args.seed,
        "config": {"workload": "RS(k=%d,n=%d) encode + random single-data-erasure decode" % (k, n),
                   "blocks_per_gpu": B, "payload_bytes": PAYLOAD, "shard_len": L,
                   "shard_stride": SHARD_STRIDE, "layout": "data [B][k][1216] + parity [B][m][1216] buffers",
                   "parallelism": "independent block ranges per GPU",
                   "rehearsal": bool(args.rehearse_one_gpu and world > 1)},
    }
    if not full:
        # the plain line: the headline figure and what the timed steps' own events say, nothing
        # that takes a run of its own
        if rank == 0:
            head["kernels"] = {
                "encode": {"ms": round(enc_ms, 4), "GB/s": round(enc_bw / 1e9, 1), "bytes": enc_bytes,
                           "frac": round(enc_bw / HBM_PEAK, 4)},
                "decode": {"ms": round(dec_ms, 4), "GB/s": round(dec_bw / 1e9, 1), "bytes": dec_bytes,
                           "frac": round(dec_bw / HBM_PEAK, 4)},
                "step_frac": round((enc_bytes + dec_bytes) / ((enc_ms + dec_ms) / 1000.0) / HBM_PEAK, 4)}
            head["note"] = "plain run: checks, roofline, traffic twins, host-resident path and CPU baseline need --full"
            print(json.dumps(head), flush=True)
        codec.close()
        if distributed:
            dist.destroy_process_group()
        return

    # 64 random blocks (data + parity) for the oracle spot-check, which runs in the cpu_baseline
    # leg (N = 1, rank 0): the only part of bench.py that touches oracle/. Otherwise None (not
    # run), with the reason beside it
    ok_parity = None
    parity_sample = None
    if rank == 0:
        pick = torch.randperm(B, device=dev)[:64]
        parity_sample = torch.cat([batch.data[pick], batch.parity[pick]], dim=1).cpu().numpy()

    # this box's ceiling for each kernel's access shape, after the checks (the twins overwrite the
    # parity and recovered buffers): traffic twins (include/fec_probe.h), interleaved with the
    # kernels themselves so both see the same box state
    probe = box_probe(torch, codec, batch, step, stream, enc_bytes, dec_bytes)
    enc_kernel = encode_kernel_name(k, m)
    if enc_ms >= dec_ms:
        dom_name = "encode"
        dominant, dom_bw, dom_bytes = enc_kernel + ">", enc_bw, enc_bytes
        traffic, traffic_src = committed_traffic(enc_kernel, "fec_encode.hip")
    else:
        dom_name = "decode"
        dominant, dom_bw, dom_bytes = "rs_recover_direct_kernel<%d" % k, dec_bw, dec_bytes
        traffic, traffic_src = committed_traffic("rs_recover_direct_kernel", "fec_recover.hip")
    if traffic_src.get("kernel"):   # the instance the profile names (store policy in its template list)
        dominant = traffic_src["kernel"].replace("void fk::", "").split("(")[0]

    if rank == 0:
        out = {
            **head,
            "roofline": {"bound": "hbm", "achieved": round(dom_bw / 1e9, 1), "peak": HBM_PEAK / 1e9,
                         "unit": "GB/s", "frac": round(dom_bw / HBM_PEAK, 4),
                         "traffic": None if traffic is None else round(traffic / 1e9, 3),
                         "traffic_unit": "GB per launch", "traffic_profile": traffic_src,
                         "kernel": dominant, "algorithmic_bytes_per_launch": dom_bytes,
                         # the kernel's traffic twin at the kernel's own residency (same shape) and
                         # its best over residency and placement (this box's ceiling for the shape),
                         # with the timed-region rate over each
                         "probe_TBps": probe[dom_name]["probe_TBps"],
                         "frac_of_probe": round(dom_bw / 1e12 / probe[dom_name]["probe_TBps"], 4),
                         "probe_best_TBps": probe[dom_name]["probe_best_TBps"],
                         "frac_of_probe_best": round(dom_bw / 1e12 / probe[dom_name]["probe_best_TBps"], 4),
                         "probe_kernel": "fec_probe.hip probe_%s_kernel (include/fec_probe.h)" % (
                             "encode" if dom_name == "encode" else "recover")},
            "kernels": {
                # read_frac: the HBM-read roofline of SURVEY.md 8(d) (reads alone: k shards per block)
                "encode": {"ms": round(enc_ms, 4), "GB/s": round(enc_bw / 1e9, 1), "bytes": enc_bytes,
                           "frac": round(enc_bw / HBM_PEAK, 4),
                           "read_frac": round(B * k * L / (enc_ms / 1000.0) / HBM_PEAK, 4),
                           "frac_of_probe": round(enc_bw / 1e12 / probe["encode"]["probe_TBps"], 4),
                           "frac_of_probe_best": round(enc_bw / 1e12 / probe["encode"]["probe_best_TBps"], 4),
                           "probe": probe["encode"]},
                "decode": {"ms": round(dec_ms, 4), "GB/s": round(dec_bw / 1e9, 1), "bytes": dec_bytes,
                           "frac": round(dec_bw / HBM_PEAK, 4),
                           "read_frac": round(B * k * L / (dec_ms / 1000.0) / HBM_PEAK, 4),
                           "api": "fec_rs_recover_batch (direct single-erasure kernel, no plan launch)",
                           "frac_of_probe": round(dec_bw / 1e12 / probe["decode"]["probe_TBps"], 4),
                           "frac_of_probe_best": round(dec_bw / 1e12 / probe["decode"]["probe_best_TBps"], 4),
                           "probe": probe["decode"]},
                "stream_reference": probe["stream_reference"],
                "decode_inplace": {"ms": round(inplace_ms, 4),
                                   "GB/s": round(dec_bytes / (inplace_ms / 1e3) / 1e9, 1),
                                   "api": "fec_rs_reconstruct_batch in place, not in the step: classify pass (one "
                                          "word: does a block need a multi-erasure plan?), then rs_reconstruct_routed_kernel, "
                                          "which on this single-erasure batch runs the direct body on three waves of each "
                                          "workgroup (the sorted plan kernel exits at once)"},
                "step_frac": round((enc_bytes + dec_bytes) / ((enc_ms + dec_ms) / 1000.0) / HBM_PEAK, 4),
            },
            "check": {"roundtrip_full_batch": ok_roundtrip, "encode_vs_oracle_64_blocks": ok_parity,
                      "encode_vs_oracle_note": "run in the N = 1 cpu_baseline leg only (the one part of bench.py "
                                               "that may touch oracle/); the round trip checks every block"},
        }
        if world == 1 and args.host_blocks > 0:
            del batch, step, encode, decode, decode_inplace   # free the device batch first
            torch.cuda.empty_cache()
            out["host_resident"] = host_resident(torch, fec, codec, k, m, args.host_blocks, args.seed)
        if world == 1 and not args.no_cpu_baseline:
            out["check"]["encode_vs_oracle_64_blocks"] = oracle_spot_check(k, m, parity_sample)
            out["cpu_baseline"] = cpu_baseline(k, m, args.cpu_sample_blocks, args.seed)
        print(json.dumps(out), flush=True)
    codec.close()
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
