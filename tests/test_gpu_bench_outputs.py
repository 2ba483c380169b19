"""bench.py's plain run and --dump-outputs on a small batch: the result line's contract fields,
and the dumped arrays (float32 / float64 .npy, the outputs of the last timed step): names, shapes,
size, the sampled shards against the whole-batch sums beside them, and the bytes every block
shares (the length trailer and its parity) against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
BLOCKS, STEPS = 4096, 3


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench_dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                        "--blocks", str(BLOCKS), "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


def test_plain_line_has_the_contract_fields(run):
    line, _ = run
    assert line["metric"].startswith("device-resident FEC encode+decode GiB/s")
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == STEPS and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value is the payload rate of the timed steps: B * k * 1200 bytes per ms_per_step
    want = BLOCKS * 8 * 1200 / 2**30 / (line["ms_per_step"] / 1e3)
    assert abs(line["value"] - want) <= 1e-3 * want + 0.01
    for moved in ("roofline", "check", "host_resident", "cpu_baseline"):
        assert moved not in line


def test_dumped_outputs(run, oracle):
    _, out = run
    arrs = {f[:-4]: np.load(os.path.join(str(out), f)) for f in sorted(os.listdir(str(out)))}
    assert set(arrs) == {"parity", "recovered", "sample_blocks", "parity_block_sums", "recovered_block_sums"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64e6
    n = min(BLOCKS, 1024)
    assert arrs["parity"].shape == (n, 4, 1202) and arrs["recovered"].shape == (n, 1202)
    pick = arrs["sample_blocks"].astype(np.int64)
    assert pick.shape == (n,) and np.all(np.diff(pick) > 0) and pick[-1] < BLOCKS
    assert arrs["parity_block_sums"].shape == (BLOCKS,) and arrs["recovered_block_sums"].shape == (BLOCKS,)
    # the sampled shards and the whole-batch sums describe the same buffers
    assert np.array_equal(arrs["parity"].sum(axis=(1, 2), dtype=np.float64), arrs["parity_block_sums"][pick])
    assert np.array_equal(arrs["recovered"].sum(axis=1, dtype=np.float64), arrs["recovered_block_sums"][pick])
    # every shard is framed: 1200 payload bytes, then the big-endian length 1200 (0x04B0); the
    # parity of the two trailer bytes is the code applied to them, the same in every block
    assert np.all(arrs["recovered"][:, 1200] == 0x04) and np.all(arrs["recovered"][:, 1201] == 0xB0)
    trailer = np.zeros((1, 12, 2), dtype=np.uint8)
    trailer[0, :8] = (0x04, 0xB0)
    oracle.rs_encode(8, 4, trailer)
    assert np.all(arrs["parity"][:, :, 1200:] == trailer[0, 8:])
    assert arrs["recovered"][:, :1200].std() > 50      # random payload bytes, not a cleared buffer
