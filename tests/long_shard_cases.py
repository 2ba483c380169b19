"""The cases of test_gpu_long_shards.py, built on the host: lengths, batch sizes, codes, masks and the
oracle's results. test_gpu_long_shards.py runs them on the device; test_long_shard_cases.py builds every
one without a device and asserts what the device tests rest on.

Lengths. 4099 bytes = 257 chunks of 16 with a 3-byte tail: the smallest shard that leaves one 256-lane
workgroup (in the wide tile its second chunk tile holds one live lane). 69 989 bytes = 4375 chunks
(17 * 256 + 23 = 68 * 64 + 23) with a 5-byte tail: a block spans 18 workgroups and its edge moves 23
lanes from block to block. Batches are tiny, 11 blocks at 4099 and 5 at 69 989: flat grids of
ceil(11 * 257 / 256) = 12 and ceil(5 * 4375 / 256) = 86 workgroups, neither a multiple of 8, so the
XCD order has workgroups on both sides of its full-rounds boundary.
"""
import os
import re

import numpy as np

import test_gpu_layouts as lay
import test_gpu_some as some
import test_gpu_wide as wide
from arena import GUARD, place

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L_SHORT, L_LONG = 4099, 69989
LENS = [L_SHORT, L_LONG]
BATCH = {L_SHORT: 11, L_LONG: 5}
ERASED = 0x5A

NARROW_CODES = [(2, 1), (8, 4), (8, 8), (16, 8), (20, 10), (6, 2), (10, 22), (31, 1)]
NARROW_LONG_CODES = [(2, 1), (8, 4), (20, 10)]        # the codes that also run at 69 989
NARROW_LAYOUTS = ["interleaved_slack", "split_parity_first"]
WIDE_ENCODES = [(5, 20), (130, 20)]
WIDE_B = 3
WIDE_CODES = {L_SHORT: [(8, 4), (20, 10), (40, 20), (128, 128)], L_LONG: [(8, 4), (40, 20)]}
WIDE_BIG_LOSS = {(8, 4): 4, (20, 10): 10, (40, 20): 20, (128, 128): 21}   # data shards the second block loses
WIDE_ARENA_B = 11
SOME_CODES = [(8, 4), (20, 10)]
XOR_KS = [1, 2, 9, 31]
HOST_L, HOST_B, HOST_CHUNK = L_LONG, 9, 2
HOST_CODES = [(8, 4), (20, 10)]
HOST_WIDE = (40, 20, L_SHORT, 3)
CUT_L = 70000


def narrow_case(oracle, k, m, L, single_only=False):
    return lay.rs_case(oracle, k, m, L, BATCH[L], single_only)


def host_case(oracle, k, m):
    return lay.rs_case(oracle, k, m, HOST_L, HOST_B)


def narrow_arena_bytes(layout, k, m, L, B):
    """Bytes of the largest arena run_rs_step makes for a case: the shard arena, or a recover's out arena
    of m slots."""
    data, par = place(layout, k, m, L, B)
    return max(max(data.end(), par.end()), GUARD + B * (m * data.ss + 32)) + GUARD


_enc = {}


def wide_encode_case(oracle, k, m, L):
    """Shards [WIDE_B, k + m, L] with the oracle's parity."""
    if (k, m, L) not in _enc:
        rng = np.random.default_rng(1000 * k + m + L)
        sh = np.zeros((WIDE_B, k + m, L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (WIDE_B, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        sh.setflags(write=False)
        _enc[(k, m, L)] = sh
    return _enc[(k, m, L)]


_wide = {}


def wide_case(oracle, fec, MUL, k, m, L):
    """Three blocks for the wide calls: one data shard lost; WIDE_BIG_LOSS data shards lost (more than
    16, a second row pass, where the code allows); k - 1 shards present. Shards [3, n, round_up(L, 16)],
    zero from L on; `ref` is the reference's in-place reconstruct of the damaged batch: the oracle's for
    codes of at most 32 shards, else the inverse-matrix reference of test_gpu_wide.py."""
    key = (k, m, L)
    if key not in _wide:
        n = k + m
        rng = np.random.default_rng(77000 + 100 * k + m + L)
        es = [1, WIDE_BIG_LOSS[(k, m)]]
        present = [wide.erase_block(rng, k, m, e) for e in es]
        fail = np.ones(n, dtype=bool)
        fail[wide.pick(rng, range(n), m + 1, [int(rng.integers(0, k))] + wide.PREFERRED)] = False
        present = np.array(present + [fail])
        assert present[-1].sum() == k - 1 and not present[-1, :k].all()
        assert list((~present[:, :k]).sum(axis=1))[:2] == es
        sh = wide.encoded(oracle, rng, WIDE_B, k, m, L)
        dmg = wide.damage(sh, present)
        ref = dmg.copy()
        if n <= 32:
            clean = (present * (1 << np.arange(n, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
            masks = rng.integers(0, 1 << 32, (WIDE_B, 2), dtype=np.uint64).astype(np.uint32)   # word 1: garbage
            masks[:, 0] = clean | (masks[:, 0] & np.uint32((0xFFFFFFFF << n) & 0xFFFFFFFF))  # and above bit n
            st_ref = np.where(oracle.rs_reconstruct(k, m, ref, clean, length=L) != 0, -4, 0).astype(np.int32)
            for b in np.flatnonzero(st_ref == 0):   # rebuilt shards carry zero padding to the 16-byte boundary
                ref[b, :k][~present[b, :k], L:] = 0
        else:
            masks = fec.wide_masks(present)
            assert masks.shape == (WIDE_B, fec.mask_words(n))
            st_ref = wide.ref_reconstruct(oracle, MUL, k, m, ref, present, L)
        assert list(st_ref) == [0, 0, -4]
        assert np.array_equal(ref[:2, :k], sh[:2, :k])          # the reference gives back the original data
        assert np.array_equal(ref[2], dmg[2]) and np.array_equal(ref[:, k:], dmg[:, k:])
        c = dict(sh=sh, present=present, masks=masks, dmg=dmg, ref=ref, st_ref=st_ref, es=np.array(es))
        for a in c.values():
            a.setflags(write=False)
        _wide[key] = c
    return _wide[key]


def some_case(oracle, k, m, L):
    return some.rs_case(oracle, k, m, L, BATCH[L])


_subset = {}


def some_subset_case(oracle, k, m, L):
    """(case, want): every block misses two data and two parity shards, the want mask names one of each."""
    if (k, m, L) not in _subset:
        _subset[(k, m, L)] = some.two_of_four_case(oracle, k, m, L, BATCH[L])
    return _subset[(k, m, L)]


_xor = {}


def xor_case(oracle, k, L):
    if (k, L) not in _xor:
        c = lay.xor_case(oracle, np.random.default_rng(31 * L + k), k, L, BATCH[L])
        for a in c.values():
            a.setflags(write=False)
        _xor[(k, L)] = c
    return _xor[(k, L)]


def cut_shape():
    """(blocks per launch, B, chunks per shard, chunks per stream) of the smallest batch of CUT_L-byte
    shards that the launch limit (fec_ctx.hpp kMaxItems items per launch) cuts in two."""
    src = open(os.path.join(ROOT, "0xfec_amd", "csrc", "fec_ctx.hpp")).read()
    lim = re.search(r"kMaxItems\s*=\s*uint64_t\(1\)\s*<<\s*(\d+)\s*;", src)
    assert lim, "the launch limit"
    assert CUT_L % 16 == 0   # overlapping windows: no zero pad may exist
    cps = CUT_L // 16
    per_launch = (1 << int(lim.group(1))) // cps
    B = per_launch + 1
    return per_launch, B, cps, B + cps - 1
