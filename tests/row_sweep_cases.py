"""The cases of test_gpu_row_sweep.py, built on the host: one sweep of every parity-row count through the
calls that share the generic fold body (verify, update / encode-idx, locate, the locate-multi and
locate-partial scans, the generic encode and the ragged encode). test_gpu_row_sweep.py runs them on the
device; test_row_sweep_cases.py builds every one without a device and asserts what the device tests rest
on: that every compiled instance of the seven launchers gets a pass at its top row count and at its
bottom one, first and later passes alike.

Codes. The row sweep is m = 1 .. 33 with k = KS[m % 8]: every row count 1 .. 16 as a first pass, as a
second pass (m = 17 .. 32) and once as a third (m = 33); none of them a code with an encode kernel of
its own, so the plain encode call takes the generic launcher. The input sweep is k = 1 .. 17 at m = 3
and m = 6: every k mod 8 (fold_group takes inputs eight at a time, in pairs, a single one for an odd
tail), k below, at and above one and two input groups, under the 4- and 8-row instances with a
predicated row. The table edge: (128,16) has 2048 tables, the last code whose tables stay in LDS,
(129,16) the first that reads them from memory, (129,17) follows a memory pass with an LDS pass of one
row, and (130,33), for locate alone, has three passes whose later two read carry slabs 0 and 1.
Locate-multi and locate-partial take codes of at most 16 rows: the row sweep cut there, the input sweep,
the first two table-edge codes, and for m <= 11 the code (12 - m, m) of 12 shards, the largest the
siblings' brute-force model takes, so the radii T = 1 .. 5 are checked against the definition
(T = 6, 7, 8 rest on the theorem, as (4,16) does in test_gpu_locate_multi.py).

Shapes. 67 blocks of 33 bytes for every flat call, the siblings' smallest: three chunks with a one-byte
tail, 201 items, so waves straddle blocks and the last wave is partly dead. The ragged encode takes two
cycles of test_gpu_ragged.py's 14 lengths. One device layout per code, alternating over the codes.

Parity. Every batch that starts from an encoded image takes its parity from oracle.rs_encode
(arena.oracle_arena), never from the device.

No code's B is cut: the slowest host model (the brute force of (2,10), T = 5) builds in about a second.
"""
import functools
import os
import re

import numpy as np

import test_gpu_locate as lo
import test_gpu_locate_multi as lm
import test_gpu_locate_partial as lp
import test_gpu_ragged as rag
import test_gpu_update as up
import test_gpu_verify as vr
from arena import CANARY, oracle_arena, rup16

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "0xfec_amd", "csrc")

L, B = 33, 67
RAGGED_NB = 28
KS = [3, 5, 9, 11, 13, 7, 10, 12]
ROW_SWEEP = [(KS[m % 8], m) for m in range(1, 34)]
INPUT_SWEEP = [(k, m) for m in (3, 6) for k in range(1, 18)]
TABLE_EDGE = [(128, 16), (129, 16), (129, 17)]
CARRY_CODE = (130, 33)
FIXED_ENCODES = [(2, 1), (8, 4), (16, 8), (20, 10)]     # fec_encode.hip fixed_encode_applies
BRUTE_CODES = [(12 - m, m) for m in range(1, 12)]

FLAT_CODES = list(dict.fromkeys(ROW_SWEEP + INPUT_SWEEP + TABLE_EDGE))     # (11,3) and (10,6) are in both sweeps
LOCATE_CODES = FLAT_CODES + [CARRY_CODE]
RAGGED_CODES = ROW_SWEEP + TABLE_EDGE
MULTI_CODES = list(dict.fromkeys([c for c in ROW_SWEEP if c[1] <= 16] + INPUT_SWEEP + TABLE_EDGE[:2] + BRUTE_CODES))
# locate-multi a second time, below the radius
MULTI_BELOW = [(k, m, max(1, m // 2 - 1)) for k, m in MULTI_CODES if min(lm.MAX_BAD, m // 2) >= 2]


def layout_of(k, m):
    return vr.LAYOUTS[(k + m) % 2]


def seed_of(k, m):
    return 1000 * k + 10 * m + L


# ------------------------------------------------------------------ the launchers, read from the sources

def source(name):
    return open(os.path.join(CSRC, name)).read()


def constant(name, header):
    got = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, source(header))
    assert got, "%s in %s" % (name, header)
    return int(got.group(1))


def flat_passes(m):
    """(rows, later pass) of every pass of a code of m parity rows through verify, update / encode-idx and
    the two encodes: fec_cores.cpp `for (int r0 = 0; r0 < code->m; r0 += 16)`."""
    return [(min(16, m - r0), r0 > 0) for r0 in range(0, m, 16)]


def locate_passes(m):
    """As flat_passes for locate (fec_cores.cpp locate_launches): row 0 and up to kLocateRows - 1 rows from
    r0 = 1, 16, 31, ...; a code of one parity row passes row 0 alone."""
    R = constant("kLocateRows", "fec_locate.hpp")
    out, r0 = [], 1
    while m > 0 and (r0 == 1 or r0 < m):
        out.append((1 + min(R - 1, m - r0), r0 > 1))
        r0 += R - 1
    return out


def single_pass(m):
    """Locate-multi and locate-partial: one scan over all rows of a code of at most kLocateMultiRows."""
    assert 1 <= m <= constant("kLocateMultiRows", "fec_locate_multi.hpp")
    return [(m, False)]


# name: (source file, launcher, the variable it selects by, passes of a code, its sweep codes, the fewest
# rows a later pass can have)
LAUNCHERS = {
    "update / encode-idx": ("fec_update.hip", "launch_rs_update", "a.m", flat_passes, FLAT_CODES, 1),
    "verify": ("fec_verify.hip", "launch_rs_verify", "a.m", flat_passes, FLAT_CODES, 1),
    "locate": ("fec_locate.hip", "launch_rs_locate", "a.rows", locate_passes, LOCATE_CODES, 2),
    "locate-multi scan": ("fec_locate_multi.hip", "launch_rs_locate_multi_scan", "a.m", single_pass, MULTI_CODES, None),
    "locate-partial scan": ("fec_locate_partial.hip", "launch_rs_locate_partial_scan", "a.m", single_pass, MULTI_CODES,
                            None),
    "encode": ("fec_encode.hip", "launch_rs_encode", "a.m", flat_passes, FLAT_CODES, 1),
    "ragged encode": ("fec_ragged.hip", "launch_rs_encode_ragged", "a.m", flat_passes, RAGGED_CODES, 1),
}
NAMED = {"kLocateRows": "fec_locate.hpp", "kLocateMultiRows": "fec_locate_multi.hpp"}


def instances(name):
    """The row counts a launcher has an instance for, ascending: its lines `if (VAR <= N) return f<N>(`
    and the instance it falls through to."""
    src, fn, var, _, _, _ = LAUNCHERS[name]
    body = re.search(r"^hipError_t %s\([^)]*\) \{\n(.*?)^\}" % fn, source(src), re.S | re.M)
    assert body, "%s in %s" % (fn, src)
    body = body.group(1)
    out = []
    for lim, inst in re.findall(r"^\s*if \(%s <= (\d+)\) return \w+<(\d+)>\(" % re.escape(var), body, re.M):
        assert lim == inst, "%s: rows <= %s go to instance <%s>" % (fn, lim, inst)
        out.append(int(lim))
    last = re.findall(r"^\s*return \w+<(\w+)>\(", body, re.M)
    assert out and len(last) == 1, "%s: the instance lines" % fn
    out.append(int(last[0]) if last[0].isdigit() else constant(last[0], NAMED[last[0]]))
    assert out == sorted(set(out))
    return out


def instance_of(name, rows):
    return next(n for n in instances(name) if rows <= n)


def reached(name, codes):
    """{instance: set of (rows, later pass)} over the passes of `codes` through a launcher."""
    passes = LAUNCHERS[name][3]
    out = {n: set() for n in instances(name)}
    for _, m in codes:
        for rows, later in passes(m) if m else []:
            out[instance_of(name, rows)].add((rows, later))
    return out


def wanted(name):
    """{instance: set of (rows, later pass)} the sweep must hold: every instance <N> whose lower neighbour is
    <P> at N rows and at P + 1 rows, as a first pass and, where the caller cuts a code into passes, as a
    later one (whose row count cannot go below the launcher's fewest: row 0 and one more for locate)."""
    least_later = LAUNCHERS[name][5]
    out, prev = {}, 0
    for n in instances(name):
        out[n] = {(n, False), (prev + 1, False)}
        if least_later is not None:
            out[n] |= {(n, True), (max(prev + 1, least_later), True)}
        prev = n
    return out


def table(name, codes):
    """One line per instance, for reading: `<4>: 3 4 | later 3 4`."""
    got = reached(name, codes)
    lines = []
    for n in sorted(got):
        first = sorted(r for r, later in got[n] if not later)
        later = sorted(r for r, later in got[n] if later)
        lines.append("<%d>: %s | later %s" % (n, " ".join(map(str, first)) or "-", " ".join(map(str, later)) or "-"))
    return lines


# ------------------------------------------------------------------ the batches

def builder(oracle):
    return functools.partial(oracle_arena, oracle)


def encode_case(oracle, k, m):
    """(image before the call, image after it, data region, parity region): the parity slots hold canary
    before, the oracle's parity with a zero pad after."""
    after, data, par = oracle_arena(oracle, layout_of(k, m), k, m, L, B, np.random.default_rng(seed_of(k, m)))
    before = after.copy()
    before[par.index(0, L)] = CANARY
    after[par.index(L, rup16(L))] = 0
    return before, after, data, par


def verify_batch(codec, fec, torch, oracle, k, m):
    return vr.Batch(codec, fec, torch, layout_of(k, m), k, m, L, B, seed_of(k, m), build=builder(oracle))


def update_batch(codec, fec, torch, oracle, k, m, zero_parity=False):
    return up.Batch(codec, fec, torch, oracle, layout_of(k, m), k, m, L, B, seed_of(k, m), zero_parity=zero_parity)


def locate_batch(codec, fec, torch, oracle, gf, k, m):
    return lo.Batch(codec, fec, torch, oracle, gf, layout_of(k, m), k, m, L, B, seed_of(k, m), build=builder(oracle))


def multi_batch(codec, fec, torch, oracle, gf, k, m, max_bad=lm.MAX_BAD):
    return lm.Batch(codec, fec, torch, oracle, gf, layout_of(k, m), k, m, L, B, seed_of(k, m) + max_bad, max_bad=max_bad,
                    build=builder(oracle))


def partial_batch(codec, fec, torch, oracle, gf, k, m):
    return lp.PBatch(codec, fec, torch, oracle, gf, layout_of(k, m), k, m, L, B, 2 * seed_of(k, m),
                     build=builder(oracle))


def partial_max_bads(m):
    """The max_bad values PBatch.run() calls with."""
    return [lp.MAX_BAD, 0] + ([1] if m >= 4 else [])


def ragged_case(oracle, k, m):
    return rag.enc_case(oracle, k, m, RAGGED_NB)
