"""Layouts and cases of the far-offset device tests (test_gpu_far_offsets.py): every device entry point
of include/fec_hip.h on batches whose byte offsets do not fit 32 bits. No device is needed here;
test_far_cases.py checks this module on the CPU.

The arena is 11.85 GiB of canary bytes on the device (far_arena.py; RS(8,12) alone would need 6.0 GiB
for far_blocks and 10.0 GiB for the other families, (10,22) on far_shards sets the figure); a case's
five blocks occupy a few KB of it, in regions placed by one of four families:

  far_blocks        the bases a few KB apart, every block stride 2^30 + 16*4099: block 2 lies past
                    2^31 and block 4 past 2^32 (stresses b * block_stride of every region)
  far_parity_above  small block strides; parity at data + 2^32 + 16*777, the third region (a recover's
                    out, the update's old data) at data + 2^31 + 16*333 (stresses the distances between
                    regions: data-relative parity offsets, the store-policy hulls)
  far_parity_below  the same with parity lowest and the data more than 4 GiB above it (the wrapped
                    negative distance, parity_base's k strides below the parity pointer)
  far_shards        shard-major: block stride rup16(L) + 16, shard stride just large enough for the
                    first parity shard to lie past 2^32 (RS(8,12): 2^29 + 16*257, shard 4 past 2^31 and
                    shard 8 past 2^32), always below 2^32 (stresses j * shard_stride). A code whose
                    k + m shards would not fit the arena at that stride takes the largest stride that
                    fits (a later shard is then the first past 2^32: for (10,22) shard 13, parity
                    shard 3; block 4 of its cases loses parity shards 0..16, so its decode reads
                    parity shards 17..21). A third region lies in the gaps
                    of the data region's strides, shard-major too. The wide (40,20) case takes the
                    stride 2^26 + 16*257: none of its 60 shards reaches 2^32, shard 32 passes 2^31, so
                    it can expose a sign extension only (stress kind "sign" below); the same case runs
                    once more at the stride that puts shard 40 past 2^32 (opt "past4g").

THE RULE. A 32-bit mistake must show as wrong bytes, never as a memory fault. Take every base pointer
P a call is given (data, parity, out, old) and every shard-slot address A it may touch through any of
them, first and last chunk of the slot. With o = (A - P) mod 2^64, both P + (o mod 2^32) (the offset
truncated) and P + sign_extend32(o) (truncated and sign-extended) lie inside the arena, at least 16
bytes before its end. The arena's size follows from the cases by this rule (arena_bytes) and is at most
12 GiB; the lowest base of every layout lies LEAD = 2^31 + 4096 bytes into it. And for every stride or
distance a case is meant to stress there is a pair (P, A) whose two aliases both differ from A (kind
"both"), so the mistake cannot go unseen; where a quantity stays below 2^32 only the sign-extended
alias can differ (kind "sign"). The address A of such a pair is one the call really forms: a slot that
the case's masks make it read or write (touched, stress_of). So the blocks' kinds are placed, not
shuffled: block 4, the one past 2^32 in far_blocks, and block 2, past 2^31, are rebuilt (far_lost).

A shard stride of 2^32 and more (REFUSED_STRIDE) is refused by the calls that rebuild (reconstruct,
recover, their wide and ragged forms, reconstruct-some) before anything is enqueued; the other calls
take any 64-bit stride, which no arena of 12 GiB can hold, so they are not run on it.
"""
from collections import namedtuple

import numpy as np

from arena import GUARD, Region, rup16

FAMILIES = ["far_blocks", "far_parity_above", "far_parity_below", "far_shards"]
LEAD = (1 << 31) + 4096
CAP = 12 << 30
B = 5
L_LONG, L_SHORT = 1202, 33           # 76 chunks with a 2-byte tail; the short-shard tile rebuild
BLOCK_STRIDE = (1 << 30) + 16 * 4099
DIST_HI = (1 << 32) + 16 * 777       # parity - data (far_parity_above), data - parity (far_parity_below)
DIST_MID = (1 << 31) + 16 * 333      # the third region above the lowest one
WIDE_SHARD_STRIDE = (1 << 26) + 16 * 257
REFUSED_STRIDE = 1 << 32
RAGGED_LENS = (1202, 1, 17, 600, 1202)

# kind: "both"; "sign": only the sign-extended alias differs (0 < A - P < 2^32); "wrap": a negative
# distance of less than 4 GiB, whose zero-extended alias differs (the third region seen from the highest)
Stress = namedtuple("Stress", "what P A kind")


def shard_stride_for(k, m):
    """far_shards: the shard stride that puts shard t, t >= k as small as the arena allows, just past
    2^32: rup16(ceil(2^32 / t)) + 16*257."""
    for t in range(k, k + m):
        ss = rup16(-(-(1 << 32) // t)) + 16 * 257
        if LEAD + (k + m) * ss + (1 << 20) <= CAP:
            return ss
    raise ValueError("no shard of RS(%d,%d) can lie past 2^32 in a 12 GiB arena" % (k, k + m))


class FarLayout:
    """The regions of one case (name -> Region, each with .win, the bytes of a slot the host models:
    the whole slot, for shard-major regions the block stride), the bases the call is given,
    and the arena bytes the rule asks for."""

    def __init__(self, family, regions, win, L):
        self.family, self.regions, self.L = family, regions, L
        for r in regions.values():
            r.win = win
            assert rup16(L) <= win <= r.ss
        lo, hi = alias_extent(self)
        assert lo >= GUARD, "an alias below the arena"
        self.size = -(-(max(hi + 16, max(r.end() for r in regions.values())) + GUARD) // 4096) * 4096

    def bases(self):
        return {name: r.off for name, r in self.regions.items()}


def aliases(P, A):
    """What address A becomes when its offset from the base P is cut to 32 bits: zero-extended and
    sign-extended."""
    lo = ((A - P) % (1 << 64)) % (1 << 32)
    return P + lo, P + (lo - (1 << 32) if lo >= (1 << 31) else lo)


def slot_addresses(lay):
    """First and last chunk of every shard slot of every region."""
    last = rup16(lay.L) - 16
    for r in lay.regions.values():
        for b in range(r.B):
            for j in range(r.rows):
                yield r.at(b, j)
                yield r.at(b, j) + last


def alias_extent(lay):
    """(lowest, highest) alias of any slot address through any base."""
    al = [x for P in lay.bases().values() for A in slot_addresses(lay) for x in aliases(P, A)]
    return min(al), max(al)


def far_layout(family, k, m, L, third=None, rows=0, shard_stride=None):
    """The layout of B blocks of RS(k, k+m) shards of L bytes in one family; third: the name of a third
    region of `rows` slots per block ("out" of a recover, "old" of the update), or None."""
    R = rup16(L)
    if family == "far_blocks":
        ss, bs = R + 32, BLOCK_STRIDE
        d = LEAD
        p = d + k * ss + 64
        regions = dict(data=Region(d, bs, ss, k, B), parity=Region(p, bs, ss, m, B))
        if third:
            regions[third] = Region(p + m * ss + 48, bs, ss, rows, B)
        win = ss
    elif family in ("far_parity_above", "far_parity_below"):
        ss = R + 32
        lo, mid, hi = LEAD, LEAD + DIST_MID, LEAD + DIST_HI
        d, p = (lo, hi) if family == "far_parity_above" else (hi, lo)
        regions = dict(data=Region(d, k * ss + 48, ss, k, B), parity=Region(p, m * ss + 16, ss, m, B))
        if third:
            regions[third] = Region(mid, rows * ss + 32, ss, rows, B)
        win = ss
    elif family == "far_shards":
        sp = R + 16
        SS = shard_stride or shard_stride_for(k, m)
        assert SS < (1 << 32) and 2 * B * sp + 64 <= SS
        regions = dict(data=Region(LEAD, sp, SS, k, B), parity=Region(LEAD + k * SS, sp, SS, m, B))
        if third:   # in the gaps of the data region's strides
            regions[third] = Region(LEAD + B * sp + 64, sp, SS, rows, B)
        win = sp
    else:
        raise ValueError(family)
    return FarLayout(family, regions, win, L)


# ---------------------------------------------------------------- the cases

# Routes among the shipped kernels, forced with the tune fixture as the variant tables of
# test_gpu_codec.py do. A route that a shape takes by itself has no knobs.
ROUTES = {
    "default": {},
    "own": dict(enc_fixed=1),                    # the code's own encode kernel
    "generic": dict(enc_fixed=0),                # the generic encode
    "direct": {},                                # one output slot, or m = 1
    "routed": dict(dec_route=1),                 # RS(8,12) in place: classify pass, then one routed kernel
    "noroute": dict(dec_route=0),                # RS(8,12) in place: sorted plans, runtime-k wave rebuild
    "wave": {},                                  # sorted plans, runtime-k wave rebuild
    "rebuild_k": {},                             # sorted plans, compile-time-k rebuild
    "tile": dict(dec_direct=0, dec_wave=0),      # plans in block order, workgroup-tile rebuild
    "short": {},                                 # the same by shard length (L = 33)
}

Case = namedtuple("Case", "call family k m L step route opt")


def case_id(c):
    return "-".join(str(x) for x in (c.call[4:].replace("_batch", ""), c.family, c.k, c.m, c.L, c.step, c.route, c.opt)
                    if x not in (None, ""))


def _narrow_decode():
    """(k, m, L, step, route, opt) of the reconstruct and recover cases; opt "single": no recoverable
    block loses two data shards, so the routed kernel runs on a zero route word."""
    out = [(2, 1, L_LONG, "reconstruct", "direct", None), (2, 1, L_LONG, "recover_1", "direct", None),
           (8, 4, L_LONG, "reconstruct", "routed", "single"), (8, 4, L_LONG, "reconstruct", "routed", None),
           (8, 4, L_LONG, "reconstruct", "noroute", None), (8, 4, L_LONG, "recover_m", "wave", None),
           (8, 4, L_LONG, "recover_1", "direct", None),
           (8, 4, L_LONG, "reconstruct", "tile", None), (8, 4, L_LONG, "recover_m", "tile", None),
           (8, 4, L_SHORT, "reconstruct", "short", None), (8, 4, L_SHORT, "recover_m", "short", None)]
    for k, m in ((6, 2), (10, 22)):
        out += [(k, m, L_LONG, "reconstruct", "wave", None), (k, m, L_LONG, "recover_m", "wave", None)]
    out.append((6, 2, L_LONG, "recover_1", "direct", None))
    for k, m in ((16, 8), (20, 10)):
        out += [(k, m, L_LONG, "reconstruct", "rebuild_k", None), (k, m, L_LONG, "recover_m", "rebuild_k", None),
                (k, m, L_LONG, "recover_1", "direct", None)]
    return out


def _cases():
    out = []
    for f in FAMILIES:
        for k, m in ((2, 1), (8, 4), (16, 8), (20, 10)):
            out += [Case("fec_rs_encode_batch", f, k, m, L_LONG, "encode", r, None) for r in ("own", "generic")]
        out += [Case("fec_rs_encode_batch", f, k, m, L_LONG, "encode", "generic", None) for k, m in ((6, 2), (5, 11))]
        for k, m, L, step, route, opt in _narrow_decode():
            call = "fec_rs_reconstruct_batch" if step == "reconstruct" else "fec_rs_recover_batch"
            out.append(Case(call, f, k, m, L, step, route, opt))
        out += [Case("fec_xor_encode_batch", f, 3, 1, L_LONG, "encode", "default", None),
                Case("fec_xor_reconstruct_batch", f, 3, 1, L_LONG, "reconstruct", "default", None)]
        for k, m in ((20, 10), (40, 20)):
            out += [Case("fec_rs_reconstruct_wide_batch", f, k, m, L_LONG, "reconstruct", "default", None),
                    Case("fec_rs_recover_wide_batch", f, k, m, L_LONG, "recover_m", "default", None)]
        if f == "far_shards":   # (40,20) again at the stride that puts shard 40 past 2^32
            out += [Case("fec_rs_reconstruct_wide_batch", f, 40, 20, L_LONG, "reconstruct", "default", "past4g"),
                    Case("fec_rs_recover_wide_batch", f, 40, 20, L_LONG, "recover_m", "default", "past4g")]
        out += [Case("fec_rs_encode_ragged_batch", f, 8, 4, L_LONG, "encode", "default", None),
                Case("fec_rs_reconstruct_ragged_batch", f, 8, 4, L_LONG, "reconstruct", "default", None),
                Case("fec_rs_recover_ragged_batch", f, 8, 4, L_LONG, "recover_m", "default", None)]
        out += [Case("fec_rs_verify_batch", f, k, m, L_LONG, "verify", "default", None) for k, m in ((8, 4), (20, 10))]
        out += [Case(call, f, 8, 4, L_LONG, step, "default", None) for call, step in (
            ("fec_rs_reconstruct_some_batch", "some"), ("fec_rs_update_batch", "update"),
            ("fec_rs_encode_idx_batch", "encode_idx"), ("fec_rs_locate_batch", "locate"),
            ("fec_rs_locate_multi_batch", "locate_multi"), ("fec_rs_locate_partial_batch", "locate_partial"))]
    return out


CASES = _cases()

# Every device entry point: the families it runs on, what it is refused on, its forced routes. The
# families and routes are those of CASES (test_far_cases.py compares them); a call added to
# include/fec_hip.h must be added here and given cases.
REBUILD_CALLS = {"fec_rs_reconstruct_batch", "fec_rs_recover_batch", "fec_rs_reconstruct_wide_batch",
             "fec_rs_recover_wide_batch", "fec_rs_reconstruct_ragged_batch", "fec_rs_recover_ragged_batch",
             "fec_rs_reconstruct_some_batch"}
TABLE = {call: dict(run=sorted({c.family for c in CASES if c.call == call}, key=FAMILIES.index),
                    refused=["shard_stride_4gib"] if call in REBUILD_CALLS else [],
                    routes=sorted({c.route for c in CASES if c.call == call}))
         for call in ["fec_rs_encode_batch", "fec_rs_reconstruct_batch", "fec_rs_recover_batch",
                      "fec_rs_reconstruct_wide_batch", "fec_rs_recover_wide_batch", "fec_rs_encode_ragged_batch",
                      "fec_rs_reconstruct_ragged_batch", "fec_rs_recover_ragged_batch", "fec_rs_verify_batch",
                      "fec_rs_locate_batch", "fec_rs_locate_multi_batch", "fec_rs_locate_partial_batch",
                      "fec_rs_reconstruct_some_batch", "fec_rs_update_batch", "fec_rs_encode_idx_batch",
                      "fec_xor_encode_batch", "fec_xor_reconstruct_batch"]}


def cases_of(*calls):
    return [c for c in CASES if c.call in calls]


def slots_of(c):
    """Output slots per block of a recover case (0: the call has no out region)."""
    return {"recover_m": c.m, "recover_1": 1}.get(c.step, 0)


def layout_of(c):
    if c.step == "update":
        third, rows = "old", c.k
    else:
        rows = slots_of(c)
        third = "out" if rows else None
    wide = c.call.endswith("_wide_batch") and (c.k, c.m) == (40, 20) and c.opt != "past4g"
    return far_layout(c.family, c.k, c.m, c.L, third, rows, WIDE_SHARD_STRIDE if wide else None)


_size = []


def arena_bytes():
    """The arena every case fits by the rule."""
    if not _size:
        _size.append(max(layout_of(c).size for c in CASES))
    return _size[0]


# ---------------------------------------------------------------- which shards a case loses

WIDE_W = 2   # mask words of the wide cases: (20,10) with two words runs the wide kernels, not the forward


def mode_of(c):
    """"single": no recoverable block loses two data shards (the routed kernel's zero route word);
    "one_slot": a recover into one slot per block; else "multi"."""
    return "single" if c.opt == "single" else "one_slot" if c.step == "recover_1" else "multi"


def far_lost(k, m, mode="multi"):
    """bool [B, k + m], shard j of block b lost. The kinds are placed so that the blocks far from the
    bases do work: block 0 intact, block 1 too few shards (every parity shard and data shard 0 lost),
    block 2 one data shard lost (and parity shard 0), block 3 parity-only loss, block 4 several data
    shards lost. A block that is rebuilt loses its farthest data shard, k - 1, and block 4 also the
    first parity shards, as many as leave it k shards, so that it reads the last parity shards, the
    farthest of all. Codes and modes that cannot rebuild two data shards of a block ("single", m = 1)
    lose one in block 4. "one_slot" with min(k, m) >= 2: block 0 has the parity-only loss, block 3 loses
    several data shards (more than the slot holds: refused, untouched), block 4 one."""
    n, lo = k + m, min(k, m)
    e = lo if lo <= 3 else lo // 2

    def rebuilt(e_d):
        row = np.zeros(n, dtype=bool)
        row[[k - 1] + list(range(0, k - 1, 2))[:e_d - 1]] = True
        row[k:k + m - e_d] = True
        assert row[:k].sum() == e_d and row.sum() == m
        return row

    lost = np.zeros((B, n), dtype=bool)
    lost[1, k:] = True
    lost[1, 0] = True
    lost[2, k // 2] = True
    lost[2, k:k + (1 if m >= 2 else 0)] = True
    par_only = 0 if (mode == "one_slot" and lo >= 2) else 3
    lost[par_only, n - 1] = True
    lost[par_only, k:k + (1 if m >= 3 else 0)] = True
    if mode == "one_slot" and lo >= 2:
        lost[3] = rebuilt(e)
    lost[4] = rebuilt(e if (mode == "multi" and lo >= 2) else 1)
    return lost


def block_kinds(lost, k):
    """Kind of each block as test_gpu_layouts.make_masks numbers them: 0 intact, 1 parity-only loss, 2 one
    data shard lost, 3 several, 4 too few shards."""
    e_d = lost[:, :k].sum(axis=1)
    few = (e_d > 0) & ((~lost).sum(axis=1) < k)
    return np.where(few, 4, np.where(e_d >= 2, 3, np.where(e_d == 1, 2, np.where(lost.any(axis=1), 1, 0))))


def kinds_wanted(k, m, mode):
    if min(k, m) < 2 or mode == "single":
        return [0, 4, 2, 1, 2]
    return [1, 4, 2, 3, 2] if mode == "one_slot" else [0, 4, 2, 1, 3]


def xor_lost(k):
    """XOR(k, 1): block 0 intact, block 1 two shards lost (fails), block 2 one data shard, block 3 the
    parity, block 4 the farthest data shard."""
    lost = np.zeros((B, k + 1), dtype=bool)
    lost[1, [0, k]] = True
    lost[2, k // 2] = True
    lost[3, k] = True
    lost[4, k - 1] = True
    return lost


def masks_of(lost):
    """uint32 [B] present masks (k + m <= 32)."""
    n = lost.shape[1]
    assert n <= 32
    return ((~lost).astype(np.uint64) << np.arange(n, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def column_sets(k):
    """Update: bool [B, k]: no column, the first, all, every other one, the last (the farthest shard)."""
    cols = np.zeros((B, k), dtype=bool)
    cols[1, 0] = True
    cols[2] = True
    cols[3, ::2] = True
    cols[4, k - 1] = True
    return cols


def idx_columns(k):
    """Encode-idx: two columns per block, the farthest among them."""
    cols = np.zeros((B, k), dtype=bool)
    cols[np.arange(B), np.arange(B) % (k - 1)] = True
    cols[:, k - 1] = True
    return cols


def partial_lost(k, m):
    """Locate-partial: blocks 1, 2 and 4 miss a shard (data 3, data 0, parity 0)."""
    lost = np.zeros((B, k + m), dtype=bool)
    lost[1, 3] = lost[2, 0] = lost[4, k] = True
    return lost


def lost_of(c):
    """The lost shards of a decoding case (None: the call is given every shard)."""
    if c.call.startswith("fec_xor"):
        return xor_lost(c.k) if c.step == "reconstruct" else None
    if c.step in ("reconstruct", "recover_m", "recover_1", "some"):
        return far_lost(c.k, c.m, mode_of(c))
    return partial_lost(c.k, c.m) if c.step == "locate_partial" else None


def touched(c):
    """The shard slots (region, block, slot) that the call of case c must read or write, by its masks."""
    k, m = c.k, c.m
    T = set()
    lost = lost_of(c)

    def add(b, shard):
        T.add(("data", b, shard) if shard < k else ("parity", b, shard - k))

    if c.step in ("encode", "verify", "locate", "locate_multi"):
        T = {("data", b, j) for b in range(B) for j in range(k)} | {("parity", b, i) for b in range(B) for i in range(m)}
    elif c.step == "locate_partial":
        for b, j in np.argwhere(~lost):
            add(int(b), int(j))
    elif c.step in ("update", "encode_idx"):
        cols = column_sets(k) if c.step == "update" else idx_columns(k)
        for b in np.flatnonzero(cols.any(axis=1)):
            T |= {("parity", int(b), i) for i in range(m)}
            for j in np.flatnonzero(cols[b]):
                T.add(("data", int(b), int(j)))
                if c.step == "update":
                    T.add(("old", int(b), int(j)))
    else:
        slots = slots_of(c)
        for b in range(B):
            gone, have = np.flatnonzero(lost[b]), np.flatnonzero(~lost[b])
            e_d = int((gone < k).sum())
            if c.call.startswith("fec_xor"):
                works = e_d == 1 and len(gone) == 1
            elif c.step == "some":
                works = len(gone) > 0 and len(have) >= k
            else:
                works = e_d > 0 and len(have) >= k and (slots == 0 or e_d <= slots)
            if not works:
                continue
            for j in have[:k]:
                add(b, int(j))
            for r, j in enumerate(gone if c.step == "some" else gone[gone < k]):
                if slots:
                    T.add(("out", b, r))
                else:
                    add(b, int(j))
    return T


def stress_of(c):
    """The pairs (P, A) of case c: for every stride or distance its family stresses, a base and the
    farthest slot address that the call forms through it (touched)."""
    lay = layout_of(c)
    T = touched(c)

    def far(names, blocks=range(B)):
        at = [lay.regions[n].at(b, j) for n, b, j in T if n in names and b in blocks]
        assert at, "the call touches no slot of %s in blocks %s" % (names, list(blocks))
        return max(at)

    out = []
    third = [n for n in lay.regions if n not in ("data", "parity")]
    if c.family == "far_blocks":
        for name, r in lay.regions.items():
            out += [Stress("b * %s block stride" % name, r.off, far([name]), "both"),
                    Stress("b * %s block stride past 2^31" % name, r.off, far([name], (2, 3)), "sign")]
    elif c.family in ("far_parity_above", "far_parity_below"):
        d, p = lay.regions["data"].off, lay.regions["parity"].off
        out = [Stress("parity - data", d, far(["parity"]), "both"), Stress("data - parity", p, far(["data"]), "both")]
        for name in third:
            lo, hi = (("data", d), ("parity", p)) if d < p else (("parity", p), ("data", d))
            out += [Stress("%s - %s" % (name, lo[0]), lo[1], far([name]), "sign"),
                    Stress("%s - %s" % (name, hi[0]), hi[1], far([name]), "wrap")]
    else:
        wide_sign = lay.regions["data"].ss == WIDE_SHARD_STRIDE
        out = [Stress("j * shard stride", lay.regions["data"].off, far(["data", "parity"]), "sign" if wide_sign else "both")]
    return out


# ---------------------------------------------------------------- contents

_contents = {}


def far_rs_case(oracle, k, m, L, mode="multi"):
    """Host side of the reconstruct and recover cases, computed once: shards [B, n, L] with the oracle's
    parity, every block with contents of its own, the lost shards of far_lost, the damaged batch (lost
    shards 0x5A) and the oracle's in-place reconstruct of it (k + m <= 32)."""
    key = (k, m, L, mode)
    if key not in _contents:
        sh = np.zeros((B, k + m, L), dtype=np.uint8)
        sh[:, :k] = np.random.default_rng(100000 * k + 1000 * m + L).integers(0, 256, (B, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        lost = far_lost(k, m, mode)
        masks = masks_of(lost)
        e_d = lost[:, :k].sum(axis=1)
        few = block_kinds(lost, k) == 4
        dmg = sh.copy()
        dmg[lost] = 0x5A
        rec = dmg.copy()
        st = oracle.rs_reconstruct(k, m, rec, masks)
        assert np.array_equal(st != 0, few)
        assert np.array_equal(rec[~few][:, :k], sh[~few][:, :k])
        assert np.array_equal(rec[few], dmg[few]) and np.array_equal(rec[:, k:], dmg[:, k:])
        for a in (sh, masks, lost, e_d, few, dmg, rec):
            a.setflags(write=False)
        _contents[key] = dict(sh=sh, masks=masks, lost=lost, e_d=e_d, few=few, dmg=dmg, rec=rec)
    return _contents[key]


def far_xor_case(oracle, k, L):
    """The same for XOR(k, 1): the lost shards of xor_lost, fail: the blocks the call cannot rebuild."""
    key = ("xor", k, L)
    if key not in _contents:
        sh = np.zeros((B, k + 1, L), dtype=np.uint8)
        sh[:, :k] = np.random.default_rng(77 + k).integers(0, 256, (B, k, L), dtype=np.uint8)
        oracle.xor_encode(k, sh)
        lost = xor_lost(k)
        masks = masks_of(lost)
        dmg = sh.copy()
        dmg[lost] = 0x5A
        rec = dmg.copy()
        st = oracle.xor_reconstruct(k, rec, masks)
        fail = lost[:, :k].any(axis=1) & (lost.sum(axis=1) >= 2)
        assert np.array_equal(st != 0, fail) and fail.tolist() == [False, True, False, False, False]
        assert np.array_equal(rec[~fail][:, :k], sh[~fail][:, :k])
        _contents[key] = dict(sh=sh, masks=masks, lost=lost, dmg=dmg, rec=rec, fail=fail)
    return _contents[key]
