"""Batches of the ragged verify and the ragged reconstruct-some tests (test_gpu_ragged_more.py,
test_gpu_ragged_more_far.py) and their expected images. No device is needed here;
test_ragged_more_cases.py checks this module on the CPU.

Expected parity comes from an encode function given by the caller (the oracle's for the default
matrix, tests/cauchy_model.py's for the other kinds), run per block at the block's own length;
expected statuses come from the masks and the lengths alone.

A batch lives in one canary-filled arena (arena.py) whose every byte is compared after a call: shard
stride S = 1216 with max_shard_len 1202, block strides with gaps, guards at both ends.
  verify  nothing is written, so the image after the call is the image before it. Every slot holds
          random garbage from the block's length on, to the end of the slot: bytes that must not matter.
  some    input slots hold canary from the block's length on and lost shards ERASED over their whole
          slot; a rebuilt shard receives bytes [0, len) and zeros to round_up(len, 16), and every other
          byte stays, those of failed, zero-length and oversize blocks included.
"""
import numpy as np

import far_cases as fc
from arena import CANARY, GUARD, Region, canary_image, rup16

ERASED = 0x5A
GAP = 208
S = 1216
MAXL = 1202
B = 301
PATTERN = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1200, 1201, 1202]
RAG_G = [0, 1, 3, 16]
SHARD_SIZE, TOO_FEW, SINGULAR = -5, -4, -11

# (10,22): two row passes; (100,40): three passes of up to 1600 tables, staged in LDS; (130,20): a first
# pass of 16 * 130 = 2080 tables, past the 2048 kept in LDS, read from global memory (k > 128 is what
# that takes), and a second pass of 4 rows from LDS
VERIFY_SHAPES = [(8, 4, B), (20, 10, B), (2, 1, B), (1, 1, B), (10, 22, B), (100, 40, 20), (130, 20, 20)]
SOME_SHAPES = [(8, 4), (20, 10), (2, 1), (16, 16), (10, 22), (1, 31), (5, 0)]

# what is done to a block of a verify batch
V_CLEAN, V_DATA_LAST, V_PAR_LAST, V_DATA_FIRST, V_PAR_MID, V_DATA_MID, V_PAR_HIGH = range(7)
# how a block of a reconstruct-some batch loses shards, and what its want mask names
M_FULL, M_EXACT, M_FEW, M_PARITY, M_DATA, M_MIXED = range(6)
W_ALL, W_DATA, W_PARITY, W_ZERO, W_RANDOM = range(5)


def default_lens(nb):
    return np.array([PATTERN[b % len(PATTERN)] for b in range(nb)], dtype=np.uint32)


def usable(lens, maxl=MAXL):
    """The lengths with the oversize ones at 0: the bytes of a block that a call may touch."""
    lens = np.asarray(lens, dtype=np.uint32)
    return np.where(lens <= maxl, lens, 0).astype(np.int64)


def span_mask(lo, hi, width):
    """bool [len(lo), 1, width]: byte x of block b lies in [lo[b], hi[b])."""
    x = np.arange(width)[None, None, :]
    return (x >= np.asarray(lo)[:, None, None]) & (x < np.asarray(hi)[:, None, None])


def signature(*parts):
    """A hashable statement of the inputs a cached batch was built from (arrays by their bytes)."""
    out = []
    for p in parts:
        if p is None or isinstance(p, (int, str, tuple)):
            out.append(p)
        elif isinstance(p, dict):
            out.append(tuple(sorted((b, tuple(v)) for b, v in p.items())))
        else:
            a = np.ascontiguousarray(p)
            out.append((a.dtype.str, a.shape, a.tobytes()))
    return tuple(out)


def oracle_encode(oracle):
    def enc(k, m, data):
        sh = np.zeros((data.shape[0], k + m, data.shape[2]), dtype=np.uint8)
        sh[:, :k] = data
        if m:
            oracle.rs_encode(k, m, sh)
        return sh[:, k:]
    enc.tag = "oracle"
    return enc


def matrix_encode(M):
    """The encode of an n x k matrix M by tests/cauchy_model.py's arithmetic."""
    import cauchy_model as cm

    def enc(k, m, data):
        return cm.encode(M, data)
    enc.tag = signature(M)
    return enc


def encoded(enc, k, m, data, ok):
    """[nb, k + m, ss]: the data below each block's length (zero from it on) and its parity."""
    ss = data.shape[2]
    sh = np.zeros((data.shape[0], k + m, ss), dtype=np.uint8)
    sh[:, :k] = np.where(span_mask(0 * ok, ok, ss), data, 0)
    if m:
        sh[:, k:] = enc(k, m, sh[:, :k])
    return sh


def make_arena(layout, nb, k, m, ss=S):
    """(image, data, parity): one canary-filled arena; the blocks of a region lie apart."""
    n = k + m
    if layout == "interleaved":
        bs = n * ss + 48
        data = Region(GUARD, bs, ss, k, nb)
        par = Region(GUARD + k * ss, bs, ss, m, nb)
    else:   # split: the parity region below the data region
        par = Region(GUARD, max(m, 1) * ss + 16, ss, m, nb)
        data = Region(par.end() + GAP, k * ss + 48, ss, k, nb)
    return canary_image([data, par]), data, par


# ---------------------------------------------------------------- verify

_verify = {}


def verify_case(enc, k, m, nb=B, lens=None, key=None, ss=S, maxl=MAXL, hits=None):
    """One verify batch, built once per set of inputs and left unchanged: the slots' contents [nb, k + m, ss]
    (encoded below each block's length, random from it on, then corrupted), what was done to each
    block, the flipped bytes (block, shard, offset), and the expected statuses. Block b's kind is
    (b // 14 + b % 14) % 7, so that every residue of the length pattern meets every kind; `hits`
    (block -> list of (shard, offset)) replaces the kinds."""
    lens = default_lens(nb) if lens is None else np.asarray(lens, dtype=np.uint32)
    ck = (k, m, nb, key, ss, maxl, enc.tag) + signature(lens, hits)
    if ck in _verify:
        return _verify[ck]
    n = k + m
    rng = np.random.default_rng(424243 * k + 1013 * m + nb)
    ok = usable(lens, maxl)
    slots = rng.integers(0, 256, (nb, n, ss), dtype=np.uint8)
    sh = encoded(enc, k, m, slots[:, :k], ok)
    v = span_mask(0 * ok, ok, ss)
    slots = np.where(v, sh, slots)
    kind = np.zeros(nb, dtype=np.int64)
    flips = []
    for b in range(nb):
        Lb = int(ok[b])
        if Lb == 0 or m == 0:
            continue
        mid = (Lb // 2) & ~15 | 5 if Lb > 48 else Lb // 2
        if hits is not None:
            todo = hits.get(b, [])
            kind[b] = V_DATA_MID if todo else V_CLEAN
        else:
            kd = (b // 14 + b % 14) % 7
            if kd == V_PAR_HIGH and m <= 16:
                kd = V_DATA_MID
            kind[b] = kd
            todo = {V_CLEAN: [], V_DATA_LAST: [(int(rng.integers(0, k)), Lb - 1)],
                    V_PAR_LAST: [(k + int(rng.integers(0, m)), Lb - 1)], V_DATA_FIRST: [(int(rng.integers(0, k)), 0)],
                    V_PAR_MID: [(k + int(rng.integers(0, m)), mid)], V_DATA_MID: [(int(rng.integers(0, k)), mid)],
                    V_PAR_HIGH: [(k + int(rng.integers(16, max(m, 17))), mid)]}[kd]
        for j, x in todo:
            assert 0 <= x < Lb and j < n
            slots[b, j, x] ^= 1 << int(rng.integers(0, 8))
            flips.append((b, j, x))
    bad = np.zeros(nb, dtype=bool)
    bad[[f[0] for f in flips]] = True
    # (a code without parity has nothing to compare and launches nothing: every status is 1, the
    # oversize blocks' too, and the sticky word stays clear; fec_hip_ragged.h)
    status = (np.where(lens > maxl, SHARD_SIZE, np.where(bad, 0, 1)) if m else np.ones(nb)).astype(np.int32)
    for a in (lens, ok, slots, sh, kind, status):
        a.setflags(write=False)
    _verify[ck] = dict(k=k, m=m, lens=lens, ok=ok, slots=slots, sh=sh, kind=kind, flips=flips, status=status,
                       count=int(bad.sum()))
    return _verify[ck]


def verify_image(c, layout, ss=S):
    """(image, data, parity) of a verify batch: the image the call is given and must leave."""
    k, m = c["k"], c["m"]
    img, data, par = make_arena(layout, c["lens"].size, k, m, ss)
    data.view(img)[...] = c["slots"][:, :k]
    par.view(img)[...] = c["slots"][:, k:]
    return img, data, par


# ---------------------------------------------------------------- reconstruct-some

_some = {}


def bits(words, n):
    return ((np.asarray(words, dtype=np.uint32)[:, None] >> np.arange(n, dtype=np.uint32)[None, :]) & 1).astype(bool)


def pack(b):
    n = b.shape[1]
    assert n <= 32
    return (b.astype(np.uint64) << np.arange(n, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def lose(rng, k, m, kd):
    """The shards a block of mask kind kd loses (what the code cannot express falls back to a kind it
    can: without parity every loss is one too many)."""
    n = k + m
    if kd == M_FEW:
        return rng.choice(n, size=m + 1, replace=False)
    if m == 0 or kd == M_FULL:
        return np.array([], dtype=np.int64)
    if kd == M_EXACT:
        return rng.choice(n, size=m, replace=False)
    if kd == M_PARITY:
        return k + rng.choice(m, size=int(rng.integers(1, m + 1)), replace=False)
    if kd == M_MIXED and m >= 2:
        nd = int(rng.integers(1, min(k, m - 1) + 1))
        npar = int(rng.integers(1, m - nd + 1))
        return np.concatenate([rng.choice(k, size=nd, replace=False), k + rng.choice(m, size=npar, replace=False)])
    return rng.choice(k, size=int(rng.integers(1, min(k, m) + 1)), replace=False)


def some_statuses(lost, want, k, lens, maxl=MAXL, singular=None):
    """(status, rebuilt [nb, n]) by the masks: nothing missing and wanted 0; fewer than k present
    TOO_FEW; dependent rows (singular [nb], custom codes) SINGULAR; else the missing wanted shards are
    rebuilt. An oversize length overrides the status; a block without bytes has nothing written."""
    R = lost & want
    few = R.any(axis=1) & ((~lost).sum(axis=1) < k)
    sing = np.zeros(len(lost), dtype=bool) if singular is None else (singular & R.any(axis=1) & ~few)
    st = np.where(few, TOO_FEW, np.where(sing, SINGULAR, 0))
    rebuilt = R & ~(few | sing)[:, None] & (usable(lens, maxl) > 0)[:, None]
    return np.where(np.asarray(lens) > maxl, SHARD_SIZE, st).astype(np.int32), st.astype(np.int32), rebuilt


def some_case(enc, k, m, nb=B, lens=None, key=None, ss=S, maxl=MAXL, lost=None, want=None, singular=None):
    """One reconstruct-some batch, built once per set of inputs: the encoded shards, per block the lost shards
    (mask kind (b // 14 + b % 14) % 6) and the want mask (want kind (b // 3) % 5), the expected
    statuses with and without want masks, and the shards each form rebuilds."""
    lens = default_lens(nb) if lens is None else np.asarray(lens, dtype=np.uint32)
    ck = (k, m, nb, key, ss, maxl, enc.tag) + signature(lens, lost, want, singular)
    if ck in _some:
        return _some[ck]
    n = k + m
    rng = np.random.default_rng(7907 * k + 37 * m + nb)
    ok = usable(lens, maxl)
    sh = encoded(enc, k, m, rng.integers(0, 256, (nb, k, ss), dtype=np.uint8), ok)
    mkind = np.array([(b // 14 + b % 14) % 6 for b in range(nb)])
    wkind = np.array([(b // 3) % 5 for b in range(nb)])
    if lost is None:
        lost = np.zeros((nb, n), dtype=bool)
        for b in range(nb):
            lost[b, lose(rng, k, m, mkind[b])] = True
    if want is None:
        want = np.zeros((nb, n), dtype=bool)
        for b in range(nb):
            want[b] = {W_ALL: np.ones(n, dtype=bool), W_DATA: np.arange(n) < k, W_PARITY: np.arange(n) >= k,
                       W_ZERO: np.zeros(n, dtype=bool), W_RANDOM: rng.integers(0, 2, n).astype(bool)}[wkind[b]]
    masks, wants = pack(~lost), pack(want)
    # bits at and above n are ignored: set some in both words
    if n < 32:
        masks = masks | (rng.integers(0, 2, nb).astype(np.uint32) << np.uint32(n))
        wants = wants | (np.uint32(0xFFFFFFFF) << np.uint32(n)) * (wkind == W_ALL).astype(np.uint32)
    out = dict(k=k, m=m, lens=lens, ok=ok, sh=sh, lost=lost, want=want, masks=masks.astype(np.uint32),
               wants=wants.astype(np.uint32), mkind=mkind, wkind=wkind)
    for name, w in (("all", np.ones((nb, n), dtype=bool)), ("want", want)):
        st, by_mask, rebuilt = some_statuses(lost, w, k, lens, maxl, singular)
        out["st_" + name], out["by_mask_" + name], out["rebuilt_" + name] = st, by_mask, rebuilt
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _some[ck] = out
    return out


def some_images(c, layout, which, ss=S):
    """(image before, model after, data, parity) of a reconstruct-some batch; which: "all" (no want
    masks) or "want"."""
    k, m, ok = c["k"], c["m"], c["ok"]
    nb = c["lens"].size
    img, data, par = make_arena(layout, nb, k, m, ss)
    v = span_mask(0 * ok, ok, ss)
    src = np.where(c["lost"][:, :, None], ERASED, np.where(v, c["sh"], CANARY)).astype(np.uint8)
    data.view(img)[...] = src[:, :k]
    par.view(img)[...] = src[:, k:]
    model = img.copy()
    sel = c["rebuilt_" + which][:, :, None]
    after = np.where(sel & v, c["sh"], np.where(sel & span_mask(ok, rup16(ok), ss), 0, src)).astype(np.uint8)
    data.view(model)[...] = after[:, :k]
    par.view(model)[...] = after[:, k:]
    return img, model, data, par


def sync_code(statuses, by_mask=None):
    """What fec_sync() returns after a call with these statuses (by_mask: what the masks alone give,
    which the sticky word records for oversize blocks too)."""
    seen = set(np.asarray(statuses).tolist()) | (set(np.asarray(by_mask).tolist()) if by_mask is not None else set())
    for code in (TOO_FEW, SHARD_SIZE, SINGULAR):
        if code in seen:
            return code
    return 0


# ---------------------------------------------------------------- past 4 GiB

FAR_LENS = (1202, 1, 17, 600, 1202)


def far_layout(k, m, L=MAXL):
    """Five blocks whose block stride (2^30 + 16 * 4099: block 2 past 2^31, block 4 past 2^32) and
    data-to-parity distance (2^32 + 16 * 777) both exceed 32 bits, in the sparse arena of far_arena.py.
    far_cases.FarLayout asserts the rule of far_cases.py for every slot address through either base:
    a 32-bit mistake lands inside the arena."""
    ss = rup16(L) + 32
    regions = dict(data=Region(fc.LEAD, fc.BLOCK_STRIDE, ss, k, fc.B),
                   parity=Region(fc.LEAD + fc.DIST_HI, fc.BLOCK_STRIDE, ss, m, fc.B))
    return fc.FarLayout("far_blocks_and_parity", regions, ss, L)


def far_stress(lay, touched):
    """The pairs (P, A) a far case stresses, A the farthest touched slot (region, block, slot): the
    block stride of each region through its own base, and the distance between the regions through
    the other region's base."""
    def far(name, blocks=range(fc.B)):
        at = [lay.regions[n].at(b, j) for n, b, j in touched if n == name and b in blocks]
        assert at, "the call touches no slot of %s in blocks %s" % (name, list(blocks))
        return max(at)
    d, p = lay.regions["data"].off, lay.regions["parity"].off
    return [fc.Stress("b * data block stride", d, far("data"), "both"),
            fc.Stress("b * parity block stride", p, far("parity"), "both"),
            fc.Stress("b * data block stride past 2^31", d, far("data", (2, 3)), "sign"),
            fc.Stress("parity - data", d, far("parity", (0, 1)), "both"),
            fc.Stress("data - parity", p, far("data", (0, 1)), "both")]


def far_some_lost(k, m):
    """Block 0 loses a data and a parity shard, block 1 too many, block 2 one data shard and parity
    shard 0, block 3 only parity, block 4 its farthest data shard and its farthest parity shard."""
    lost = fc.far_lost(k, m).copy()
    lost[0, [1, k + 1]] = True
    lost[4] = False
    lost[4, [k - 1, k + m - 1]] = True
    return lost


def far_some_touched(lost, k):
    T = set()
    for b in range(fc.B):
        have = np.flatnonzero(~lost[b])
        if not lost[b].any() or len(have) < k or FAR_LENS[b] == 0:
            continue
        for j in list(have[:k]) + list(np.flatnonzero(lost[b])):
            T.add(("data", b, int(j)) if j < k else ("parity", b, int(j - k)))
    return T


def far_verify_touched(k, m):
    return {("data", b, j) for b in range(fc.B) for j in range(k)} | {("parity", b, i) for b in range(fc.B)
                                                                       for i in range(m)}
