"""Host-resident calls (FEC_HOST, FEC_HOST_PINNED) over host layouts, whole arena against a model:
the host-memory twin of test_gpu_layouts.py. include/fec_hip.h lets these flags take host memory
"with any layout" and promises exactly shard_len bytes written per output shard.

Every case lives in one host arena of uint8 pre-filled with a canary, with guards of GUARD bytes at
both ends; input slots hold canary from L on. After each call the WHOLE arena is compared byte for
byte with a numpy model: the image before the call with only the bytes the header lets the call
write changed. Encode: bytes [0, L) of every parity slot = the oracle's parity. Reconstruct: bytes
[0, L) of every erased data slot of a block that has an erased data shard and at least k shards
present = the oracle's rebuilt shard. Nothing else: not bytes [L, stride) of a slot, not an erased
parity slot, not a failed or complete block, not a gap, not a guard. Masks and statuses sit in
canary-guarded arrays of their own.

Memory kinds: "pageable" (numpy, FEC_HOST), "pinned" (torch pin_memory, FEC_HOST_PINNED, the region
bases interior pointers at addresses = 1, 2, 3 mod 4 across the cases) and "registered" (a numpy
arena under hipHostRegister for the length of the case, FEC_HOST_PINNED, regions at odd offsets
inside the registration).

Routes. The pinned path picks its copies from the caller's strides (fec_host.cpp): a chunk of nb
blocks goes up as ONE linear copy of its span plus span_to_stage_kernel when
    4 * ((nb - 1) * dbs + (k - 1) * ss + L) <= 5 * nb * k * L        ("dense"),
else as one 2D copy per data shard column; parity comes down as stage_to_packed_kernel plus ONE
linear copy when ss == L and pbs == m * L ("packed"), else as one 2D copy per column. For RS(8,4),
B = 61, chunks of 8 (seven of 8 blocks and one of 5), 7 (eight of 7, one of 5) or 61 (host_chunk = 0):

  layout              L     nb    4 * span    5 * nb*k*L   up              down
  packed_split        any   any   4 * nb*k*L  <            linear + s2s    s2p + linear
  slack_split         1202  8     309924      384640       linear + s2s    2D per column
                      1202  5     193668      240400       linear + s2s    2D
                      1202  7     271172      336560       linear + s2s    2D
                      1202  61    2363780     2932880      linear + s2s    2D
                      33    8     10660       10560        2D per column   2D
                      33    5     6628        6600         2D              2D
                      33    61    81892       80520        2D              2D
                      16    8     6308        5120         2D              2D
                      16    61    48708       39040        2D              2D
                      7     8     4004        2240         2D              2D
                      7     61    31140       17080        2D              2D
  word_slack          1202  8     309672      384640       linear + s2s    2D
                      1202  61    2361832     2932880      linear + s2s    2D
                      33    8     10660       10560        2D              2D
                      33    61    81892       80520        2D              2D
                      16    8     5552        5120         2D              2D
                      16    61    42864       39040        2D              2D
                      7     8     3500        2240         2D              2D
  interleaved         1202  8     443428      384640       2D              2D
                      1202  61    3508948     2932880      2D              2D
                      33    8     13236       10560        2D              2D
                      16    8     6980        5120         2D              2D
                      7     8     3668        2240         2D              2D
  shard_major_packed  1202  61    2346304     2932880      linear + s2s    2D, pitch == width
                      1202  8     2091480     384640       2D              2D, pitch == width
                      1202  7     2086672     336560       2D              2D, pitch == width
                      1202  5     2077056     240400       2D              2D, pitch == width
                      L     61    4 * 488 L   5 * 488 L    linear + s2s    2D, pitch == width
                      L     nb<9  4 (427+nb) L  40 nb L    2D              2D, pitch == width

(s2s = span_to_stage_kernel, s2p = stage_to_packed_kernel. The spans: slack_split, ss = L + 7 and
dbs = 8 ss + 16, has (nb - 1) dbs + 7 ss + L; word_slack the same with ss = round_up(L, 4) + 4, which
is L + 7 again at L = 33; interleaved, ss = L + 3 and dbs = 12 ss, carries four parity slots per block
and is never dense; shard_major_packed, dbs = L and ss = 61 L, has (nb - 1) L + 7 * 61 L + L =
(427 + nb) L, dense only when the chunk is the whole batch, and there span_to_stage runs with a
block stride below its shard stride. packed_split's span is exactly nb k L.) RS(2,1) and RS(5,3)
fall on the same side in every row; RS(20,10) does too except that its slack_split and word_slack
are dense at L = 33 as well (4 * span = 26020 <= 26400 at nb = 8, 199012 <= 201300 at nb = 61: the
16-byte gap weighs less on 20 shards), so span_to_stage also runs on 33-byte shards. XOR(2,1) and
XOR(3,1): packed_split linear both ways, interleaved 2D both ways, slack_split linear up at
L = 1202 and 2D at L = 33. In-place reconstruct uploads data the same way and always returns the
rebuilt shards through the library's own pinned buffer and a host scatter; its parity planes go up
by one 2D copy per plane that at least 3/4 of the chunk's blocks read, the others through
gather_planes_kernel reading the caller's mapped memory, so the masks below fix per chunk which
planes take which way. The tests assert bytes, not routes; a kernel trace of this module shows the
three kernels launched.

Masks at host_chunk = 8, per chunk of 8 blocks (scaled to m; at other chunk sizes the same masks
simply fall differently):
  0  6 of 8 blocks lose one data shard, all parity present: plane 0 exactly on the 3/4 threshold
  1  5 of 8 lose one data shard: plane 0 below the threshold
  2  complete blocks and parity-only losses: nothing to rebuild, nothing may change
  3  every block loses one data shard, every second one parity 0 too (m >= 2): planes 0 and 1 are
     each read by half of the blocks
  4  every block loses min(k, m) data shards: every plane dense, min(k, m) output slots
  5  0..m+1 losses anywhere: failing blocks among good ones
  6  every block has fewer than k shards present: all -4, nothing written
  7  (5 blocks) seeded random
and where k + m < 32 a third of the masks carry stray bits at and above k + m.
"""
import contextlib
import ctypes

import numpy as np
import pytest

from arena import CANARY, GUARD, MUL, check_arena, torch  # noqa: F401
from test_gpu_wide import erase_block, pick, ref_reconstruct

pytestmark = pytest.mark.gpu

ERASED = 0x5A
GAP = 80            # canary bytes between two regions of one arena
B = 61
WORD_GUARD = 64     # canary words on either side of a mask or status array
WORD_CANARY = 0x7B7B7B7B
UNSET = 99          # statuses before a call

LAYOUTS = ["packed_split", "slack_split", "word_slack", "interleaved", "shard_major_packed"]
RS_LENGTHS = {(8, 4): [1202, 33, 16, 7], (2, 1): [1202, 33], (5, 3): [1202, 33], (20, 10): [1202, 33]}


@pytest.fixture(scope="module")
def codec(fec):
    c = fec.Codec(0)
    yield c
    c.close()


# ------------------------------------------------------------------ arenas, regions, layouts

class Region:
    """Shard slots of L bytes at off + b*bs + r*ss (byte offsets into an arena), b < nb, r < rows."""

    def __init__(self, off, bs, ss, rows, nb, L):
        self.off, self.bs, self.ss, self.rows, self.nb, self.L = off, bs, ss, rows, nb, L

    def starts(self):
        return (self.off + np.arange(self.nb)[:, None] * self.bs + np.arange(self.rows)[None, :] * self.ss).ravel()

    def index(self):
        """[nb, rows, L] arena indices of bytes [0, L) of every slot."""
        return self.starts().reshape(self.nb, self.rows, 1) + np.arange(self.L)[None, None, :]

    def end(self):
        return int(self.starts().max()) + self.L


def place(lo, mod, res):
    """The first offset >= lo that is res mod `mod`."""
    return lo + (res - lo) % mod


def make_layout(name, k, m, L, nb, dres, pres):
    """(arena size, data region, parity region) of one layout. The arena's base is 16-byte aligned,
    so the data and parity bases land on addresses dres and pres mod 4 (word_slack: 4 mod 16)."""
    n = k + m
    if name == "packed_split":
        data = Region(place(GUARD, 4, dres), k * L, L, k, nb, L)
        par = Region(place(data.end() + GAP, 4, pres), m * L, L, m, nb, L)
    elif name == "slack_split":          # parity below the data
        ss = L + 7
        par = Region(place(GUARD, 4, pres), m * ss + 3, ss, m, nb, L)
        data = Region(place(par.end() + GAP, 4, dres), k * ss + 16, ss, k, nb, L)
    elif name == "word_slack":           # every shard address a multiple of 4 (the + 3 becomes + 4)
        ss = (L + 3) // 4 * 4 + 4
        par = Region(place(GUARD, 16, 4), m * ss + 4, ss, m, nb, L)
        data = Region(place(par.end() + GAP, 16, 4), k * ss + 16, ss, k, nb, L)
    elif name == "interleaved":
        ss = L + 3
        data = Region(place(GUARD, 4, dres), n * ss, ss, k, nb, L)
        par = Region(data.off + k * ss, n * ss, ss, m, nb, L)
    elif name == "shard_major_packed":
        data = Region(place(GUARD, 4, dres), L, nb * L, k, nb, L)
        par = Region(place(data.end() + GAP, 4, pres), L, nb * L, m, nb, L)
    else:
        raise ValueError(name)
    assert data.ss == par.ss
    starts = np.sort(np.concatenate([data.starts(), par.starts()]))
    assert starts[0] >= GUARD and (np.diff(starts) >= L).all(), "slots must not overlap"
    return max(data.end(), par.end()) + GUARD, data, par


_hip = []


def hip_runtime():
    """The HIP runtime this process already runs (the one the library is bound to), by ctypes."""
    if not _hip:
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
        assert len(paths) == 1, "one HIP runtime per process: %r" % paths
        rt = ctypes.CDLL(paths[0])
        rt.hipHostRegister.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint]
        rt.hipHostUnregister.argtypes = [ctypes.c_void_p]
        _hip.append(rt)
    return _hip[0]


@contextlib.contextmanager
def host_arena(kind, size, torch, fec):
    """(arena, flag): `size` canary bytes of host memory of one kind, the base 16-byte aligned."""
    if kind == "pinned":
        t = torch.from_numpy(np.full(size, CANARY, dtype=np.uint8)).pin_memory()
        arena = t.numpy()
        assert t.is_pinned() and arena.ctypes.data == t.data_ptr() and t.data_ptr() % 16 == 0
        yield arena, fec.FEC_HOST_PINNED
        return
    raw = np.full(size + 16, CANARY, dtype=np.uint8)
    skip = -raw.ctypes.data % 16
    arena = raw[skip:skip + size]
    if kind == "pageable":
        yield arena, fec.FEC_HOST
        return
    assert kind == "registered"
    rt = hip_runtime()
    assert rt.hipHostRegister(arena.ctypes.data, size, 0) == 0
    try:
        yield arena, fec.FEC_HOST_PINNED
    finally:
        assert rt.hipHostUnregister(arena.ctypes.data) == 0


def guarded_words(values):
    """(whole, view): a copy of `values` (4-byte words) between two runs of canary words."""
    values = np.ascontiguousarray(values)
    whole = np.full(values.size + 2 * WORD_GUARD, WORD_CANARY, dtype=values.dtype)
    view = whole[WORD_GUARD:WORD_GUARD + values.size]
    view[:] = values.ravel()
    return whole, view


def phases(kind, salt):
    """Address residues mod 4 of the data and parity bases: pinned 1, 2, 3 in turn over the cases,
    registered odd, pageable any."""
    if kind == "pinned":
        return 1 + salt % 3, 1 + (salt + 1) % 3
    if kind == "registered":
        return 1, 3
    return salt % 4, (salt + 3) % 4


# ------------------------------------------------------------------ the two checks every form shares

def scrub(arena, before, data, par, run, flags):
    """The library keeps its staging between calls, and the same shards at the same place of the
    stage would let a call that forgets an upload pass on what the call before it left there. So
    each checked call follows the same call on the complement of every shard byte, as FEC_HOST
    (whose staging copies share nothing with the pinned routes) and with the case's own flag;
    whatever that leaves in the stage is wrong everywhere. Then the arena is put back."""
    arena[data.index()] ^= 0xFF
    arena[par.index()] ^= 0xFF
    for flag in flags:
        run(flag)
    arena[:] = before


def check_encode(call, codec, fec, torch, kind, layout, k, m, L, nb, chunk, sh, salt):
    """call(nblocks, data, dbs, parity, pbs, ss, flag) -> rc encodes; sh [nb, k + m, L] holds the
    oracle's parity."""
    size, data, par = make_layout(layout, k, m, L, nb, *phases(kind, salt))
    with host_arena(kind, size, torch, fec) as (arena, flag):
        arena[data.index()] = sh[:, :k]
        before = arena.copy()
        model = before.copy()
        model[par.index()] = sh[:, k:]
        base = arena.ctypes.data
        where = (base + data.off, data.bs, base + par.off, par.bs, data.ss)
        args = where + (flag,)
        flags = sorted({fec.FEC_HOST, flag})
        old = codec.set_tuning(host_chunk=chunk)
        try:
            assert call(0, *args) == fec.FEC_OK
            check_arena(arena, before, "encode of no blocks")
            scrub(arena, before, data, par, lambda f: call(nb, *where, f), flags)
            rc = call(nb, *args)
        finally:
            codec.set_tuning(**old)
        assert rc == fec.FEC_OK
        check_arena(arena, model, "encode")
        assert codec.lib_sync_rc() == fec.FEC_OK


def check_reconstruct(call, codec, fec, torch, kind, layout, k, m, L, nb, chunk, c, salt):
    """call(nblocks, data, dbs, parity, pbs, ss, masks, status, flag) -> rc reconstructs in place.
    c: dmg [nb, k + m, L] (the damaged batch), masks (what the call gets), rebuilt [nb, k] (the
    data shards the call must write), rec [nb, k + m, L] (the reference's result), st_want [nb]."""
    size, data, par = make_layout(layout, k, m, L, nb, *phases(kind, salt))
    rebuilt, st_want = c["rebuilt"], c["st_want"]
    masks_all, masks = guarded_words(c["masks"])
    st_all, st = guarded_words(np.full(nb, UNSET, dtype=np.int32))
    masks_before = masks_all.copy()
    with host_arena(kind, size, torch, fec) as (arena, flag):
        arena[data.index()] = c["dmg"][:, :k]
        arena[par.index()] = c["dmg"][:, k:]
        before = arena.copy()
        model = before.copy()
        model[data.index()[rebuilt]] = c["rec"][:, :k][rebuilt]
        base = arena.ctypes.data
        where = (base + data.off, data.bs, base + par.off, par.bs, data.ss, masks.ctypes.data)
        flags = sorted({fec.FEC_HOST, flag})
        old = codec.set_tuning(host_chunk=chunk)
        try:
            assert call(0, *where, st.ctypes.data, flag) == fec.FEC_OK
            check_arena(arena, before, "reconstruct of no blocks")
            assert (st_all == np.int32(UNSET)).sum() == nb and (st == UNSET).all()
            scrub(arena, before, data, par, lambda f: call(nb, *where, None, f), flags)
            rc = call(nb, *where, st.ctypes.data, flag)
            sync_rc = codec.lib_sync_rc()
            got = arena.copy()
            scrub(arena, before, data, par, lambda f: call(nb, *where, None, f), flags)
            rc_null = call(nb, *where, None, flag)
            got_null = arena.copy()
        finally:
            codec.set_tuning(**old)
    failed = bool((st_want != 0).any())
    check_arena(got, model, "reconstruct")
    assert np.array_equal(st, st_want)
    assert rc == (fec.FEC_ERR_TOO_FEW_SHARDS if failed else fec.FEC_OK)
    assert (st_all[:WORD_GUARD] == WORD_CANARY).all() and (st_all[-WORD_GUARD:] == WORD_CANARY).all()
    assert np.array_equal(masks_all, masks_before)
    assert sync_rc == fec.FEC_OK          # the sticky word belongs to FEC_DEVICE calls
    assert rc_null == rc
    check_arena(got_null, model, "reconstruct without block_status")


# ------------------------------------------------------------------ RS, narrow

def rs_lost(rng, k, m):
    """bool [B, k + m], shard lost: the per-chunk plan of the module docstring."""
    n, top = k + m, min(k, m)
    lost = np.zeros((B, n), dtype=bool)

    def lose(b, count):
        lost[b, rng.choice(n, size=count, replace=False)] = True

    for b in range(0, 6):                         # chunk 0
        lost[b, (5 * b + 1) % k] = True
    for b in range(8, 13):                        # chunk 1
        lost[b, (3 * b + 2) % k] = True
    for b in range(17, 24, 2):                    # chunk 2: parity only
        lost[b, k + rng.choice(m, size=int(rng.integers(1, m + 1)), replace=False)] = True
    for b in range(24, 32):                       # chunk 3
        lost[b, (7 * b) % k] = True
        if m >= 2 and b % 2:
            lost[b, k] = True
    for b in range(32, 40):                       # chunk 4
        lost[b, rng.choice(k, size=top, replace=False)] = True
    lose(41, m + 1)                               # chunk 5: 40 complete, 41 and 45 fail, the rest seeded
    lose(45, m + 1)
    for b in (42, 43, 44, 46, 47):
        lose(b, int(rng.integers(0, m + 2)))
    for b in range(48, 56):                       # chunk 6
        lose(b, int(rng.integers(m + 1, min(n, m + 3) + 1)))
    for b in range(56, B):                        # chunk 7
        lose(b, int(rng.integers(0, m + 2)))
    return lost


_rs = {}


def rs_case(oracle, fec, k, m, L):
    """One (k, m, L), computed once and then read-only: the encoded batch, the masks, the damaged
    batch and the oracle's in-place reconstruct of it."""
    key = (k, m, L)
    if key not in _rs:
        n = k + m
        rng = np.random.default_rng(100000 * k + 1000 * m + L)
        sh = np.zeros((B, n, L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        lost = rs_lost(rng, k, m)
        e_d = lost[:, :k].sum(axis=1)
        few = (e_d > 0) & ((n - lost.sum(axis=1)) < k)
        # the plan holds: the chunks that choose a route have the losses they name
        assert list(e_d[0:8]) == [1] * 6 + [0] * 2 and not lost[0:8, k:].any()
        assert list(e_d[8:16]) == [1] * 5 + [0] * 3 and not lost[8:16, k:].any()
        assert not e_d[16:24].any() and lost[16:24, k:].any()
        assert (e_d[24:32] == 1).all() and lost[24:32, k].sum() == (4 if m >= 2 else 0)
        assert (e_d[32:40] == min(k, m)).all() and not few[:40].any()
        assert few[41] and few[45] and not few[40] and few[48:56].all()
        clean = (lost == 0).dot(1 << np.arange(n, dtype=np.uint64)).astype(np.uint32)
        masks = clean.copy()
        if n < 32:                                  # stray bits at and above n in a third of the masks
            high = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32) | np.uint32(1)
            stray = np.arange(B) % 3 == 1
            masks[stray] |= (high[stray].astype(np.uint64) << np.uint64(n)).astype(np.uint32)
            assert (masks[stray] >> n).all() and np.array_equal(masks & np.uint32((1 << n) - 1), clean)
        dmg = sh.copy()
        dmg[lost] = ERASED
        rec = dmg.copy()
        st_ref = oracle.rs_reconstruct(k, m, rec, clean)
        assert np.array_equal(st_ref != 0, few)
        rebuilt = lost[:, :k] & ~few[:, None]
        # the oracle gives back the original data and touches nothing else
        assert np.array_equal(rec[:, :k][rebuilt], sh[:, :k][rebuilt])
        untouched = np.ones((B, n), dtype=bool)
        untouched[:, :k] = ~rebuilt
        assert np.array_equal(rec[untouched], dmg[untouched])
        st_want = np.where(st_ref != 0, fec.FEC_ERR_TOO_FEW_SHARDS, 0).astype(np.int32)
        for a in (sh, masks, dmg, rec, rebuilt, st_want):
            a.setflags(write=False)
        _rs[key] = dict(sh=sh, masks=masks, dmg=dmg, rec=rec, rebuilt=rebuilt, st_want=st_want)
    return _rs[key]


def rs_runs():
    runs = []
    for (k, m), lengths in RS_LENGTHS.items():
        for li, L in enumerate(lengths):
            for chunk in (8, 0) + ((7,) if (k, m, L) == (8, 4, 1202) else ()):
                for yi, layout in enumerate(LAYOUTS):
                    for kind in ("pageable", "pinned"):
                        runs.append((kind, layout, k, m, L, chunk, li + yi + chunk))
    for yi, layout in enumerate(LAYOUTS):
        runs.append(("registered", layout, 8, 4, 1202, 8, yi))
    return [pytest.param(*r, id="%s-%s-rs%d_%d-L%d-chunk%d" % r[:6]) for r in runs]


@pytest.mark.parametrize("step", ["encode", "reconstruct"])
@pytest.mark.parametrize("kind,layout,k,m,L,chunk,salt", rs_runs())
def test_rs_host_call_writes_only_what_the_header_allows(codec, oracle, torch, fec, kind, layout, k, m, L, chunk,
                                                         salt, step):
    c = rs_case(oracle, fec, k, m, L)
    if step == "encode":
        def call(nb, data, dbs, parity, pbs, ss, flag):
            return codec.rs_encode_raw(k, m, L, nb, data, dbs, parity, pbs, ss, flag)   # raises unless FEC_OK
        check_encode(call, codec, fec, torch, kind, layout, k, m, L, B, chunk, c["sh"], salt)
    else:
        def call(nb, data, dbs, parity, pbs, ss, masks, status, flag):
            return codec.rs_reconstruct_raw(k, m, L, nb, data, dbs, parity, pbs, ss, masks, status, flag)
        check_reconstruct(call, codec, fec, torch, kind, layout, k, m, L, B, chunk, c, salt)


# ------------------------------------------------------------------ XOR(k, 1)

XOR_LAYOUTS = ["packed_split", "interleaved", "slack_split"]
_xor = {}


def xor_case(oracle, fec, k, L):
    """Blocks in turn: nothing lost, one data shard lost, parity lost only, a data shard and the
    parity lost, two data shards lost (the last two fail with -4 and stay as they are)."""
    key = (k, L)
    if key not in _xor:
        n = k + 1
        rng = np.random.default_rng(77 * k + L)
        sh = np.zeros((B, n, L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
        oracle.xor_encode(k, sh)
        kind = (np.arange(B) + np.arange(B) // 8) % 5        # every kind at every place of a chunk of 8
        lost = np.zeros((B, n), dtype=bool)
        for b in range(B):
            i = (b // 5) % k
            if kind[b] in (1, 3, 4):
                lost[b, i] = True
            if kind[b] in (2, 3):
                lost[b, k] = True
            if kind[b] == 4:
                lost[b, (i + 1) % k] = True
        masks = (lost == 0).dot(1 << np.arange(n, dtype=np.uint64)).astype(np.uint32)
        dmg = sh.copy()
        dmg[lost] = ERASED
        rec = dmg.copy()
        st_ref = oracle.xor_reconstruct(k, rec, masks)
        assert np.array_equal(st_ref != 0, kind >= 3)
        rebuilt = lost[:, :k] & (kind == 1)[:, None]
        assert rebuilt.sum() == (kind == 1).sum() and np.array_equal(rec[:, :k][rebuilt], sh[:, :k][rebuilt])
        untouched = np.ones((B, n), dtype=bool)
        untouched[:, :k] = ~rebuilt
        assert np.array_equal(rec[untouched], dmg[untouched])
        st_want = np.where(st_ref != 0, fec.FEC_ERR_TOO_FEW_SHARDS, 0).astype(np.int32)
        for a in (sh, masks, dmg, rec, rebuilt, st_want):
            a.setflags(write=False)
        _xor[key] = dict(sh=sh, masks=masks, dmg=dmg, rec=rec, rebuilt=rebuilt, st_want=st_want)
    return _xor[key]


@pytest.mark.parametrize("step", ["encode", "reconstruct"])
@pytest.mark.parametrize("chunk", [8, 0])
@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("layout", XOR_LAYOUTS)
@pytest.mark.parametrize("k,L", [(2, 1202), (2, 33), (3, 1202), (3, 33)])
def test_xor_host_call_writes_only_what_the_header_allows(codec, oracle, torch, fec, k, L, layout, kind, chunk, step):
    c = xor_case(oracle, fec, k, L)
    h = codec.handle
    salt = XOR_LAYOUTS.index(layout) + k + L + chunk
    if step == "encode":
        def call(nb, data, dbs, parity, pbs, ss, flag):
            return fec.lib.fec_xor_encode_batch(h, k, L, nb, data, dbs, parity, pbs, ss, flag)
        check_encode(call, codec, fec, torch, kind, layout, k, 1, L, B, chunk, c["sh"], salt)
    else:
        def call(nb, data, dbs, parity, pbs, ss, masks, status, flag):
            return fec.lib.fec_xor_reconstruct_batch(h, k, L, nb, data, dbs, parity, pbs, ss, masks, status, flag)
        check_reconstruct(call, codec, fec, torch, kind, layout, k, 1, L, B, chunk, c, salt)


# ------------------------------------------------------------------ RS, wide (two mask words)

WIDE_B = 9
_wide = {}


def wide_case(oracle, fec, MUL, L):
    """RS(40,20), the erasure counts of test_gpu_wide.test_wide_host_form (the last block has
    k - 1 shards present) against its inverse-matrix reference."""
    if L not in _wide:
        k, m = 40, 20
        n = k + m
        rng = np.random.default_rng(4020 + L)
        present = np.array([erase_block(rng, k, m, e) for e in [0, 1, 16, 17, min(k, m), 2, 3, 5]] +
                           [np.zeros(n, dtype=bool)])
        present[-1, pick(rng, range(n), k - 1)] = True
        assert len(present) == WIDE_B
        sh = np.zeros((WIDE_B, n, L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (WIDE_B, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        dmg = sh.copy()
        dmg[~present] = ERASED
        # the reference works on 16-byte slots (it zeroes a rebuilt shard's padding)
        wide = np.zeros((WIDE_B, n, (L + 15) // 16 * 16), dtype=np.uint8)
        wide[:, :, :L] = dmg
        st_ref = ref_reconstruct(oracle, MUL, k, m, wide, present, L)
        rec = np.ascontiguousarray(wide[:, :, :L])
        assert list(st_ref) == [0] * 8 + [-4]
        rebuilt = ~present[:, :k] & (st_ref == 0)[:, None]
        assert np.array_equal(rec[:, :k][rebuilt], sh[:, :k][rebuilt])
        untouched = np.ones((WIDE_B, n), dtype=bool)
        untouched[:, :k] = ~rebuilt
        assert np.array_equal(rec[untouched], dmg[untouched])
        st_want = np.where(st_ref != 0, fec.FEC_ERR_TOO_FEW_SHARDS, 0).astype(np.int32)
        masks = fec.wide_masks(present)
        assert masks.shape == (WIDE_B, 2)
        for a in (masks, dmg, rec, rebuilt, st_want):
            a.setflags(write=False)
        _wide[L] = dict(masks=masks, dmg=dmg, rec=rec, rebuilt=rebuilt, st_want=st_want)
    return _wide[L]


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("layout", ["interleaved", "slack_split"])
@pytest.mark.parametrize("L", [1202, 33])
def test_wide_host_call_writes_only_what_the_header_allows(codec, oracle, torch, fec, MUL, L, layout, kind, chunk):
    k, m = 40, 20
    c = wide_case(oracle, fec, MUL, L)

    def call(nb, data, dbs, parity, pbs, ss, masks, status, flag):
        return codec.rs_reconstruct_wide_raw(k, m, L, nb, data, dbs, parity, pbs, ss, masks, 2, status, flag)
    check_reconstruct(call, codec, fec, torch, kind, layout, k, m, L, WIDE_B, chunk, c, L + chunk + len(layout))


_wide_fail_first = {}


def wide_fail_first_case(oracle, fec, MUL):
    """RS(31,2), 33 shards, so two mask words and the wide route; L = 17. Block 0 has k - 1 shards
    present (a data shard and both parity shards lost) and fails; blocks 1 and 2 each lose one data
    shard, block 2 parity 0 as well, so it reads the shard of the second mask word."""
    if not _wide_fail_first:
        k, m, L, nb = 31, 2, 17, 3
        n = k + m
        rng = np.random.default_rng(3102)
        present = np.ones((nb, n), dtype=bool)
        present[0, [3, k, k + 1]] = False
        present[1, 30] = False
        present[2, [0, k]] = False
        assert present[0].sum() == k - 1 and list((~present[:, :k]).sum(axis=1)) == [1, 1, 1]
        sh = np.zeros((nb, n, L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (nb, k, L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        dmg = sh.copy()
        dmg[~present] = ERASED
        wide = np.zeros((nb, n, (L + 15) // 16 * 16), dtype=np.uint8)
        wide[:, :, :L] = dmg
        st_ref = ref_reconstruct(oracle, MUL, k, m, wide, present, L)
        rec = np.ascontiguousarray(wide[:, :, :L])
        assert list(st_ref) == [-4, 0, 0]
        rebuilt = ~present[:, :k] & (st_ref == 0)[:, None]
        assert rebuilt.sum() == 2 and np.array_equal(rec[:, :k][rebuilt], sh[:, :k][rebuilt])
        untouched = np.ones((nb, n), dtype=bool)
        untouched[:, :k] = ~rebuilt
        assert np.array_equal(rec[untouched], dmg[untouched])
        st_want = np.where(st_ref != 0, fec.FEC_ERR_TOO_FEW_SHARDS, 0).astype(np.int32)
        masks = fec.wide_masks(present)
        assert masks.shape == (nb, 2)
        for a in (masks, dmg, rec, rebuilt, st_want):
            a.setflags(write=False)
        _wide_fail_first.update(masks=masks, dmg=dmg, rec=rec, rebuilt=rebuilt, st_want=st_want)
    return _wide_fail_first


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_wide_host_failing_block_before_clean_chunks(codec, oracle, torch, fec, MUL, kind):
    """Chunks of one block: the failing block is the first chunk, and two chunks that rebuild follow
    it. check_reconstruct runs the call with block_status given and with NULL: both return
    FEC_ERR_TOO_FEW_SHARDS, the statuses are [-4, 0, 0], the arena equals the model, fec_sync is
    FEC_OK."""
    k, m, L = 31, 2, 17
    c = wide_fail_first_case(oracle, fec, MUL)
    assert list(c["st_want"]) == [fec.FEC_ERR_TOO_FEW_SHARDS, 0, 0]

    def call(nb, data, dbs, parity, pbs, ss, masks, status, flag):
        return codec.rs_reconstruct_wide_raw(k, m, L, nb, data, dbs, parity, pbs, ss, masks, 2, status, flag)
    check_reconstruct(call, codec, fec, torch, kind, "slack_split", k, m, L, 3, 1, c, 1)
