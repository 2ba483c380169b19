"""The guarded arena of the device oracle tests (test_gpu_*.py): a batch lives in one canary-filled
byte image with guards at both ends, its shard slots placed by regions with slack and gaps, and after
a call the WHOLE image is compared with a model. Here: the regions, the device layouts, the image, the
comparison, the encoded batch that verify, locate and locate-multi start from (encoded_arena: parity
by the device's encode; oracle_arena: the same image with the oracle's parity, built without a device,
which test_gpu_row_sweep.py starts from), and the fixtures the test modules import by name.
test_arena.py checks this module on the CPU.
"""
import numpy as np
import pytest

CANARY = 0xC7
GUARD = 256
STALE = 0x7EADBEEF          # what an output word holds before a call

LAYOUTS = ["interleaved", "interleaved_slack", "split", "split_parity_first", "shard_major", "shard_major_split"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU test needs a HIP device"
    return t


@pytest.fixture(scope="module")
def codec(fec):
    c = fec.Codec(0).use_torch_stream()
    yield c
    c.close()


@pytest.fixture(scope="module")
def MUL(oracle):
    """The oracle's field: MUL[a, b] = gf_mul(a, b)."""
    t = np.zeros((256, 256), dtype=np.uint8)
    for a in range(256):
        for b in range(a, 256):
            t[a, b] = t[b, a] = oracle.gf_mul(a, b)
    return t


@pytest.fixture(scope="module")
def gf(oracle):
    """The oracle's field: MUL[a, b] = gf_mul(a, b), INV[a] (INV[0] = 0)."""
    mul = np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    inv = np.zeros(256, dtype=np.uint8)
    a, b = np.nonzero(mul == 1)
    inv[a] = b
    return mul, inv


def rup16(x):
    return (x + 15) // 16 * 16


class Region:
    """Shard slots at off + b*bs + r*ss (byte offsets into an arena) of B blocks of `rows` shards."""

    def __init__(self, off, bs, ss, rows, B):
        self.off, self.bs, self.ss, self.rows, self.B = off, bs, ss, rows, B
        assert off % 16 == 0 and bs % 16 == 0 and ss % 16 == 0

    def at(self, b, r):
        return self.off + b * self.bs + r * self.ss

    def index(self, lo, hi):
        """[B, rows, hi - lo] arena indices of bytes [lo, hi) of every slot."""
        return (self.off + np.arange(self.B)[:, None, None] * self.bs +
                np.arange(self.rows)[None, :, None] * self.ss + np.arange(lo, hi)[None, None, :])

    def view(self, img, lo=0, hi=None):
        """Bytes [lo, hi) of every slot (default: all ss) as a [B, rows, hi - lo] view of the arena, writable
        if the arena is (slots do not overlap)."""
        hi = self.ss if hi is None else hi
        assert self.end() <= img.size and hi <= self.ss
        v = np.lib.stride_tricks.as_strided(img[self.off:], (self.B, self.rows, self.ss), (self.bs, self.ss, 1),
                                            writeable=img.flags.writeable)
        return v[:, :, lo:hi]

    def end(self):
        """One past the last byte of the last slot, each slot taken as ss bytes (the header asks for
        every slot to be readable over its whole shard stride); a region without rows ends as one of
        one row does."""
        return self.off + (self.B - 1) * self.bs + max(self.rows - 1, 0) * self.ss + self.ss


def place(name, k, m, L, B):
    """(data region, parity region) of a device layout: slots with slack, block strides with gaps,
    every offset and stride a multiple of 16, the first slot at GUARD."""
    R = rup16(L)
    if name in ("interleaved", "interleaved_slack"):
        ss = R + 32
        bs = (k + m) * ss + 48
        data = Region(GUARD, bs, ss, k, B)
        par = Region(GUARD + k * ss, bs, ss, m, B)
    elif name in ("split", "split_parity_first"):   # parity below the data in memory
        ss = R + 16
        par = Region(GUARD, m * ss + 16, ss, m, B)
        data = Region(par.end() + 80, k * ss + 48, ss, k, B)
    elif name == "shard_major":                     # [k + m][B] slots
        sp = R + 16
        ss = B * sp
        data = Region(GUARD, sp, ss, k, B)
        par = Region(GUARD + k * ss, sp, ss, m, B)
    elif name == "shard_major_split":               # parity below the data, not a whole shard stride apart
        sp = R + 16
        ss = B * sp
        par = Region(GUARD, sp, ss, m, B)
        gap = 208
        assert gap % ss != 0
        data = Region(GUARD + m * ss + gap, sp, ss, k, B)
    else:
        raise ValueError(name)
    assert data.ss == par.ss
    return data, par


def canary_image(regions):
    """An arena of canary bytes that holds the regions with at least GUARD bytes after the last slot
    (and before the first: the regions are placed so)."""
    assert min(r.off for r in regions) >= GUARD
    return np.full(max(r.end() for r in regions) + GUARD, CANARY, dtype=np.uint8)


def check_arena(got, model, what):
    if not np.array_equal(got, model):
        bad = np.flatnonzero(got != model)
        raise AssertionError("%s: %d bytes differ from the model, first at arena offset %d (got 0x%02x, want 0x%02x)"
                             % (what, bad.size, bad[0], got[bad[0]], model[bad[0]]))


def encoded_arena(codec, fec, torch, layout, k, m, L, B, rng):
    """(image, data region, parity region) of an encoded batch: bytes [0, L) of the data slots drawn
    from rng, the parity made by fec_rs_encode_batch on the device, and its zero pad put back to canary
    (the parity slots too hold canary from L on)."""
    data, par = place(layout, k, m, L, B)
    img = canary_image([data, par])
    img[data.index(0, L)] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    if m:
        dev = torch.from_numpy(img).cuda()
        p = dev.data_ptr()
        assert p % 16 == 0
        assert fec.lib.fec_rs_encode_batch(codec.handle, k, m, L, B, p + data.off, data.bs, p + par.off, par.bs,
                                           data.ss, fec.FEC_DEVICE) == fec.FEC_OK
        assert codec.lib_sync_rc() == fec.FEC_OK
        img = dev.cpu().numpy()
        pad = par.index(L, rup16(L))
        assert (img[pad] == 0).all()
        img[pad] = CANARY
    return img, data, par


def oracle_arena(oracle, layout, k, m, L, B, rng):
    """encoded_arena without a device: the same regions, canaries and data bytes (the same draws from
    rng), the parity over [0, L) taken from oracle.rs_encode, canary from L on. A test that starts from
    this image does not rest on the library's own encode."""
    data, par = place(layout, k, m, L, B)
    img = canary_image([data, par])
    sh = np.zeros((B, k + m, L), dtype=np.uint8)
    sh[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    img[data.index(0, L)] = sh[:, :k]
    if m:
        oracle.rs_encode(k, m, sh)
        img[par.index(0, L)] = sh[:, k:]
    return img, data, par


def shards(img, data, par):
    """[B, k + m, ss] copy of the arena's data and parity slots."""
    out = np.empty((data.B, data.rows + par.rows, data.ss), dtype=np.uint8)
    out[:, :data.rows] = img[data.index(0, data.ss)]
    if par.rows:
        out[:, data.rows:] = img[par.index(0, data.ss)]
    return out


# ---------------------------------------------------------------- models shared by the near and the far tests

def recover_statuses(fec, e_d, few, slots):
    """What a recover call reports per block: the erased data shards rebuilt, or why none was."""
    return np.where(e_d == 0, 0, np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS,
                                          np.where(e_d > slots, fec.FEC_ERR_INVALID_ARG, e_d)))


def folded_parity(oracle, k, m, delta, cols, parity):
    """Update / encode-idx: parity [B, m, L] ^ the oracle's encode of delta [B, k, L] with every column
    outside cols (bool [B, k]) zero; blocks with no column keep their parity."""
    Bn, _, L = delta.shape
    D = np.zeros((Bn, k + m, L), dtype=np.uint8)
    D[:, :k] = delta * cols[:, :, None]
    oracle.rs_encode(k, m, D)
    out = parity.copy()
    hit = cols.any(axis=1)
    out[hit] = parity[hit] ^ D[hit, k:]
    return out
