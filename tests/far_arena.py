"""The sparse far arena of test_gpu_far_offsets.py: several GiB of canary bytes that live on the device
only. The host models the windows of a case (the first `win` bytes of every shard slot of every region
the call is given, far_cases.FarLayout): it writes their bytes before the call with small copies,
reads them back after it and compares them with the model byte for byte; then it puts the windows back
to canary and asserts, on the device, that the WHOLE arena is canary. That is the whole-arena guarantee
of arena.check_arena: a store that went to a wrapped address is found wherever it landed.
"""
import numpy as np
import pytest

import far_cases
from arena import CANARY

_WORD = int(np.frombuffer(bytes([CANARY]) * 8, dtype=np.int64)[0])
_SCAN = 1 << 25      # int64 words per compared chunk: a 32 MiB temporary


class FarArena:
    def __init__(self, t, size):
        assert size % 8 == 0 and size <= far_cases.CAP
        self.t, self.size = t, size
        self.dev = t.full((size,), CANARY, dtype=t.uint8, device="cuda")
        self.ptr = self.dev.data_ptr()
        assert self.ptr % 16 == 0

    def addr(self, region):
        return self.ptr + region.off

    def window(self, r):
        """The [B, rows, win] strided view of a region's windows."""
        assert r.end() <= self.size
        return self.t.as_strided(self.dev, (r.B, r.rows, r.win), (r.bs, r.ss, 1), r.off)

    def blank(self, lay):
        """Host windows of a layout, all canary: name -> uint8 [B, rows, win]."""
        return {name: np.full((r.B, r.rows, r.win), CANARY, dtype=np.uint8) for name, r in lay.regions.items()}

    def write(self, lay, wins):
        for name, r in lay.regions.items():
            if r.rows:
                self.window(r).copy_(self.t.from_numpy(wins[name]).cuda())

    def read(self, lay):
        return {name: (self.window(r).cpu().numpy() if r.rows else np.empty((r.B, 0, r.win), dtype=np.uint8))
                for name, r in lay.regions.items()}

    def first_dirty(self):
        """The lowest arena offset that does not hold the canary, or None."""
        t = self.t
        words = self.dev.view(t.int64)
        dirty = t.stack([(words[i:i + _SCAN] != _WORD).any() for i in range(0, words.numel(), _SCAN)]).cpu().numpy()
        if not dirty.any():
            return None
        i = int(np.flatnonzero(dirty)[0]) * _SCAN
        w = i + int((words[i:i + _SCAN] != _WORD).nonzero()[0, 0])
        got = self.dev[8 * w:8 * w + 8].cpu().numpy()
        return 8 * w + int(np.flatnonzero(got != CANARY)[0])

    def check(self, lay, model, what):
        """The windows against the model, then the windows back to canary and every byte of the arena
        against the canary."""
        got = self.read(lay)
        for r in lay.regions.values():
            if r.rows:
                self.window(r).fill_(CANARY)
        bad = []
        for name, r in lay.regions.items():
            ne = np.argwhere(got[name] != model[name])
            if len(ne):
                b, j, x = (int(v) for v in ne[0])
                bad.append((r.at(b, j) + x, len(ne), name, b, j, x, got[name][b, j, x], model[name][b, j, x]))
        stray = self.first_dirty()
        if stray is not None:
            self.dev.fill_(CANARY)       # the next test starts from a clean arena
        bases = ", ".join("%s 0x%x" % nb for nb in sorted(lay.bases().items()))
        if bad:
            off, _, name, b, j, x, g, w = min(bad)
            raise AssertionError("%s: %d bytes differ from the model, first at arena offset %d = 0x%x (%s, block %d, "
                                 "slot %d, byte %d: got 0x%02x, want 0x%02x); first byte written outside every "
                                 "window: %s (bases: %s)"
                                 % (what, sum(v[1] for v in bad), off, off, name, b, j, x, g, w,
                                    "none" if stray is None else "0x%x" % stray, bases))
        if stray is not None:
            raise AssertionError("%s: a byte outside every window was written, first at arena offset %d = 0x%x "
                                 "(bases: %s)" % (what, stray, stray, bases))


@pytest.fixture(scope="module")
def far(torch):
    """The module's arena, as large as the cases need by the rule of far_cases.py."""
    size = far_cases.arena_bytes()
    assert size <= 12 << 30
    a = FarArena(torch, size)
    yield a
    a.dev = None
    del a
    torch.cuda.empty_cache()
