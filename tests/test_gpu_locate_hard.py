"""fec_rs_locate_multi_batch and fec_rs_locate_partial_batch on the device, on the adversarial batches
of locate_hard_cases.py: blocks beyond the radius with no cap on the corrupt shards, miscorrections to
a disjoint set, locators with a root outside the code or at a missing shard, zero pivots, and merges
over chunks and waves, in codes of up to 256 shards at the full radius. The expected results are the
Berlekamp-Welch model's (locate_model.py), which test_locate_hard_cases.py holds against every
construction and against the siblings' brute force.

The guarded-arena method and the call paths are those of test_gpu_locate_multi.py and
test_gpu_locate_partial.py (Batch.locate, PBatch.locate): outputs pre-filled with a stale value, the
whole arena compared with its image before the call, bad_count, present_out at the minimum word count
and at 8 words, and the counts. Then the heal loop, fec_rs_reconstruct_some_batch for n <= 32 and
fec_rs_reconstruct_some_wide_batch above, with the whole arena compared again: a located block holds
its original bytes in every shard, a miscorrected one (class b) the codeword clean ^ c, which
fec_rs_verify_batch passes; an unknown block's present shards are untouched.

The same runs under the Cauchy code (a ctx with FEC_MATRIX_CAUCHY): the batches of
locate_hard_cases.params(cauchy=True), whose clean codewords are cauchy_oracle's and whose zero pivots,
pseudo-roots and miscorrections are built with the weights u_r / v_r, so they are the hard cases of
that code; fec_rs_locate_batch is held to model_verdicts over the Cauchy matrix. The codes: k a power
of two and not, m odd, and 40 and 256 shards, which heal through rs_plan_wide_kernel<true>.
"""
import numpy as np
import pytest

import cauchy_oracle
from arena import STALE, check_arena, codec, gf, rup16, torch  # noqa: F401
from locate_hard_cases import cases, params
from locate_model import UNKNOWN
from test_gpu_locate import model_verdicts
from test_gpu_locate_multi import Batch
from test_gpu_locate_partial import PBatch

pytestmark = pytest.mark.gpu

LAYOUTS = ["interleaved", "split"]


@pytest.fixture(scope="module")
def cauchy_codec(fec):
    c = fec.Codec(0, matrix="cauchy").use_torch_stream()
    assert c.matrix == "cauchy"
    yield c
    c.close()


class Hard:
    """What the two calls' batches share: the arena of a Cases in a layout, and the heal loop."""

    def setup(self, codec, fec, torch, oracle, gf, cs, layout):
        self.codec, self.fec, self.torch, self.oracle, self.gf, self.cs = codec, fec, torch, oracle, gf, cs
        self.k, self.m, self.n, self.L, self.B, self.max_bad = cs.k, cs.m, cs.n, cs.L, cs.B, cs.max_bad
        self.img, self.clean, self.data, self.par = cs.arena(layout)
        self.img.setflags(write=False)
        self.want, self.sets = cs.want, cs.sets

    def slot(self, b, s):
        return self.data.at(b, s) if s < self.k else self.par.at(b, s - self.k)

    def heal(self, dev, got, pm, W):
        """The reconstruct with the masks the locate call wrote, against a model of the whole arena."""
        fec, cs, p, k, L = self.fec, self.cs, dev.data_ptr(), self.k, self.L
        before = dev.cpu().numpy()
        st = self.torch.full((self.B,), 99, dtype=self.torch.int32, device="cuda")
        args = (self.codec.handle, k, self.m, L, self.B, p + self.data.off, self.data.bs, p + self.par.off,
                self.par.bs, self.data.ss, pm.data_ptr(), None)
        if self.n <= 32:
            assert W == 1
            rc = fec.lib.fec_rs_reconstruct_some_batch(*args, st.data_ptr(), fec.FEC_DEVICE)
        else:
            rc = fec.lib.fec_rs_reconstruct_some_wide_batch(*args, W, st.data_ptr(), fec.FEC_DEVICE)
        assert rc == fec.FEC_OK and self.codec.lib_sync_rc() == fec.FEC_OK
        assert (st.cpu().numpy() == 0).all()
        after = dev.cpu().numpy()
        model = before.copy()
        pad = np.zeros(rup16(L) - L, dtype=np.uint8)
        for b in range(self.B):
            for s in sorted(cs.miss[b] | (set(self.sets[b]) if got[b] > 0 else set())):
                at = self.slot(b, s)
                if got[b] == UNKNOWN:      # rebuilt from k shards of an inconsistent block: not modelled
                    model[at:at + rup16(L)] = after[at:at + rup16(L)]
                else:
                    model[at:at + L] = cs.final[b, s]
                model[at + L:at + rup16(L)] = pad
        check_arena(after, model, "heal")
        healed = self.shards(after)[:, :, :L]
        ok = got >= 0
        assert np.array_equal(healed[ok], cs.final[ok]), "located and clean blocks hold the codeword expected"
        mis = [b for b in range(self.B) if cs.kind[b] == "b"]
        assert mis and all(got[b] > 0 and not np.array_equal(cs.final[b], cs.clean[b]) for b in mis)
        for b in np.flatnonzero(~ok):
            has = sorted(set(range(self.n)) - cs.miss[b])
            assert np.array_equal(healed[b, has], cs.bad[b, has]), "an unknown block's present shards are untouched"
        status = self.torch.full((self.B,), 99, dtype=self.torch.int32, device="cuda")
        assert fec.lib.fec_rs_verify_batch(self.codec.handle, k, self.m, L, self.B, p + self.data.off, self.data.bs,
                                           p + self.par.off, self.par.bs, self.data.ss, status.data_ptr(), None,
                                           fec.FEC_DEVICE) == fec.FEC_OK
        assert self.codec.lib_sync_rc() == fec.FEC_OK
        status = status.cpu().numpy()
        assert (status[ok] == 1).all(), "every healed block verifies, the miscorrected ones included"
        if not any(cs.miss):
            assert (status[~ok] == 0).all()


class HardMulti(Hard, Batch):
    def __init__(self, *a):
        self.setup(*a)

    def run(self):
        fec, cs = self.fec, self.cs
        Wmin = fec.mask_words(self.n)
        dev = self.upload()
        self.locate(dev, Wmin, what="minimum mask words")
        self.locate(dev, 8, counts=False, what="8 mask words, no counts")
        self.single(dev, Wmin)
        W = 1 if self.n <= 32 else Wmin
        got, pm = self.locate(dev, W, what="heal: locate")
        self.heal(dev, got, pm, W)
        want2 = np.where(got > 0, 0, got).astype(np.int32)
        self.locate(dev, W, want=want2, what="heal: second locate")

    def single(self, dev, W):
        """fec_rs_locate_batch on the same arena against its own model; a block whose sums are those of
        one error at a point outside the code is unknown."""
        fec, torch, cs, p = self.fec, self.torch, self.cs, dev.data_ptr()
        out = torch.full((self.B,), 99, dtype=torch.int32, device="cuda")
        assert fec.lib.fec_rs_locate_batch(self.codec.handle, self.k, self.m, self.L, self.B, p + self.data.off,
                                           self.data.bs, p + self.par.off, self.par.bs, self.data.ss, out.data_ptr(),
                                           None, W, None, fec.FEC_DEVICE) == fec.FEC_OK
        assert self.codec.lib_sync_rc() == fec.FEC_OK
        out = out.cpu().numpy()
        assert np.array_equal(out, model_verdicts(self.oracle, self.gf, self.k, self.m, cs.bad, self.L))
        one = [b for b in range(self.B) if cs.kind[b] == "c" and cs.v[b] == 1]
        assert (out[one] == fec.FEC_LOCATE_UNKNOWN).all() and (one or self.n == 256)


class HardPartial(Hard, PBatch):
    def __init__(self, *a):
        self.setup(*a)
        cs, B = self.cs, self.B
        self.kinds, self.few = cs.kind, np.zeros(B, dtype=bool)
        rng = np.random.default_rng(cs.seed + 2)
        bits = np.zeros((B, 256), dtype=np.uint8)
        bits[:, :self.n] = 1
        for b in range(B):
            bits[b, sorted(cs.miss[b])] = 0
            if b % 3 == 0:
                bits[b, self.n:] = rng.integers(0, 2, 256 - self.n)   # stray bits at and above n: ignored
        self.bits = bits

    def expect(self, max_bad):
        assert max_bad == self.cs.max_bad
        return self.want, self.sets

    def run(self):
        fec, mb = self.fec, self.max_bad
        Wmin = fec.mask_words(self.n)
        dev = self.upload()
        self.locate(dev, Wmin, max_bad=mb, what="minimum mask words")
        self.locate(dev, 8, counts=False, max_bad=mb, what="8 mask words, no counts")
        W = 1 if self.n <= 32 else Wmin
        got, pm, _ = self.locate(dev, W, max_bad=mb, what="heal: locate")
        self.heal(dev, got, pm, W)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call,k,m,L,max_bad", params())
def test_locate_hard_cases_and_heal(codec, torch, fec, oracle, gf, call, k, m, L, max_bad, layout):
    cs = cases(oracle, gf, call, k, m, L, max_bad)
    (HardMulti if call == "multi" else HardPartial)(codec, fec, torch, oracle, gf, cs, layout).run()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("call,k,m,L,max_bad", params(cauchy=True))
@pytest.mark.parametrize("matrix", ["cauchy"])
def test_locate_hard_cases_and_heal_under(cauchy_codec, torch, fec, gf, matrix, call, k, m, L, max_bad, layout):
    assert np.array_equal(gf[0], cauchy_oracle.gf()[0])
    cs = cases(cauchy_oracle, gf, call, k, m, L, max_bad, cauchy_oracle.code_multipliers(k, m))
    (HardMulti if call == "multi" else HardPartial)(cauchy_codec, fec, torch, cauchy_oracle, gf, cs, layout).run()
