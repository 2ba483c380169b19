"""Model-based sequences over the whole device ABI (test_seq_model.py on the CPU, test_gpu_sequences.py
on the device): every FEC_DEVICE entry point is asynchronous and ordered on the ctx stream, and calls
of different kinds share state there (the plan workspace, the route word, the sticky error word, the
stream-side presets, masks handed from one call to the next in device memory). A program queues 12-16
steps over three live batches back to back; each step has a device form (Device) and an exact numpy
model (Batch) that acts on the batch's CPU image with the oracle alone.

  POOL        the live batches: the smallest shapes that still reach each kernel family
  Batch       one batch: a canary arena with guards (tests/arena.py), an out arena for the recover
              calls, a second arena that holds the new data of update, and one arena of words (masks,
              statuses, verdicts, counts, present masks, column masks, lengths) with canary words
              between its arrays; and the model of every step
  program     the seeded generator; N_PROGRAMS seeds give the coverage test_seq_model.py asserts
  Trace       a program run on the model alone: per step the inputs the device form needs, the sticky
              code, and the images after it
  Device      the same program on a ctx, queued with no host wait, or synced after every step
"""
from collections import namedtuple

import numpy as np

from arena import CANARY, GUARD, STALE, Region, canary_image, check_arena, place, rup16
from test_gpu_ragged import PATTERN

N_PROGRAMS = 48          # seeds 0..47 meet every coverage condition of test_seq_model.py

ERASED = 0x5A
CANARY32 = 0xC7C7C7C7
WGUARD = 4               # canary words on both sides of every word array
OK, TOO_FEW, INVALID, SHARD_SIZE = 0, -4, -1, -5
CLEAN = -1               # FEC_LOCATE_CLEAN
NEW_FLIP = 0x3C          # update: the new arena's used columns are changed by this after the call

Spec = namedtuple("Spec", "id kind k m L B layout")
POOL = {s.id: s for s in [
    Spec("A", "rs", 8, 4, 1202, 257, "interleaved_slack"),
    Spec("B", "rs", 20, 10, 1202, 67, "split_parity_first"),
    Spec("C", "rs", 16, 8, 513, 131, "shard_major"),
    Spec("D", "rs", 6, 3, 33, 67, "interleaved"),
    Spec("E", "rs", 10, 22, 200, 67, "split"),
    Spec("F", "rs", 33, 20, 97, 37, "interleaved"),
    Spec("G", "xor", 3, 1, 1202, 67, "interleaved_slack"),
    Spec("H", "ragged", 8, 4, 1202, 67, "interleaved"),
]}

# The users of Work::d_plans (fec_cores.cpp): who writes and reads records there.
USERS = ["block", "sorted2", "sorted3", "routed", "wide", "some", "ragged", "lmulti"]
# The batches on which a user can be reached, and the call that reaches it there.
USER_BATCHES = {"block": "DE", "sorted2": "A", "sorted3": "BC", "routed": "A", "wide": "F", "some": "DABCE",
                "ragged": "H", "lmulti": "DABC"}
SMALL_PLANS, LARGE_PLANS = "D", "AC"      # plan_bytes: every user of D stays under 4 KB, the decodes of A and C need 12-21 KB

KINDS = ["encode", "xor_encode", "ragged_encode", "erase", "reconstruct", "recover", "ragged_reconstruct",
         "ragged_recover", "xor_reconstruct", "reconstruct_wide", "recover_wide", "reconstruct_some", "verify",
         "update", "encode_idx", "corrupt", "locate", "locate_multi", "heal", "host_call", "sync"]
TORCH_ONLY = ("erase", "corrupt")     # the caller's own kernels: not library calls

Step = namedtuple("Step", "kind batch args")


def worst(codes):
    """The code fec_sync reports for the sticky word after these step codes."""
    for c in (TOO_FEW, INVALID, SHARD_SIZE):
        if c in codes:
            return c
    return OK


def user_of(step):
    """The workspace user a step's library call is (fec_cores.cpp's dispatch at default knobs), or None."""
    if step.batch is None:
        return None
    s = POOL[step.batch]
    cps = (s.L + 15) // 16
    kind = step.kind
    if kind in ("reconstruct", "recover"):
        if kind == "recover" and step.args["slots"] == 1 and cps >= 32:
            return None                                   # the direct kernel: no plan records
        if cps < 32:
            return "block"
        if kind == "reconstruct" and s.k == 8 and s.m >= 2:
            return "routed"
        return "sorted3" if (s.k, s.m) in ((16, 8), (20, 10)) else "sorted2"
    if kind in ("reconstruct_wide", "recover_wide"):
        return "wide"
    if kind == "heal":
        return "some" if s.k + s.m <= 32 else "wide"
    return {"reconstruct_some": "some", "ragged_reconstruct": "ragged", "ragged_recover": "ragged",
            "locate_multi": "lmulti"}.get(kind)


def plan_bytes(step):
    """The workspace bytes a step's call asks grow_plans for (0: none), by the record layouts of
    fec_kernels.hip (plan_layout), fec_wide.hpp (wide_layout) and fec_locate_multi.hpp (one bitmap bit per
    chunk in 32-byte units, then words + 1 words per block): what decides whether a call reallocates the
    workspace in the middle of the queue."""
    u = user_of(step)
    if u is None:
        return 0
    s = POOL[step.batch]
    k, m, B = s.k, s.m, s.B
    maxe = max(1, min(k, m))

    def narrow(sorted_):
        nout = (k + 7) // 8 * 8 + maxe
        coef = (nout + 4) // 4 * 4 + 4 if sorted_ else (nout + 4) // 4 * 4
        return rup16(coef + maxe * k)

    def wide(rows):
        return rup16(rup16((k + 7) // 8 * 8 + rows + 1) + rows * k)

    if u == "lmulti":
        cps, words = (s.L + 15) // 16, (k + m + 31) // 32
        return (B * cps + 255) // 256 * 32 + rup16(B * (words + 1) * 4)
    if u == "wide":
        return B * wide(min(maxe, step.args.get("slots", maxe)))
    if u == "some":
        return B * wide(max(m, 1))
    return B * narrow(u in ("sorted2", "sorted3", "routed"))


def bits_to_words(bits, W):
    """bool [B, n] -> uint32 [B, W], shard i at bit i % 32 of word i // 32."""
    B, n = bits.shape
    full = np.zeros((B, 32 * W), dtype=np.uint8)
    full[:, :n] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view("<u4").reshape(B, W)


def words_to_bits(words, n):
    B = words.shape[0]
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(B, -1), axis=1,
                         bitorder="little")[:, :n].astype(bool)


_MUL = []


def gf_mul_table(oracle):
    if not _MUL:
        _MUL.append(np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8))
    return _MUL[0]


def gen_present(rng, s, mode):
    """Present bits [B, n]. data: 0..min(k, m) data shards lost; single: 0 or 1 data shard; any: up to m
    shards of either kind; few: as any, with every ninth block short of k shards (a data shard among
    the lost)."""
    k, m, n = s.k, s.m, s.k + s.m
    present = np.ones((s.B, n), dtype=bool)
    for b in range(s.B):
        if mode == "few" and b % 9 == 4:
            lost = [0] + [1 + int(i) for i in rng.choice(n - 1, size=m, replace=False)]
        elif mode == "single":
            lost = rng.choice(k, size=int(rng.integers(0, 2)), replace=False)
        elif mode == "data":
            lost = rng.choice(k, size=int(rng.integers(0, min(k, m) + 1)), replace=False)
        else:
            lost = rng.choice(n, size=int(rng.integers(0, m + 1)), replace=False)
        present[b, np.asarray(lost, dtype=int)] = False
    return present


class Batch:
    """One live batch on the CPU: its images and the exact model of every step."""

    def __init__(self, spec, oracle, seed):
        self.s, self.o = spec, oracle
        k, m, B = spec.k, spec.m, spec.B
        self.n = n = k + m
        self.W, self.Wk = (n + 31) // 32, (k + 31) // 32
        rng = np.random.default_rng([seed, ord(spec.id)])
        self.data, self.par = place(spec.layout, k, m, spec.L, B)
        self.ss = self.data.ss
        ss = self.w_ = rup16(spec.L) + 16    # the bytes of a slot the model looks at (in every layout slots are
        assert ss <= self.ss                 # at least this far apart; a shard-major stride spans other slots)
        if spec.kind == "ragged":
            self.lens = np.array([PATTERN[b % len(PATTERN)] for b in range(B)], dtype=np.uint32)
        else:
            self.lens = np.full(B, spec.L, dtype=np.uint32)
        assert self.lens.max() == spec.L
        x = np.arange(ss)[None, None, :]
        ln = self.lens.astype(np.int64)[:, None, None]
        self.body = x < ln                                 # [B, 1, ss]: bytes below the block's length
        self.pad = (x >= ln) & (x < rup16(ln))             # zero fill of an output slot
        self.img = canary_image([self.data, self.par])
        dv = self.dview(self.img)
        dv[...] = np.where(self.body, rng.integers(0, 256, (B, k, ss), dtype=np.uint8), CANARY)
        self.pview(self.img)[...] = np.where(self.body, self.encode_of(dv), CANARY)
        # the recover calls' out slots lie one shard stride apart, as the batch's own
        self.outreg = (Region(GUARD, self.data.bs, self.ss, m, B) if spec.layout.startswith("shard_major") else
                       Region(GUARD, m * self.ss + 32, self.ss, m, B))
        self.out = canary_image([self.outreg])
        self.new = canary_image([self.data, self.par])
        self.dview(self.new)[...] = np.where(self.body, rng.integers(0, 256, (B, k, ss), dtype=np.uint8), CANARY)
        # lengths with two blocks past the maximum, for the ragged encode's oversize statuses
        self.lens2 = self.lens.copy()
        self.lens2[[5, B - 3]] = [spec.L + 1, 4000]
        self.seg, off = {}, WGUARD
        for name, cnt in [("mask", B * self.W), ("status", B), ("verdict", B), ("counts", 2), ("present", B * self.W),
                          ("col", B * self.Wk), ("lens", B), ("lens2", B), ("want", B)]:
            self.seg[name] = (off, cnt)
            off += cnt + WGUARD
        self.words = np.full(off, CANARY32, dtype=np.uint32)
        self.present = np.ones((B, n), dtype=bool)
        self.w("mask")[:] = bits_to_words(self.present, self.W).ravel()
        for name in ("status", "verdict", "counts", "present"):
            self.w(name)[:] = STALE
        self.w("col")[:] = 0
        self.w("lens")[:] = self.lens
        self.w("lens2")[:] = self.lens2
        self.w("want")[:] = 0xFFFFFFFF
        self.hit = [frozenset()] * B

    def dview(self, img):
        return self.data.view(img, 0, self.w_)

    def pview(self, img):
        return self.par.view(img, 0, self.w_)

    def w(self, name):
        off, cnt = self.seg[name]
        return self.words[off:off + cnt]

    def images(self):
        return dict(img=self.img.copy(), out=self.out.copy(), new=self.new.copy(), words=self.words.copy())

    # ---- the oracle over per-block lengths

    def groups(self, sel=None):
        for length in np.unique(self.lens):
            idx = np.flatnonzero((self.lens == length) if sel is None else (self.lens == length) & sel)
            if length and idx.size:
                yield int(length), idx

    def encode_of(self, d):
        """[B, m, ss]: the oracle's parity of data rows d [B, k, ss] over each block's length, zero past it."""
        k, m = self.s.k, self.s.m
        res = np.zeros((self.s.B, m, self.w_), dtype=np.uint8)
        for length, idx in self.groups():
            sub = np.zeros((idx.size, k + m, length), dtype=np.uint8)
            sub[:, :k] = d[idx][:, :, :length]
            if self.s.kind == "xor":
                self.o.xor_encode(k, sub)
            else:
                self.o.rs_encode(k, m, sub)
            res[idx, :, :length] = sub[:, k:]
        return res

    def rebuilt(self, present):
        """(rec, e_d, few): the arena's shards [B, n, ss] with every missing data shard of a block that has
        k present shards rebuilt over the block's length from its first k present shards: the oracle's
        ReconstructData, and for codes of more than 32 shards the inverse of the first-k-present submatrix
        of the oracle's matrix (as test_gpu_wide.py)."""
        k, m, n = self.s.k, self.s.m, self.n
        sh = np.concatenate([self.dview(self.img), self.pview(self.img)], axis=1)
        lost = ~present
        e_d, few = lost[:, :k].sum(axis=1), present.sum(axis=1) < k
        rec = sh.copy()
        todo = (e_d > 0) & ~few
        if n <= 32:
            masks = bits_to_words(present, 1).ravel()
            for length, idx in self.groups(todo):
                sub = np.ascontiguousarray(sh[idx][:, :, :length])
                if self.s.kind == "xor":
                    st = self.o.xor_reconstruct(k, sub, masks[idx])
                else:
                    st = self.o.rs_reconstruct(k, m, sub, masks[idx])
                assert not st.any()
                rec[idx, :k, :length] = sub[:, :k]
        else:
            MUL, M, L = gf_mul_table(self.o), self.o.build_matrix(k, n), self.s.L
            for b in np.flatnonzero(todo):
                have = np.flatnonzero(present[b])[:k]
                inv = self.o.invert(M[have])
                src = sh[b, have, :L]
                for i in np.flatnonzero(lost[b, :k]):
                    rec[b, i, :L] = np.bitwise_xor.reduce(MUL[inv[i][:, None], src], axis=0)
        return rec, e_d, few

    def write(self, view, sel, vals):
        """Output slots sel [B, rows] of view [B, rows, ss] receive vals below the block's length and zeros
        up to the next multiple of 16."""
        view[self.body & sel[:, :, None]] = vals[self.body & sel[:, :, None]]
        view[self.pad & sel[:, :, None]] = 0

    def slot_bytes(self, sel):
        """Arena offsets of the bytes below the block's length of the shards sel [B, n]."""
        k = self.s.k
        return np.concatenate([self.data.index(0, self.w_)[self.body & sel[:, :k, None]],
                               self.par.index(0, self.w_)[self.body & sel[:, k:, None]]])

    def stale(self, *names):
        for name in names:
            self.w(name)[:] = STALE

    # ---- the steps: each returns (sticky code, the inputs its device form needs)

    def erase(self, a):
        self.present = gen_present(np.random.default_rng(a["seed"]), self.s, a["mode"])
        idx = self.slot_bytes(~self.present)
        self.img[idx] = ERASED
        mw = bits_to_words(self.present, self.W).ravel()
        self.w("mask")[:] = mw
        return OK, dict(idx=idx, mask=mw)

    def encode(self, a):
        dv, pv = self.dview(self.img), self.pview(self.img)
        sel = np.ones((self.s.B, self.s.m), dtype=bool)
        code = OK
        if self.s.kind == "ragged":
            over = (self.lens2 > self.s.L) & bool(a.get("oversize"))
            sel &= ~over[:, None]
            self.stale("status")
            self.w("status")[:] = np.where(over, SHARD_SIZE, 0).astype(np.int32).view(np.uint32)
            code = SHARD_SIZE if over.any() else OK
        self.write(pv, sel, self.encode_of(dv))
        return code, {}

    xor_encode = ragged_encode = encode

    def decode(self, a, present=None, slots=0, want=None, some=False):
        """The in-place and out-of-place reconstructs of every family, and reconstruct-some."""
        k, B = self.s.k, self.s.B
        present = self.present if present is None else present
        rec, e_d, few = self.rebuilt(present)
        lost = ~present
        self.stale("status")
        if some:
            R = lost & (np.ones_like(lost) if want is None else want)
            st = np.where(R.any(axis=1) & few, TOO_FEW, 0)
            good = R.any(axis=1) & ~few
            self.write(self.dview(self.img), R[:, :k] & good[:, None], rec[:, :k])
            self.write(self.pview(self.img), R[:, k:] & good[:, None], self.encode_of(rec[:, :k]))
        elif slots == 0:
            st = np.where((e_d > 0) & few, TOO_FEW, 0)
            self.write(self.dview(self.img), lost[:, :k] & ((e_d > 0) & ~few)[:, None], rec[:, :k])
        else:
            st = np.where(e_d == 0, 0, np.where(few, TOO_FEW, np.where(e_d > slots, INVALID, e_d)))
            vals = np.zeros((B, self.s.m, self.w_), dtype=np.uint8)
            sel = np.zeros((B, self.s.m), dtype=bool)
            for b in np.flatnonzero(st > 0):
                rows = np.flatnonzero(lost[b, :k])
                vals[b, :rows.size] = rec[b, rows]
                sel[b, :rows.size] = True
            self.write(self.outreg.view(self.out, 0, self.w_), sel, vals)
        self.w("status")[:] = st.astype(np.int32).view(np.uint32)
        return worst(set(st[st < 0].tolist())), {}

    def reconstruct(self, a):
        return self.decode(a)

    def recover(self, a):
        return self.decode(a, slots=a["slots"])

    ragged_reconstruct = xor_reconstruct = reconstruct_wide = reconstruct
    ragged_recover = recover_wide = recover

    def reconstruct_some(self, a):
        want = None
        inputs = {}
        if a.get("want_seed") is not None:
            want = np.random.default_rng(a["want_seed"]).random((self.s.B, self.n)) < 0.6
            inputs["want"] = bits_to_words(want, 1).ravel()
            self.w("want")[:] = inputs["want"]
        code, _ = self.decode(a, want=want, some=True)
        return code, inputs

    def heal(self, a):
        """The present masks the preceding locate wrote, as they lie in the words."""
        present = words_to_bits(self.w("present").reshape(self.s.B, self.W), self.n)
        if self.n <= 32:
            return self.decode(a, present=present, some=True)
        return self.decode(a, present=present)

    def verify(self, a):
        want = self.encode_of(self.dview(self.img))
        bad = ((want != self.pview(self.img)) & self.body).any(axis=(1, 2))
        self.stale("status", "counts")
        self.w("status")[:] = np.where(bad, 0, 1)
        self.w("counts")[0] = int(bad.sum())
        return OK, {}

    def columns(self, a):
        col = np.random.default_rng(a["seed"]).random((self.s.B, self.s.k)) < a.get("p", 0.3)
        col[::7] = False                                  # blocks with an empty mask: untouched
        cw = bits_to_words(col, self.Wk).ravel()
        self.w("col")[:] = cw
        return col, cw

    def fold(self, col, delta):
        pv = self.pview(self.img)
        fold = self.encode_of(np.where(col[:, :, None] & self.body, delta, 0))
        self.write(pv, np.repeat(col.any(axis=1)[:, None], self.s.m, axis=1), pv ^ fold)

    def update(self, a):
        """parity ^= encode(masked columns of old ^ new); then the caller copies the new columns over the
        old, and changes them in the new arena so that the next update has something to fold."""
        col, cw = self.columns(a)
        dv, nv = self.dview(self.img), self.dview(self.new)
        self.fold(col, dv ^ nv)
        idx = self.data.index(0, self.w_)[self.body & col[:, :, None]]
        self.img[idx] = self.new[idx]
        self.new[idx] ^= NEW_FLIP
        return OK, dict(col=cw, idx=idx)

    def encode_idx(self, a):
        col, cw = self.columns(a)
        self.fold(col, self.dview(self.img))
        return OK, dict(col=cw)

    def corrupt(self, a):
        """Bytes below L of t_b <= t shards of about half the blocks are flipped; the batch was consistent."""
        rng = np.random.default_rng(a["seed"])
        k, n, L = self.s.k, self.n, self.s.L
        idx, vals, self.hit = [], [], []
        for b in range(self.s.B):
            t = int(rng.integers(1, a["t"] + 1)) if rng.random() < 0.5 else 0
            hit = [int(s) for s in rng.choice(n, size=t, replace=False)]
            self.hit.append(frozenset(hit))
            for s in hit:
                base = self.data.at(b, s) if s < k else self.par.at(b, s - k)
                for x in rng.choice(L, size=min(L, int(rng.integers(1, 4))), replace=False):
                    idx.append(base + int(x))
                    vals.append(int(rng.integers(1, 256)))
        idx, vals = np.array(idx, dtype=np.int64), np.array(vals, dtype=np.uint8)
        self.img[idx] ^= vals
        return OK, dict(idx=idx, vals=vals)

    def located(self, verdicts):
        present = np.ones((self.s.B, self.n), dtype=bool)
        for b, h in enumerate(self.hit):
            present[b, sorted(h)] = False
        t = np.array([len(h) for h in self.hit])
        self.stale("verdict", "present", "counts")
        self.w("verdict")[:] = verdicts.astype(np.int32).view(np.uint32)
        self.w("present")[:] = bits_to_words(present, self.W).ravel()
        self.w("counts")[:] = [int((t > 0).sum()), 0]
        return OK, {}

    def locate(self, a):
        assert self.s.m >= 2 and all(len(h) <= 1 for h in self.hit)
        return self.located(np.array([min(h) if h else CLEAN for h in self.hit]))

    def locate_multi(self, a):
        assert all(len(h) <= min(a["max_bad"], self.s.m // 2) for h in self.hit)
        return self.located(np.array([len(h) for h in self.hit]))


# ------------------------------------------------------------------ the program generator

def euler_chains():
    """The 56 ordered pairs of distinct users as one closed walk (Hierholzer on the complete digraph),
    cut into 28 chains of three users: every pair lies in exactly one."""
    out = {u: [v for v in USERS if v != u] for u in USERS}
    stack, walk = [USERS[0]], []
    while stack:
        u = stack[-1]
        if out[u]:
            stack.append(out[u].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == 57
    return [tuple(walk[i:i + 3]) for i in range(0, 56, 2)]


CHAINS = euler_chains()


def program(seed):
    """12-16 steps over three live batches: a prologue that uses no workspace, a chain of three workspace
    users as consecutive library calls (the caller's own kernels alone between them), then what brings
    the batches back to a consistent state, interleaved with further episodes on the three batches,
    syncs, a host-path call, and in every fourth program a step with failing blocks."""
    rng = np.random.default_rng(0x5E9 + seed)
    chain = CHAINS[seed % len(CHAINS)]
    if seed >= len(CHAINS):       # two users, so that a batch outside the chain is live: the XOR one in every second
        u, v = (str(u) for u in rng.permutation(USERS)[:2])
        chain = (u, v, u)
    grow = seed % 2 == 0          # prefer a small first batch and a large later one

    def choose(u, cand, first):
        if grow:
            cand = [c for c in cand if c in (SMALL_PLANS if first else LARGE_PLANS)] or cand
            return cand[0]
        return cand[int(rng.integers(len(cand)))]

    # the chain's batches: locate-multi needs a consistent batch, so one that no other user of the chain
    # leaves erased; reconstruct-some takes a batch of its own too
    pick = {}
    for own in (False, True):
        for u in chain:
            if u not in pick and (u in ("lmulti", "some")) == own:
                cand = list(USER_BATCHES[u])
                if own:
                    cand = [c for c in cand if c not in pick.values()] or cand
                pick[u] = choose(u, cand, u == chain[0])
    live = list(dict.fromkeys(pick[u] for u in chain))
    spare = [str(b) for b in rng.permutation(sorted(POOL)) if b not in live]
    if seed % 2 == 0:
        spare.sort(key=lambda b: b != "G")
    live += spare[:3 - len(live)]
    state = {b: "clean" for b in live}
    steps = []
    ns = [0]

    def S(kind, b=None, **args):
        ns[0] += 1
        if kind in ("erase", "corrupt", "update", "encode_idx"):
            args.setdefault("seed", 1000 * seed + ns[0])
        steps.append(Step(kind, b, args))

    def fam(b, kind):
        f = POOL[b].kind
        if b == "F":
            return {"reconstruct": "reconstruct_wide", "recover": "recover_wide"}.get(kind, kind)
        if f == "xor":
            return "xor_" + kind
        return "ragged_" + kind if f == "ragged" else kind

    # prologue: two steps that use no workspace and leave their batches consistent
    folded = {}
    for b in (str(b) for b in rng.permutation(live)[:2]):
        f = POOL[b].kind
        c = int(rng.integers(4))
        if f == "xor":
            S("xor_encode", b)
        elif f == "ragged":
            S("ragged_encode", b, oversize=c == 0)
        elif c == 3:
            S("encode_idx", b)
            folded[b] = steps[-1]
        else:
            S(("encode", "verify", "update")[c], b)
    for b, st in folded.items():        # the second fold of the same columns gives the parity back
        S("verify", b)
        steps.append(st)
    # the chain
    for u in chain:
        b = pick[u]
        s = POOL[b]
        if u == "lmulti":
            assert state[b] in ("clean", "corrupt"), (seed, chain, pick, state)
            if state[b] == "clean":
                S("corrupt", b, t=min(s.m // 2, 3))
            S("locate_multi", b, max_bad=8)
            state[b] = "corrupt"
            continue
        assert state[b] in ("clean", "erased"), (seed, chain, pick, state)
        if state[b] == "clean":
            S("erase", b, mode="single" if u == "routed" and rng.random() < 0.3 else "data")
            state[b] = "erased"
        if u == "some":
            S("reconstruct_some", b, want_seed=int(rng.integers(1 << 30)) if rng.random() < 0.4 else None)
            if steps[-1].args["want_seed"] is None:
                state[b] = "clean"
        elif u == "sorted2" or (u != "routed" and rng.random() < 0.4):
            S(fam(b, "recover"), b, slots=s.m)
        else:
            S(fam(b, "reconstruct"), b)
            state[b] = "clean"                      # only data shards were lost
    # back to a consistent state, then more episodes, interleaved
    queues = {b: [] for b in live}

    def Q(b, kind, **args):
        queues[b].append((kind, args))

    for b in live:
        if state[b] == "corrupt":
            Q(b, "heal")
        elif state[b] == "erased":
            Q(b, "reconstruct_some" if POOL[b].kind == "rs" and b != "F" else fam(b, "reconstruct"))
        state[b] = "clean"
    fail = seed % 4 == 1
    for r in range(3):
        for b in (str(b) for b in rng.permutation(live)):
            s = POOL[b]
            if state[b] == "failed":
                continue
            c = int(rng.integers(6))
            if fail and r == 0 and b == live[seed // 4 % 3]:
                Q(b, "erase", mode="few")
                Q(b, fam(b, "reconstruct") if rng.random() < 0.6 or s.kind != "rs" or b == "F" else "reconstruct_some")
                if seed % 8 == 1:
                    Q(b, "sync")
                state[b] = "failed"
            elif s.kind == "xor":
                if c < 3:
                    Q(b, "erase", mode="single"), Q(b, "xor_reconstruct")
                else:
                    Q(b, "xor_encode")
            elif s.kind == "ragged":
                if c < 2:
                    Q(b, "erase", mode="data"), Q(b, "ragged_reconstruct")
                elif c < 4:
                    Q(b, "erase", mode="data"), Q(b, "ragged_recover", slots=1 if c == 2 else s.m)
                    Q(b, "ragged_reconstruct")
                else:
                    Q(b, "ragged_encode", oversize=c == 4)
            elif c == 0 and s.m >= 2:
                Q(b, "corrupt", t=1), Q(b, "locate"), Q(b, "heal")
                if b == "F":
                    Q(b, "encode")
            elif c == 1 and s.m <= 16:
                Q(b, "corrupt", t=min(s.m // 2, 3)), Q(b, "locate_multi", max_bad=8), Q(b, "heal")
            elif c == 2:
                Q(b, "erase", mode="any"), Q(b, fam(b, "reconstruct")), Q(b, "encode")
            elif c == 3:
                Q(b, "erase", mode="data"), Q(b, fam(b, "recover"), slots=1 if rng.random() < 0.5 else s.m)
                Q(b, fam(b, "reconstruct"))
            elif c == 4:
                Q(b, "update")
            else:
                Q(b, "encode_idx"), Q(b, "verify"), Q(b, "encode")
    extra = (["host_call"] if seed % 3 == 0 else []) + (["sync"] if seed % 5 == 0 else [])
    # interleave: a batch's own steps keep their order; past 12 steps, stop where no batch is in the
    # middle of an episode (every episode ends in a library call that leaves its batch consistent)
    starts = ("erase", "corrupt", "encode_idx", "update", "xor_encode", "ragged_encode")
    open_ = {b: bool(queues[b]) and queues[b][0][0] not in starts for b in live}
    while any(queues.values()) and len(steps) < 16:
        if extra and rng.random() < 0.3:
            S(extra.pop())
            continue
        b = str(rng.choice([q for q in live if queues[q]]))
        kind, args = queues[b].pop(0)
        S(kind, None if kind == "sync" else b, **args)
        open_[b] = bool(queues[b]) and queues[b][0][0] not in starts
        if len(steps) >= 12 and not any(open_.values()):
            break
    ends_clean = [b for b in live if state[b] != "failed" and not open_[b]]
    return live, steps, ends_clean


def expected_codes(steps, codes):
    """Per sync step (and the final sync, the last entry): the code fec_sync reports there."""
    out, pending = [], set()
    for st, c in zip(steps, codes):
        if st.kind == "sync":
            out.append(worst(pending))
            pending = set()
        else:
            pending.add(c)
    out.append(worst(pending))
    return out


class Trace:
    """A program run on the model alone."""

    def __init__(self, oracle, seed, live=None, steps=None, keep=False):
        """keep: the images after every step, for the synced form (else the words alone)."""
        self.seed = seed
        self.live, self.steps, self.ends_clean = program(seed) if steps is None else (live, steps, [])
        self.batches = {b: Batch(POOL[b], oracle, seed) for b in self.live}
        self.initial = {b: x.images() for b, x in self.batches.items()}
        self.codes, self.inputs, self.after = [], [], []
        for st in self.steps:
            if st.batch is None:
                code, inp = OK, {}
                self.after.append(None)
            else:
                code, inp = getattr(self.batches[st.batch], st.kind)(st.args)
                x = self.batches[st.batch]
                self.after.append(x.images() if keep else dict(words=x.words.copy()))
            self.codes.append(code)
            self.inputs.append(inp)
        self.sync_codes = expected_codes(self.steps, self.codes)
        self.final = {b: x.images() for b, x in self.batches.items()}

    def describe(self, i):
        st = self.steps[i]
        return "step %d: %s on %s %s" % (i, st.kind, st.batch, st.args)


# ------------------------------------------------------------------ the device form

class Device:
    """A traced program on a ctx. Everything is uploaded first (arenas, words and each step's inputs);
    then step(i) queues step i on the ctx stream with no host wait. A status array is refilled with
    STALE before the call that writes it and the words are cloned after it, both on the stream."""

    def __init__(self, fec, torch, codec, trace, oracle, stream=None):
        self.fec, self.torch, self.c, self.t, self.o, self.stream = fec, torch, codec, trace, oracle, stream
        self.dev, self.clones, self.sync_rcs = {}, [], []
        with self.on():
            for b, im in trace.initial.items():
                self.dev[b] = {name: torch.from_numpy(a.view(np.int32) if name == "words" else a.copy()).cuda()
                               for name, a in im.items()}
                assert all(t.data_ptr() % 16 == 0 for t in self.dev[b].values())
            self.inp = [{name: torch.from_numpy(a.astype(np.int64) if name == "idx" else
                                                a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
                         for name, a in inp.items()} for inp in trace.inputs]

    def on(self):
        return self.torch.cuda.stream(self.stream) if self.stream is not None else _Null()

    def seg(self, b, name):
        off, cnt = self.t.batches[b].seg[name]
        return self.dev[b]["words"][off:off + cnt]

    def step(self, i):
        with self.on():
            self._step(i)

    def _step(self, i):
        st, inp = self.t.steps[i], self.inp[i]
        fec, lib, h, D = self.fec, self.fec.lib, self.c.handle, self.fec.FEC_DEVICE
        if st.kind == "sync":
            self.sync_rcs.append((self.c.lib_sync_rc(), self.c.lib_sync_rc()))
            return
        if st.kind == "host_call":
            self.host_call()
            return
        b, kind, a = st.batch, st.kind, st.args
        m_ = self.t.batches[b]
        s, d = m_.s, self.dev[b]
        k, m, L, B = s.k, s.m, s.L, s.B
        p = d["img"].data_ptr()
        region = (k, m, L, B, p + m_.data.off, m_.data.bs, p + m_.par.off, m_.par.bs, m_.ss)

        def ptr(name):
            return self.seg(b, name).data_ptr()

        def stale(*names):
            for name in names:
                self.seg(b, name).fill_(STALE)

        out = (d["out"].data_ptr() + m_.outreg.off, m_.outreg.bs)
        rc = fec.FEC_OK
        if kind == "erase":
            d["img"][inp["idx"]] = ERASED
            self.seg(b, "mask").copy_(inp["mask"])
            return
        if kind == "corrupt":
            d["img"][inp["idx"]] = d["img"][inp["idx"]] ^ inp["vals"]
            return
        if kind == "encode":
            rc = lib.fec_rs_encode_batch(h, *region, D)
        elif kind == "xor_encode":
            rc = lib.fec_xor_encode_batch(h, k, *region[2:], D)
        elif kind == "ragged_encode":
            stale("status")
            rc = lib.fec_rs_encode_ragged_batch(h, *region, ptr("lens2" if a.get("oversize") else "lens"),
                                                ptr("status"), D)
        elif kind == "reconstruct":
            stale("status")
            rc = lib.fec_rs_reconstruct_batch(h, *region, ptr("mask"), ptr("status"), D)
        elif kind == "recover":
            stale("status")
            rc = lib.fec_rs_recover_batch(h, *region, ptr("mask"), *out, a["slots"], ptr("status"), D)
        elif kind == "reconstruct_wide":
            stale("status")
            rc = lib.fec_rs_reconstruct_wide_batch(h, *region, ptr("mask"), m_.W, ptr("status"), D)
        elif kind == "recover_wide":
            stale("status")
            rc = lib.fec_rs_recover_wide_batch(h, *region, ptr("mask"), m_.W, *out, a["slots"], ptr("status"), D)
        elif kind == "ragged_reconstruct":
            stale("status")
            rc = lib.fec_rs_reconstruct_ragged_batch(h, *region, ptr("mask"), ptr("lens"), ptr("status"), D)
        elif kind == "ragged_recover":
            stale("status")
            rc = lib.fec_rs_recover_ragged_batch(h, *region, ptr("mask"), ptr("lens"), *out, a["slots"],
                                                 ptr("status"), D)
        elif kind == "xor_reconstruct":
            stale("status")
            rc = lib.fec_xor_reconstruct_batch(h, k, *region[2:], ptr("mask"), ptr("status"), D)
        elif kind == "reconstruct_some":
            stale("status")
            if "want" in inp:
                self.seg(b, "want").copy_(inp["want"])
            rc = lib.fec_rs_reconstruct_some_batch(h, *region, ptr("mask"), ptr("want") if "want" in inp else None,
                                                   ptr("status"), D)
        elif kind == "heal":                   # the masks are where the locate call wrote them
            stale("status")
            if m_.n <= 32:
                rc = lib.fec_rs_reconstruct_some_batch(h, *region, ptr("present"), None, ptr("status"), D)
            else:
                rc = lib.fec_rs_reconstruct_wide_batch(h, *region, ptr("present"), m_.W, ptr("status"), D)
        elif kind == "verify":
            stale("status", "counts")
            rc = lib.fec_rs_verify_batch(h, *region, ptr("status"), ptr("counts"), D)
        elif kind == "update":
            self.seg(b, "col").copy_(inp["col"])
            q = d["new"].data_ptr()
            rc = lib.fec_rs_update_batch(h, k, m, L, B, p + m_.data.off, m_.data.bs, q + m_.data.off, m_.data.bs,
                                         p + m_.par.off, m_.par.bs, m_.ss, ptr("col"), m_.Wk, D)
            d["img"][inp["idx"]] = d["new"][inp["idx"]]
            d["new"][inp["idx"]] = d["new"][inp["idx"]] ^ NEW_FLIP
        elif kind == "encode_idx":
            self.seg(b, "col").copy_(inp["col"])
            rc = lib.fec_rs_encode_idx_batch(h, *region, ptr("col"), m_.Wk, D)
        elif kind == "locate":
            stale("verdict", "present", "counts")
            rc = lib.fec_rs_locate_batch(h, *region, ptr("verdict"), ptr("present"), m_.W, ptr("counts"), D)
        elif kind == "locate_multi":
            stale("verdict", "present", "counts")
            rc = lib.fec_rs_locate_multi_batch(h, *region, a["max_bad"], ptr("verdict"), ptr("present"), m_.W,
                                               ptr("counts"), D)
        else:
            raise ValueError(kind)
        assert rc == fec.FEC_OK, (self.t.describe(i), rc)
        self.clones.append((i, d["words"].clone()))

    def host_call(self):
        """One FEC_HOST RS(8,4) encode and reconstruct of 9 blocks on the same ctx: correct bytes, and the
        device path's sticky word is not its business."""
        rng = np.random.default_rng(9)
        sh = np.zeros((9, 12, 48), dtype=np.uint8)
        sh[:, :8] = rng.integers(0, 256, (9, 8, 48), dtype=np.uint8)
        want = self.o.rs_encode(8, 4, sh.copy())
        self.c.rs_encode(8, 4, sh)
        assert np.array_equal(sh, want), "host-path encode in the middle of the queue"
        masks = np.full(9, 0xFFF & ~0b100100000101, dtype=np.uint32)
        dmg = want.copy()
        dmg[:, [0, 2, 8, 11]] = 0x77
        st = np.full(9, 7, dtype=np.int32)
        assert self.c.rs_reconstruct(8, 4, dmg, masks, status=st) == self.fec.FEC_OK and not st.any()
        assert np.array_equal(dmg[:, :8], want[:, :8]), "host-path reconstruct in the middle of the queue"

    # ---- comparisons (they copy to the host: only after the program, or in the synced form)

    def compare_batch(self, b, want, what):
        for name in ("img", "out", "new"):
            check_arena(self.dev[b][name].cpu().numpy(), want[name], "%s: batch %s, %s arena" % (what, b, name))
        compare_words(self.t.batches[b], self.dev[b]["words"].cpu().numpy().view(np.uint32), want["words"],
                      "%s: batch %s" % (what, b))

    def compare_final(self, what):
        for b in self.t.live:
            self.compare_batch(b, self.t.final[b], what)
        for i, w in self.clones:
            compare_words(self.t.batches[self.t.steps[i].batch], w.cpu().numpy().view(np.uint32),
                          self.t.after[i]["words"], "%s: words cloned after %s" % (what, self.t.describe(i)))
        syncs = self.sync_rcs
        assert [r[0] for r in syncs] == self.t.sync_codes[:len(syncs)], \
            "%s: fec_sync gave %s, want %s" % (what, syncs, self.t.sync_codes)
        assert all(r[1] == OK for r in syncs), "%s: the sticky word is reported once: %s" % (what, syncs)


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def compare_words(batch, got, want, what):
    if np.array_equal(got, want):
        return
    i = int(np.flatnonzero(got != want)[0])
    name = next((n for n, (off, cnt) in batch.seg.items() if off <= i < off + cnt), "a guard word")
    off = batch.seg[name][0] if name in batch.seg else 0
    raise AssertionError("%s: %d words differ from the model, first in %s at %d (got 0x%08x, want 0x%08x)"
                         % (what, int((got != want).sum()), name, i - off, got[i], want[i]))


def run_queued(fec, torch, codec, trace, oracle, stream=None):
    """The whole program with no host wait but its own sync steps, one final fec_sync, then every compare."""
    dev = Device(fec, torch, codec, trace, oracle, stream)
    for i in range(len(trace.steps)):
        dev.step(i)
    finish(dev, "queued")
    return dev


def finish(dev, what):
    dev.sync_rcs.append((dev.c.lib_sync_rc(), dev.c.lib_sync_rc()))
    dev.compare_final("%s program %d" % (what, dev.t.seed))


def first_synced_difference(fec, torch, trace, oracle):
    """The program again on a new ctx with a sync and a full compare after every step: the first step that
    differs from the model, or that the program differs only when queued."""
    trace = Trace(oracle, trace.seed, trace.live, trace.steps, keep=True)
    c = fec.Codec(0).use_torch_stream()
    try:
        dev = Device(fec, torch, c, trace, oracle)
        for i, st in enumerate(trace.steps):
            dev.step(i)
            if st.kind == "sync":
                continue
            rc = c.lib_sync_rc()
            if st.batch is None:
                continue
            try:
                assert rc == trace.codes[i], "fec_sync gave %d, want %d" % (rc, trace.codes[i])
                dev.compare_batch(st.batch, trace.after[i], "synced")
            except AssertionError as e:
                return "first differing step when synced: %s (%s)" % (trace.describe(i), e)
        return "differs only when queued"
    finally:
        c.close()
