"""Adversarial batches for fec_rs_locate_multi_batch and fec_rs_locate_partial_batch in codes of any
size, each block's expected result derived by construction and, independently, by the Berlekamp-Welch
model of locate_model.py. Built from the oracle's parity (arena.oracle_arena) without a device:
test_locate_hard_cases.py checks the batches on the CPU, test_gpu_locate_hard.py runs them.

A block has the present shards P (all n for locate-multi), m' = |P| - k checks and the radius
T = min(max_bad, m' / 2). With u_r = 1 / prod_{j in P, j != r} (r ^ j), a byte column with the errors
e_r has the sums W_l = sum_r u_r e_r r^l, l < m' (0^0 = 1), all zero exactly for a codeword. Every
construction works on one byte column of one block; a block's classes:

  a    beyond the radius, random: t shards, T < t <= min(|P|, m' + 2). Expected: the model's (almost
       always unknown; a block that ends located is a miscorrection found by chance).
  b    miscorrection to a disjoint set: S of m' + 1 present shards; c_r = g prod_{j in P \\ S} (r ^ j) is a
       codeword with support S; the shards A of S, |A| = m' + 1 - T', are changed by c_r (T' = T or 1).
       Expected: (T', S \\ A), none of the changed shards; healing gives the codeword clean ^ c.
  c    pseudo-root outside the code (n < 256): the sums of v - 1 errors at present points and one at a
       point z >= n, realised as real errors on the last m' present shards (the parity shards when all
       are present) by solving [u_r r^l] e = W. Expected: unknown: an explanation of weight <= T within
       the code would, with the v <= T terms of W, be a vanishing combination of at most 2 T <= m'
       distinct columns [r^l], whose weight at z is not zero.
  d    the same with z a missing shard of the block (locate-partial).
  e    zero pivots: two errors with W_0 = 0 (e_b = e_a u_a / u_b), or three with W_0 W_2 = W_1^2, a zero
       2 x 2 leading minor. Expected: located exactly.
  f    merges over 16-byte chunks (for L = 1202 more than 64 chunks apart, so in different waves):
       f1/f2 every column within the radius, the union T + 1 / 2 T shards: unknown; f3 a located
       column and a class c (d, a where there is none) column: unknown; f4 the same set from a column
       of T errors and a column of one: that set.
  loc  T errors in one column: located at v = T.       clean  nothing.

A batch: 67 blocks (23 for (240,16)), block b of class CYCLE[b % 7], the last one clean; a class that a
block cannot have is replaced (c in 256 shards and d without missing shards by a; e at a radius below
2 by loc). Locate-partial: block b has 1, 2 or m - 2 missing shards by b % 3 (one of m - 1, m - 2 is
odd), shard 0 and a parity shard first, every byte of their slots garbage; a class e block keeps a
radius of 2 by having one missing shard, and in 256 shards class a keeps to 1 and 2 missing shards
(see there). At most two corrupt byte columns per block. The bytes depend on (call, code, L, max_bad)
alone, not on the layout, so the model's work is done once per batch.

Every piece takes an optional vector v of per-shard multipliers (cauchy_oracle.multipliers) for a code
whose shard r is v_r p(r), the Cauchy code: the model decodes y_r / v_r, the weights are u_r / v_r (so
the zero pivots and the pseudo-roots are those of that code; the bytes of a batch built for u_r are
ordinary errors to it), class b's codeword is v_r g prod (r ^ j), a located class a block heals to
v_r f(r), and the clean codewords come from the encoder given as `oracle` (cauchy_oracle). Without v
nothing changes: the same draws, bytes and expectations as before. The Cauchy batches: CAUCHY_CODES x
CAUCHY_LENS (params(cauchy=True)).
"""
import numpy as np

from arena import CANARY, oracle_arena, place, shards  # noqa: F401
from locate_model import UNKNOWN, model_block, plan, poly_eval, reduce_rows, unscale, xdot

CODES = [(8, 4), (20, 10), (20, 9), (4, 16), (40, 16), (240, 16)]
LENS = [17, 33, 1202]
# under the Cauchy code: k a power of two and not, m odd, more than 32 shards, 256 shards
CAUCHY_CODES = [(8, 4), (20, 9), (40, 16), (240, 16)]
CAUCHY_LENS = [33, 1202]
CYCLE = ["a", "b", "c", "d", "e", "f", "loc"]
MODEL = "model"      # a column whose expectation is the model's

_CACHE = {}
_U = {}


def nblocks(k, m):
    return 67 if k + m <= 64 else 23


def max_bads(k, m):
    return [8, 2] if (k, m) in ((20, 10), (240, 16)) else [8]


class Col:
    """One byte column: errs {shard: xor value}, want: the set it must decode to, None (no explanation
    of weight <= T) or MODEL; cw: for class b the codeword's bytes at all n points."""

    def __init__(self, errs, want, cw=None):
        assert all(errs.values())
        self.errs, self.want, self.cw = errs, want, cw


class Builder:
    """The constructions for one set of present shards."""

    def __init__(self, gf, k, n, P, T, rng, v=None):
        self.mul, self.inv = gf[0].astype(np.int64), gf[1].astype(np.int64)
        self.gf, self.k, self.n, self.P, self.T, self.rng = gf, k, n, sorted(P), T, rng
        self.ms = len(self.P) - k
        self.miss = sorted(set(range(n)) - set(P))
        key = tuple(self.P)
        if key not in _U:
            _U[key] = {r: int(self.inv[self.prod(r ^ j for j in self.P if j != r)]) for r in self.P}
        self.u = _U[key]
        self.v = None if v is None else [int(x) for x in v]
        if v is not None:       # shard r = v_r p(r): an error e_r there is e_r / v_r in p's values
            self.u = {r: int(self.mul[u, self.inv[self.v[r]]]) for r, u in self.u.items()}

    def prod(self, xs):
        p = 1
        for x in xs:
            p = int(self.mul[p, x])
        return p

    def pw(self, r, l):
        return self.prod([r] * l)

    def nz(self):
        return int(self.rng.integers(1, 256))

    def pick(self, t, among=None):
        among = self.P if among is None else among
        return [int(s) for s in self.rng.permutation(among)[:t]]

    def sums(self, errs, count=None):
        """W_l of a column's errors {point: value} (weights u_r e_r), l < m'."""
        return [self.fold((int(self.mul[self.u[r], e]), r) for r, e in errs.items())(l)
                for l in range(self.ms if count is None else count)]

    def fold(self, terms):
        terms = list(terms)

        def W(l):
            w = 0
            for a, r in terms:
                w ^= int(self.mul[a, self.pw(r, l)])
            return w
        return W

    def random(self, S):
        return {s: self.nz() for s in S}

    def within(self, t):
        S = self.pick(t)
        return Col(self.random(S), frozenset(S))

    def beyond(self, t):
        assert self.T < t <= len(self.P)
        return Col(self.random(self.pick(t)), MODEL)

    def miscorrect(self, Tp):
        assert 1 <= Tp <= self.T
        S = self.pick(self.ms + 1)
        A, g = S[Tp:], self.nz()
        rest = [j for j in self.P if j not in S]
        cw = [int(self.mul[g, self.prod(r ^ j for j in rest)]) for r in range(self.n)]
        if self.v is not None:
            cw = [int(self.mul[self.v[r], c]) for r, c in enumerate(cw)]
        assert all((cw[r] != 0) == (r in S) for r in self.P)
        return Col({r: cw[r] for r in A}, frozenset(S[:Tp]), cw)

    def pseudo(self, v, z):
        """The sums of v - 1 errors in P and one at z (outside the code, or a missing shard), as errors on
        the last m' present shards."""
        if z is None:
            raise ValueError("a code of 256 shards has no point outside it")
        assert z not in self.P and 0 <= z < 256 and 1 <= v <= self.T
        W = self.fold([(self.nz(), r) for r in self.pick(v - 1) + [z]])
        R = self.P[-self.ms:]
        G = np.array([[int(self.mul[self.u[r], self.pw(r, l)]) for r in R] + [W(l)] for l in range(self.ms)],
                     dtype=np.uint8)
        assert reduce_rows(self.gf, G, self.ms) == list(range(self.ms))
        errs = {r: int(G[i, -1]) for i, r in enumerate(R) if G[i, -1]}
        assert self.sums(errs) == [W(l) for l in range(self.ms)]
        return Col(errs, None)

    def outside(self):
        return int(self.rng.integers(self.n, 256)) if self.n < 256 else None

    def zero_w0(self):
        a, b = self.pick(2)
        ea = self.nz()
        errs = {a: ea, b: int(self.mul[self.mul[ea, self.u[a]], self.inv[self.u[b]]])}
        assert self.sums(errs, 1) == [0]
        return Col(errs, frozenset((a, b)))

    def zero_minor(self):
        mul, inv = self.mul, self.inv
        while True:
            r = self.pick(3)
            a1, a2 = self.nz(), self.nz()
            sq = [int(mul[x, x]) for x in (r[0] ^ r[1], r[0] ^ r[2], r[1] ^ r[2])]
            den = int(mul[a1, sq[1]]) ^ int(mul[a2, sq[2]])
            if den:
                break
        a3 = int(mul[mul[mul[a1, a2], sq[0]], inv[den]])
        errs = {p: int(mul[a, inv[self.u[p]]]) for p, a in zip(r, (a1, a2, a3))}
        W = self.sums(errs, 3)
        assert W[0] and int(mul[W[0], W[2]]) == int(mul[W[1], W[1]])
        return Col(errs, frozenset(r))


class Cases:
    """A batch of hard blocks for one (call, code, L, max_bad); the same bytes in every layout."""

    def __init__(self, oracle, gf, call, k, m, L, max_bad, mult=None):
        assert call in ("multi", "partial")
        self.oracle, self.gf, self.call, self.mult = oracle, gf, call, mult
        self.k, self.m, self.n, self.L, self.max_bad = k, m, k + m, L, max_bad
        self.B = B = nblocks(k, m)
        n = k + m
        self.seed = 100000 * k + 1000 * m + 10 * L + max_bad + (5 if call == "partial" else 0)
        rng = np.random.default_rng(self.seed)
        img, data, par = oracle_arena(oracle, "interleaved", k, m, L, B, np.random.default_rng(self.seed))
        self.clean = shards(img, data, par)[:, :, :L]
        self.bad = self.clean.copy()
        self.final = self.clean.copy()          # what a located block heals to
        off = LENS.index(L) if L in LENS else 0
        es = [1, 2, m - 2]
        self.miss, self.T, self.kind, self.cols, self.t = [], [], [], [], []
        self.v = []                              # classes c and d: the size of the pseudo-support
        used = {}
        cps = (L + 15) // 16
        for b in range(B):
            kind = "clean" if b == B - 1 else CYCLE[b % len(CYCLE)]
            e = es[b % 3] if call == "partial" else 0
            if kind == "c" and n == 256:
                kind = "a"
            if kind == "e" and e and (m - e) // 2 < 2:    # the zero pivots need a radius of 2: one missing shard
                e = 1
            if kind == "a" and n == 256 and e == m - 2:
                # two sums and 242 of the 256 points in the code: W_1 / W_0 is a present shard 19 times in
                # 20, so nearly every such block would be a miscorrection; class a keeps to e = 1 and 2
                e = 1 + (b // 7) % 2
            miss = self.erasures(e) if e else set()
            P = sorted(set(range(n)) - miss)
            T = min(max_bad, (len(P) - k) // 2)
            bd = Builder(gf, k, n, P, T, rng, mult)
            if kind == "d" and not miss:
                kind = "a"
            if kind == "e" and T < 2:
                kind = "loc"
            i = used[kind] = used.get(kind, -1) + 1
            ca = int(rng.integers(min(cps, 6)))
            cb = cps - 1 - int(rng.integers(min(cps - 1, 6))) if cps > 1 else 0
            if cb == ca:
                cb = (ca + 1) % cps
            xa, xb = (16 * c + int(rng.integers(min(16, L - 16 * c))) for c in (ca, cb))
            assert cps == 1 or xa // 16 != xb // 16
            if L == 1202:
                assert abs(xa // 16 - xb // 16) > 64
            cols, v = {}, 0
            if kind == "a":     # t by a counter per number of missing shards, so that the lengths cover every t
                lo, hi = T + 1, min(len(P), len(P) - k + 2)
                j = used[("a", e)] = used.get(("a", e), -1) + 1
                cols[xa] = bd.beyond(lo + (3 * j + off) % (hi - lo + 1))
            elif kind == "b":
                cols[xa] = bd.miscorrect(T if i % 2 == 0 else 1)
            elif kind == "c":
                v = 1 + (i + off) % T
                cols[xa] = bd.pseudo(v, bd.outside())
            elif kind == "d":
                v = 1 + (i + off) % T
                cols[xa] = bd.pseudo(v, bd.miss[i % len(bd.miss)])
            elif kind == "e":
                cols[xa] = bd.zero_minor() if T >= 3 and i % 2 else bd.zero_w0()
            elif kind == "loc":
                cols[xa] = bd.within(T)
            elif kind == "f":
                f = "f%d" % (1 + (i + off) % 4)
                kind = f
                if f == "f1":
                    S = bd.pick(T + 1)
                    cols[xa], cols[xb] = Col(bd.random(S[:T]), frozenset(S[:T])), Col(bd.random(S[1:]), frozenset(S[1:]))
                elif f == "f2":
                    S = bd.pick(2 * T)
                    cols[xa], cols[xb] = Col(bd.random(S[:T]), frozenset(S[:T])), Col(bd.random(S[T:]), frozenset(S[T:]))
                elif f == "f3":
                    cols[xa] = bd.within(1 + i % T)
                    if n < 256:
                        cols[xb] = bd.pseudo(1 + i % T, bd.outside())
                    elif miss:
                        cols[xb] = bd.pseudo(1 + i % T, bd.miss[0])
                    else:
                        cols[xb] = bd.beyond(T + 1)
                else:
                    S = bd.pick(T)
                    cols[xa], cols[xb] = Col(bd.random(S), frozenset(S)), Col(bd.random(S[:1]), frozenset(S[:1]))
            for x, col in cols.items():
                for s, err in col.errs.items():
                    self.bad[b, s, x] ^= err
                if col.cw is not None:
                    self.final[b, :, x] ^= np.array(col.cw, dtype=np.uint8)
            self.miss.append(miss), self.T.append(T), self.kind.append(kind), self.cols.append(cols)
            self.v.append(v)
            self.t.append(len(set().union(*[c.errs.keys() for c in cols.values()])) if cols else 0)
        for b in range(B):                      # garbage in the missing slots
            for s in self.miss[b]:
                self.bad[b, s] = rng.integers(0, 256, L, dtype=np.uint8)
        self.bad.setflags(write=False)
        # the expectation by construction (None: the model's), then the model's
        self.built = [self.construct(b) for b in range(B)]
        self.want = np.zeros(B, dtype=np.int32)
        self.sets = [frozenset()] * B
        for b in range(B):
            self.want[b], self.sets[b] = model_block(gf, k, m, set(range(n)) - self.miss[b], self.bad[b], L, max_bad, mult)
            if self.built[b] is None and self.want[b] > 0:
                # a class a block that ends located heals to the codeword through the other present shards
                rest = sorted(set(range(n)) - self.miss[b] - self.sets[b])
                for x in self.cols[b]:
                    f = xdot(gf[0], plan(gf, rest, k)[0], unscale(gf, rest, self.bad[b][rest, x], mult)[:, None])[:, 0]
                    self.final[b, :, x] = poly_eval(gf, f, range(n))
                    if mult is not None:
                        self.final[b, :, x] = gf[0][np.asarray(mult, dtype=np.uint8), self.final[b, :, x]]
        self.final.setflags(write=False)

    def erasures(self, e):
        """e missing shards, the same for every block of the batch with this e (the model's work per set
        of present shards is done once): shard 0, a parity shard, then random ones."""
        rng = np.random.default_rng(7 * self.n + e)
        first = [0, self.k + int(rng.integers(self.m))]
        rest = [int(s) for s in rng.permutation(self.n) if s not in first]
        return set((first + rest)[:e])

    def construct(self, b):
        cols = self.cols[b].values()
        if any(c.want is MODEL for c in cols):
            return None
        if any(c.want is None for c in cols):
            return UNKNOWN, frozenset()
        U = frozenset().union(*[c.want for c in cols])
        return (len(U), U) if len(U) <= self.T[b] else (UNKNOWN, frozenset())

    def arena(self, layout):
        """(image, clean image, data region, parity region): the batch in a layout's arena."""
        k, L, B = self.k, self.L, self.B
        clean, data, par = oracle_arena(self.oracle, layout, k, self.m, L, B, np.random.default_rng(self.seed))
        assert np.array_equal(shards(clean, data, par)[:, :, :L], self.clean)
        img = clean.copy()
        img[data.index(0, L)] = self.bad[:, :k]
        img[par.index(0, L)] = self.bad[:, k:]
        rng = np.random.default_rng(self.seed + 1)
        for b in range(B):                      # a missing slot holds garbage over its whole stride
            for s in sorted(self.miss[b]):
                at = data.at(b, s) if s < k else par.at(b, s - k)
                img[at + L:at + data.ss] = rng.integers(0, 256, data.ss - L, dtype=np.uint8)
        return img, clean, data, par


def cases(oracle, gf, call, k, m, L, max_bad, v=None):
    """The batch, built once. v: the multipliers of the code that `oracle` encodes."""
    key = (call, k, m, L, max_bad) + (() if v is None else (bytes(bytearray(int(x) for x in v)),))
    if key not in _CACHE:
        _CACHE[key] = Cases(oracle, gf, call, k, m, L, max_bad, v)
    return _CACHE[key]


def params(cauchy=False, lens=None):
    """(call, k, m, L, max_bad) of every batch; cauchy: of the batches under the Cauchy code (lens: at
    other lengths than those the device runs)."""
    codes, lens = (CAUCHY_CODES, lens or CAUCHY_LENS) if cauchy else (CODES, lens or LENS)
    return [(call, k, m, L, mb) for call in ("multi", "partial") for k, m in codes for L in lens
            for mb in max_bads(k, m)]
