"""Cases of the wide reconstruct-some tests (test_gpu_some_wide.py, test_gpu_heal_wide.py,
test_gpu_some_wide_far.py): fec_rs_reconstruct_some_wide_batch (include/fec_hip_some_wide.h) on codes of
up to 256 shards. No device is needed here; test_some_wide_cases.py checks this module on the CPU.

A batch deals its blocks the kinds the code can have, as test_gpu_some.make_masks numbers them:
  0 intact, 1 parity-only loss, 2 one data shard lost, 3 mixed data and parity loss of exactly m shards,
  4 exactly k present and all of them parity (m >= k), 5 k - 1 present.
The expected bytes of every rebuilt shard come from the oracle alone and not from the library:
row o of a recoverable block is  M[o] * inverse(M[first k present]) * (the first k present shards),  M
from oracle.build_matrix, the inverse from oracle.invert, the products from oracle.gf_mul; and for every
recoverable block those bytes must equal the oracle's encode (each shard has one right value).
"""
import numpy as np

ERASED = 0x5A
B = 67            # one wave per block, four blocks per plan workgroup: the last workgroup is ragged
TOO_FEW = -4
CODES = [(20, 13), (33, 32), (64, 16), (16, 240), (128, 128), (1, 255), (255, 1), (40, 0)]
BOUNDARY = [31, 32, 63, 64]      # the shards either side of a mask word boundary

_mul = []


def mul_table(oracle):
    """MUL[a, b] = the oracle's gf_mul(a, b)."""
    if not _mul:
        t = np.zeros((256, 256), dtype=np.uint8)
        for a in range(256):
            for b in range(a, 256):
                t[a, b] = t[b, a] = oracle.gf_mul(a, b)
        t.setflags(write=False)
        _mul.append(t)
    return _mul[0]


def kinds_of(k, m):
    return sorted([0, 5] + ([1, 2] if m >= 1 else []) + ([3] if m >= 2 else []) + ([4] if m >= k else []))


def pick(rng, pool, count, first=()):
    """`count` distinct members of pool: those of `first` that are in it, then random others."""
    pool = [int(i) for i in pool]
    got = [i for i in dict.fromkeys(int(i) for i in first) if i in pool][:count]
    rest = [i for i in pool if i not in got]
    rng.shuffle(rest)
    return got + rest[:count - len(got)]


def lost_row(rng, k, m, kind, boundary):
    """The lost shards (bool [n]) of one block of a kind; boundary: lose the mask word boundary shards
    first, where the kind leaves a choice."""
    n = k + m
    first = BOUNDARY if boundary else ()
    row = np.zeros(n, dtype=bool)
    if kind == 1:
        row[pick(rng, range(k, n), int(rng.integers(1, m + 1)), first)] = True
    elif kind == 2:
        row[pick(rng, range(k), 1, first)] = True
    elif kind == 3:
        e_d = int(rng.integers(1, min(k, m - 1) + 1))
        row[pick(rng, range(k), e_d, first)] = True
        row[pick(rng, range(k, n), m - e_d, first)] = True
    elif kind == 4:
        row[:] = True
        row[pick(rng, range(k, n), k, first)] = False
    elif kind == 5:
        row[:] = True
        row[pick(rng, range(n), k - 1)] = False
    return row


def make_lost(rng, k, m, B=B):
    """(lost bool [B, n], kind [B]): the kinds of kinds_of(k, m) dealt in turn and shuffled; the first
    block of each kind prefers the boundary shards."""
    kinds = kinds_of(k, m)
    kind = np.array((kinds * (B // len(kinds) + 1))[:B])
    rng.shuffle(kind)
    seen = set()
    lost = np.zeros((B, k + m), dtype=bool)
    for b in range(B):
        lost[b] = lost_row(rng, k, m, int(kind[b]), kind[b] not in seen)
        seen.add(kind[b])
    return lost, kind


def check_kinds(lost, kind, k, m):
    """Every kind the code can have is in the batch, and each block is of the kind it is dealt."""
    n = k + m
    assert sorted(set(kind.tolist())) == kinds_of(k, m)
    nl, nd = lost.sum(axis=1), lost[:, :k].sum(axis=1)
    for b, kd in enumerate(kind.tolist()):
        if kd == 0:
            assert nl[b] == 0
        elif kd == 1:
            assert nd[b] == 0 and 1 <= nl[b] <= m
        elif kd == 2:
            assert nd[b] == 1 and nl[b] == 1
        elif kd == 3:
            assert nl[b] == m and 1 <= nd[b] < m
        elif kd == 4:
            assert nd[b] == k and n - nl[b] == k
        else:
            assert n - nl[b] == k - 1


def rebuild_rows(oracle, k, n, lost_b, block):
    """The lost shards of one block [n, L] from its first k present ones, or None with fewer than k
    present: {shard o: M[o] * inverse(M[S]) * block[S]}."""
    have = np.flatnonzero(~lost_b)
    if len(have) < k:
        return None
    MUL = mul_table(oracle)
    M = oracle.build_matrix(k, n)
    S = have[:k]
    inv = oracle.invert(M[S])
    src = block[S]
    out = {}
    for o in np.flatnonzero(lost_b):
        coef = np.zeros(k, dtype=np.uint8)          # M[o] * inv
        for t in np.flatnonzero(M[o]):
            coef ^= MUL[M[o, t], inv[t]]
        out[int(o)] = np.bitwise_xor.reduce(MUL[coef[:, None], src], axis=0)
    return out


def make_case(oracle, k, m, L, lost, seed):
    """Host side of one batch: shards [B, n, L] with the oracle's parity, the damaged batch (lost shards
    0x5A), ok (k or more present) and full: the damaged batch with every lost shard of every ok block
    put back by rebuild_rows. For every ok block full equals the oracle's encode."""
    n, nb = k + m, len(lost)
    rng = np.random.default_rng(seed)
    sh = np.zeros((nb, n, L), dtype=np.uint8)
    sh[:, :k] = rng.integers(0, 256, (nb, k, L), dtype=np.uint8)
    if m:
        oracle.rs_encode(k, m, sh)
    ok = (~lost).sum(axis=1) >= k
    dmg = sh.copy()
    dmg[lost] = ERASED
    full = dmg.copy()
    for b in np.flatnonzero(ok & lost.any(axis=1)):
        for o, row in rebuild_rows(oracle, k, n, lost[b], dmg[b]).items():
            full[b, o] = row
    assert np.array_equal(full[ok], sh[ok]), "the inverse-matrix rows give the oracle's encode"
    c = dict(sh=sh, lost=lost.copy(), ok=ok, dmg=dmg, full=full)
    for a in c.values():
        a.setflags(write=False)
    return c


_cases = {}


def rs_case(oracle, k, m, L, B=B):
    """The batch of the full-reconstruct tests, computed once per (code, length)."""
    key = (k, m, L, B)
    if key not in _cases:
        rng = np.random.default_rng(100000 * k + 1000 * m + L)
        lost, kind = make_lost(rng, k, m, B)
        check_kinds(lost, kind, k, m)
        c = make_case(oracle, k, m, L, lost, 7 * L + k)
        c["kind"] = kind
        _cases[key] = c
    return _cases[key]


def bits(masks, n):
    """uint32 [B, W] masks -> bool [B, n]."""
    masks = np.ascontiguousarray(masks, dtype=np.uint32)
    return np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def stray(masks, n, rng=None):
    """The masks with every bit at and above n set (rng: drawn)."""
    out = np.array(masks, dtype=np.uint32)
    Bn, W = out.shape
    hi = np.ones((Bn, 32 * W), dtype=bool) if rng is None else rng.integers(0, 2, (Bn, 32 * W)).astype(bool)
    hi[:, :n] = False
    return out | np.packbits(hi, axis=1, bitorder="little").view("<u4").reshape(Bn, W)


# ---------------------------------------------------------------- the far cases

FAR_CODE = (33, 32)
FAR_LENS = (33, 1202)


def far_lost(k, m):
    """bool [5, n] for the far layouts (far_cases.py), mixed data and parity loss: block 0 intact, block
    1 k - 1 present, block 2 one data shard and one parity shard, block 3 parity only (the last among
    them), block 4 its farthest data shard, some more, and the first parity shards, m in all: it reads
    the last parity shards and writes the first."""
    n = k + m
    lost = np.zeros((5, n), dtype=bool)
    lost[1, k:] = True
    lost[1, 0] = True
    lost[2, [k // 2, k]] = True
    lost[3, [k, n - 1]] = True
    e_d = min(k, m) // 2
    lost[4, [k - 1] + list(range(0, k - 1, 2))[:e_d - 1]] = True
    lost[4, k:k + m - e_d] = True
    assert lost[4].sum() == m and lost[4, :k].sum() == e_d
    return lost
