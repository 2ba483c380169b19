"""A model of the Cauchy code (klauspost WithCauchyMatrix, fec_hip_matrix.h kind 1) for the tests:
plain numpy over GF(2^8), polynomial 0x11D, from the definitions alone.

The matrix is built from its definition (identity on top, 1 / (r ^ c) below), parity is the matrix
applied by table lookups, and missing shards are rebuilt by Gaussian elimination on the rows of the
first k present shards. Nothing here interpolates over the shard indices, which is how the library
decodes, so the model is independent of what it checks. Every function takes the matrix, so the same
code serves the default matrix (fec.rs_matrix) where a test needs both.
"""
import numpy as np

EXP = np.zeros(512, dtype=np.uint8)
LOG = np.zeros(256, dtype=np.int32)
_v = 1
for _i in range(255):
    EXP[_i] = _v
    LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D
EXP[255:510] = EXP[:255]
_a = np.arange(256)
MUL = np.zeros((256, 256), dtype=np.uint8)       # MUL[a, b] = a * b
MUL[1:, 1:] = EXP[LOG[_a[1:], None] + LOG[None, _a[1:]]]
INV = np.zeros(256, dtype=np.uint8)              # INV[a] = 1 / a (INV[0] = 0)
INV[1:] = EXP[255 - LOG[_a[1:]]]


def matrix(k, m):
    """The n x k Cauchy matrix: identity on top, M[r][c] = 1 / (r ^ c) for r >= k."""
    M = np.zeros((k + m, k), dtype=np.uint8)
    M[:k] = np.eye(k, dtype=np.uint8)
    r, c = np.meshgrid(np.arange(k, k + m), np.arange(k), indexing="ij")
    M[k:] = INV[r ^ c]
    return M


def apply(rows, x):
    """rows [r, k] applied to x [..., k, L]: out[..., i, :] = XOR_j rows[i, j] * x[..., j, :]."""
    out = np.zeros(x.shape[:-2] + (rows.shape[0], x.shape[-1]), dtype=np.uint8)
    for i in range(rows.shape[0]):
        for j in range(rows.shape[1]):
            if rows[i, j]:
                out[..., i, :] ^= MUL[rows[i, j]][x[..., j, :]]
    return out


def encode(M, data):
    """Parity [..., m, L] of data [..., k, L] under the n x k matrix M."""
    return apply(M[data.shape[-2]:], data)


def invert(A):
    """Inverse of a square matrix by Gauss-Jordan elimination; None if singular."""
    n = A.shape[0]
    a = np.concatenate([A.astype(np.uint8), np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        piv = np.nonzero(a[c:, c])[0]
        if piv.size == 0:
            return None
        p = c + int(piv[0])
        if p != c:
            a[[c, p]] = a[[p, c]]
        a[c] = MUL[INV[a[c, c]]][a[c]]
        f = a[:, c].copy()
        f[c] = 0
        a ^= MUL[f[:, None], a[c][None, :]]
    return a[:, n:]


def decode_rows(M, present):
    """For a block whose present shards are `present` (bool [n]): (S, T) with S the first k present
    shard indices and T [n, k] the rows that give every shard from the shards S, T = M * inverse(M[S]);
    None when fewer than k are present."""
    k = M.shape[1]
    S = np.nonzero(present)[0][:k]
    if S.size < k:
        return None
    inv = invert(M[S])
    assert inv is not None, "k rows of the matrix are dependent"
    T = np.zeros(M.shape, dtype=np.uint8)
    for t in range(k):
        T ^= MUL[M[:, t][:, None], inv[t][None, :]]
    return S, T


_ROWS = {}


def rebuild(M, shards, present):
    """Every shard [n, L] of one block from the first k present ones of `shards` [n, L]."""
    key = (M.tobytes(), M.shape, np.asarray(present, dtype=bool).tobytes())
    if key not in _ROWS:
        _ROWS[key] = decode_rows(M, np.asarray(present, dtype=bool))
    S, T = _ROWS[key]
    return apply(T, shards[S])


def mask_bits(mask, n):
    """bool [n] from an integer present mask (bit i = shard i)."""
    return np.array([(int(mask) >> i) & 1 for i in range(n)], dtype=bool)


def corrupt(rng, shard):
    """The shard with every byte changed (a nonzero difference in every byte)."""
    return shard ^ rng.integers(1, 256, shard.shape, dtype=np.uint8)
