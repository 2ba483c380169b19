"""Test matrices and a decode model for custom code matrices (include/fec_hip_matrix.h
fec_ctx_set_custom_matrix, klauspost WithCustomMatrix): plain numpy over GF(2^8), polynomial 0x11D.

The matrices are defined here by formula; the arithmetic is tests/cauchy_model.py's, which takes any
matrix: parity by table lookups, rebuilds by Gaussian elimination on the whole k x k matrix of the
rows of the first k present shards (the library eliminates an e x e system instead). A custom code
need not be MDS, so decode() reports a singular block where cauchy_model.decode_rows would assert.
"""
import itertools

import numpy as np

from cauchy_model import INV, MUL, decode_rows, encode, invert, rebuild  # noqa: F401

NAMES = ["default", "cauchy255", "par1", "lrc"]


def gf_pow(a, n):
    v = 1
    for _ in range(n):
        v = int(MUL[v, a])
    return v


def rows(name, k, m, fec=None):
    """The m x k parity rows of a test matrix.
    default    the library's own matrix (fec.rs_matrix(k, m)[k:]): custom must equal kind 0
    cauchy255  P[i][j] = 1 / ((255 - i) ^ j): MDS, and not the built-in Cauchy rows
    par1       P[i][j] = (j + 1)^i
    lrc        (8, 4): ones on columns 0-3, ones on columns 4-7, then rows 0-1 of cauchy255"""
    i, j = np.meshgrid(np.arange(m), np.arange(k), indexing="ij")
    if name == "default":
        return fec.rs_matrix(k, m)[k:].copy()
    if name == "cauchy255":
        return INV[(255 - i) ^ j]
    if name == "par1":
        return np.array([[gf_pow(c + 1, r) for c in range(k)] for r in range(m)], dtype=np.uint8)
    if name == "lrc":
        assert (k, m) == (8, 4)
        P = np.zeros((4, 8), dtype=np.uint8)
        P[0, :4] = 1
        P[1, 4:] = 1
        P[2:] = rows("cauchy255", 8, 4)[:2]
        return P
    raise KeyError(name)


def matrix(P):
    """The n x k systematic matrix: identity on top, the parity rows P below."""
    k = P.shape[1]
    return np.concatenate([np.eye(k, dtype=np.uint8), P.astype(np.uint8)])


TOO_FEW, SINGULAR = "too few", "singular"
_DEC = {}


def decode(M, present):
    """What klauspost does with a block whose present shards are `present` (bool [n]): TOO_FEW with
    fewer than k of them, SINGULAR when the rows of the first k present are dependent, else
    cauchy_model.decode_rows' (S, T). Cached by the matrix and S (T depends on nothing else)."""
    k = M.shape[1]
    S = np.nonzero(present)[0][:k]
    if S.size < k:
        return TOO_FEW
    key = (M.tobytes(), M.shape, S.tobytes())
    if key not in _DEC:
        _DEC[key] = SINGULAR if invert(M[S]) is None else decode_rows(M, np.asarray(present, dtype=bool))
    return _DEC[key]


def patterns(n, k, lost):
    """bool [*, n] present rows: every pattern with a count in `lost` of the n shards missing, a data
    shard among them."""
    out = []
    for e in lost:
        for gone in itertools.combinations(range(n), e):
            if gone[0] < k:
                p = np.ones(n, dtype=bool)
                p[list(gone)] = False
                out.append(p)
    return np.array(out)


# What the (8, 4) test matrices must give over the 778 patterns with 1..4 missing shards, a data shard
# among them (checked with cauchy_model.invert): singular patterns per matrix.
SINGULAR_8_4 = {"default": 0, "cauchy255": 0, "par1": 8, "lrc": 172}


def check_8_4(name, P):
    """Assert that P is the (8, 4) matrix `name` as far as its singular patterns tell, so that a wrong
    matrix cannot pass silently; returns (patterns [778, 12], singular [778])."""
    M = matrix(P)
    pats = patterns(12, 8, range(1, 5))
    sing = np.array([decode(M, p) is SINGULAR for p in pats])
    assert len(pats) == 778 and int(sing.sum()) == SINGULAR_8_4[name], (name, len(pats), int(sing.sum()))
    lost = [tuple(np.nonzero(~p)[0]) for p in pats[sing]]
    if name == "par1":
        assert lost[0] == (0, 1, 2, 10)
    if name == "lrc":
        assert (4,) in lost                                   # column 4 of parity row 0 is zero
        assert (0, 4, 8) not in lost and P[1, 0] == 0         # solvable, but the leading pivot is zero
    return pats, sing
