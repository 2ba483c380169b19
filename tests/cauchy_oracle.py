"""A stand-in for the `oracle` fixture under the Cauchy code: the three members that the arena and the
locate helpers use (rs_encode in place, build_matrix, gf_mul), over the definition model of
cauchy_model.py. arena.oracle_arena, test_gpu_locate.model_verdicts and the brute-force models of the
locate tests take it in place of the oracle without change.

multipliers(M) gives, from a generator matrix alone, the per-shard multipliers v_r with which the
code is a generalized Reed-Solomon code on the points 0 .. n - 1: shard r of a codeword is
v_r p(r) for one polynomial p of degree < k per byte column. With
l_c(x) = prod_{j < k, j != c} (x ^ j) / (c ^ j):

    v_0 = 1,    v_r = M[r][0] / l_0(r) for r >= k,    v_c = v_k l_c(k) / M[k][c] for 0 < c < k,

and the function asserts M[r][c] == v_r l_c(r) / v_c for every parity r and data c, which is the
proof. Nothing here is taken from the library (rs_matrix.hpp, its log v table) or from its tests.
test_cauchy_oracle.py checks this module on the CPU.
"""
import numpy as np

import cauchy_model as cm

_M = {}


def gf_mul(a, b):
    return int(cm.MUL[a, b])


def build_matrix(k, n):
    """The n x k Cauchy matrix (the signature of oracle.build_matrix)."""
    if (k, n) not in _M:
        _M[k, n] = cm.matrix(k, n - k)
        _M[k, n].setflags(write=False)
    return _M[k, n]


def rs_encode(k, m, shards, threads=0):
    """Parity into shards[..., k:, :] from shards[..., :k, :], in place."""
    assert shards.shape[-2] == k + m
    if m:
        shards[..., k:, :] = cm.encode(build_matrix(k, k + m), shards[..., :k, :])
    return shards


def gf():
    """The field as the `gf` fixture gives it: (MUL, INV)."""
    return cm.MUL, cm.INV


def lagrange(k, c, x):
    """l_c(x) = prod_{j < k, j != c} (x ^ j) / (c ^ j)."""
    num = den = 1
    for j in range(k):
        if j != c:
            num, den = int(cm.MUL[num, x ^ j]), int(cm.MUL[den, c ^ j])
    return int(cm.MUL[num, cm.INV[den]])


def multipliers(M):
    """uint8 [n]: the v_r of the n x k generator M (identity on top), from M alone."""
    M = np.asarray(M, dtype=np.uint8)
    n, k = M.shape
    assert np.array_equal(M[:k], np.eye(k, dtype=np.uint8))
    mul, inv = cm.MUL, cm.INV
    v = np.ones(n, dtype=np.uint8)
    if n == k:
        return v
    for r in range(k, n):
        v[r] = mul[M[r, 0], inv[lagrange(k, 0, r)]]
    for c in range(1, k):
        v[c] = mul[mul[v[k], lagrange(k, c, k)], inv[M[k, c]]]
    assert v.all()
    for r in range(k, n):
        for c in range(k):
            assert M[r, c] == mul[mul[v[r], lagrange(k, c, r)], inv[v[c]]], (r, c)
    return v


def code_multipliers(k, m):
    """The multipliers of the Cauchy code RS(k, k + m)."""
    return multipliers(build_matrix(k, k + m))
