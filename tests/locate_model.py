"""The definition of fec_rs_locate_multi_batch / fec_rs_locate_partial_batch for a code of any size, by a
Berlekamp-Welch decoder written in numpy over the ORACLE's field (the `gf` fixture: gf_mul as a table,
and its inverses). test_gpu_locate_multi.py and test_gpu_locate_partial.py try every set of shards,
which stops at n = 12; this model has no such limit and shares nothing with the library's solver: no
power sums, no locator recurrence, no root search.

A consistent block is, per byte column, the values at the points 0 .. n - 1 (shard r at the field
element r) of one polynomial of degree < k. test_locate_hard_cases.py asserts that on the oracle's
encode, so the model rests on the oracle and not on a comment of the library.

One column (bw_column): y_r at the present points P, the radius T. Find a nonzero pair (Q, E) with
deg Q < k + T, deg E <= T and Q(r) = y_r E(r) on P, by elimination on the |P| x (k + 2 T + 1) system,
done in two blocks: the Q part [r^j] depends on P alone and is reduced once per (P, k + T); what is
left is a (|P| - k - T) x (T + 1) system for E. If a codeword f lies within T of y, every solution has
Q = f E (Q ^ f E has degree < k + T and at least |P| - T >= k + T roots); so: no solution, E does not
divide Q, or deg(Q / E) >= k: no explanation of weight <= T. Otherwise the errors are the points where
Q / E differs from y.

One block (model_block): every distinct byte column of [0, L) that is not a codeword is decoded; a
column without explanation makes the block unknown; otherwise U is the union of the columns' error
sets and the result is (|U|, U), or unknown if |U| > T. This equals the definition (the smallest set of
at most T present shards whose replacement makes the present shards consistent): the present shards
are a code of distance m - e + 1 > 2 T, so each column's explanation of weight <= T is unique, any
explaining set of at most T shards contains each column's, hence contains U, and U itself explains.
"""
import numpy as np

UNKNOWN, TOO_FEW = -2, -3

_PLANS = {}


def xdot(mul, A, B):
    """The matrix product A B over the field."""
    return np.bitwise_xor.reduce(mul[A[:, :, None], B[None, :, :]], axis=1)


def reduce_rows(gf, G, ncols):
    """Gauss-Jordan on the first ncols columns of G, in place. Returns the pivot columns."""
    mul, inv = gf
    piv = []
    for c in range(ncols):
        row = len(piv)
        nz = np.flatnonzero(G[row:, c])
        if nz.size == 0:
            continue
        p = row + int(nz[0])
        if p != row:
            G[[row, p]] = G[[p, row]]
        G[row] = mul[inv[G[row, c]], G[row]]
        f = G[:, c].copy()
        f[row] = 0
        rows = np.flatnonzero(f)
        G[rows] ^= mul[f[rows][:, None], G[row][None, :]]
        piv.append(c)
    return piv


def powers(gf, pts, d):
    """[len(pts), d]: pts^j for j < d, with 0^0 = 1."""
    mul, _ = gf
    pts = np.asarray(pts, dtype=np.uint8)
    X = np.ones((pts.size, d), dtype=np.uint8)
    for j in range(1, d):
        X[:, j] = mul[X[:, j - 1], pts]
    return X


def plan(gf, P, d):
    """Row operations R with R [r^j]_{r in P, j < d} = [I_d; 0], as (R's first d rows, the others): the
    first give a polynomial of degree < d from its values on P, the others vanish on exactly the value
    vectors of such polynomials. d <= |P|."""
    key = (tuple(P), d)
    if key not in _PLANS:
        G = np.concatenate([powers(gf, P, d), np.eye(len(P), dtype=np.uint8)], axis=1)
        assert reduce_rows(gf, G, d) == list(range(d)), "distinct points: full column rank"
        assert not G[d:, :d].any()
        _PLANS[key] = (G[:d, d:].copy(), G[d:, d:].copy())
    return _PLANS[key]


def null_vector(gf, A):
    """A nonzero x with A x = 0, or None."""
    G = A.copy()
    piv = reduce_rows(gf, G, G.shape[1])
    free = [c for c in range(G.shape[1]) if c not in piv]
    if not free:
        return None
    x = np.zeros(G.shape[1], dtype=np.uint8)
    x[free[0]] = 1
    for i, c in enumerate(piv):
        x[c] = G[i, free[0]]
    return x


def poly_div(gf, q, e):
    """(quotient, remainder) of the polynomials q / e, coefficients in ascending order, e != 0."""
    mul, inv = gf
    de = int(np.flatnonzero(e)[-1])
    lead = inv[e[de]]
    rem = q.copy()
    quo = np.zeros(max(q.size - de, 1), dtype=np.uint8)
    for i in range(q.size - 1, de - 1, -1):
        c = mul[rem[i], lead]
        if c:
            quo[i - de] = c
            rem[i - de:i + 1] ^= mul[c, e[:de + 1]]
    return quo, rem


def poly_eval(gf, f, pts):
    mul, _ = gf
    pts = np.asarray(pts, dtype=np.uint8)
    v = np.zeros(pts.size, dtype=np.uint8)
    for c in f[::-1]:
        v = mul[v, pts] ^ c
    return v


def unscale(gf, P, Y, v):
    """Y (row i: the shard at point P[i]) with every row divided by its multiplier v[P[i]]: a codeword
    of a generalized Reed-Solomon code, shard r = v_r p(r), becomes the values p(r). v None: Y."""
    if v is None:
        return Y
    mul, inv = gf
    scale = inv[np.asarray(v, dtype=np.uint8)[[int(r) for r in P]]]
    assert scale.all(), "multipliers are not zero"
    return mul[scale.reshape((-1,) + (1,) * (np.ndim(Y) - 1)), Y]


def bw_column(gf, P, y, k, T, v=None):
    """The errors of the byte column y (y[i] at point P[i]) within T of a codeword: a frozenset of
    points of P, or None if no codeword lies within T. v: per-shard multipliers (see unscale); the
    column decoded is y_r / v_r, whose errors sit at the same points."""
    mul, _ = gf
    P = [int(r) for r in P]
    y = unscale(gf, P, np.asarray(y, dtype=np.uint8), v)
    assert len(P) == y.size and k + 2 * T <= len(P)
    top, null = plan(gf, P, k + T)
    A = mul[y[:, None], powers(gf, P, T + 1)]             # the E part of the system: y_r r^j
    E = null_vector(gf, xdot(mul, null, A))
    if E is None:
        return None
    Q = xdot(mul, top, xdot(mul, A, E[:, None]))[:, 0]    # the polynomial through y_r E(r)
    f, rem = poly_div(gf, Q, E)
    if rem.any() or f[k:].any():
        return None
    wrong = np.flatnonzero(poly_eval(gf, f[:k], P) != y)
    return frozenset(P[i] for i in wrong) if wrong.size <= T else None


def syndromes(gf, P, Y, k, v=None):
    """[|P| - k, L]: zero exactly in the byte columns of Y (row i: the shard at point P[i]) that are
    codewords (with multipliers v: whose rows divided by v are)."""
    return xdot(gf[0], plan(gf, [int(r) for r in P], k)[1], unscale(gf, P, Y, v))


def model_block(gf, k, m, present, y, L, max_bad, v=None):
    """One block by the definition: present (the shards the caller holds), y [n, >= L] its shards, v the
    code's multipliers (None: all one). Returns (result, frozenset): too few, 0, (|U|, U) or unknown."""
    n = k + m
    P = sorted(int(r) for r in present)
    e = n - len(P)
    if e > m:
        return TOO_FEW, frozenset()
    if len(P) <= k:
        return 0, frozenset()
    T = min(max_bad, (m - e) // 2)
    Y = unscale(gf, P, np.ascontiguousarray(y[P, :L]), v)
    bad = syndromes(gf, P, Y, k).any(axis=0)
    if not bad.any():
        return 0, frozenset()
    U = set()
    for col in np.unique(Y[:, bad], axis=1).T:
        s = bw_column(gf, P, col, k, T)
        if s is None:
            return UNKNOWN, frozenset()
        assert s, "a column that is no codeword has an error"
        U |= s
    return (len(U), frozenset(U)) if len(U) <= T else (UNKNOWN, frozenset())


def model_batch(gf, k, m, shards, L, max_bad, missing=None, v=None):
    """(results [B] int32, sets [B]) of a batch [B, n, >= L]; missing: per block the shards not held;
    v: the code's multipliers."""
    B, n = shards.shape[0], k + m
    want = np.zeros(B, dtype=np.int32)
    sets = [frozenset()] * B
    for b in range(B):
        present = set(range(n)) - set(missing[b] if missing else ())
        want[b], sets[b] = model_block(gf, k, m, present, shards[b], L, max_bad, v)
    return want, sets
