"""Seeded inputs of the coreset tests and the numpy definition of the greedy selection (int64, exact).

The definition (csrc/coreset_pack.h, include/aaclip.h): rows are quantised once, q = clamp(rint(v * 2^14), -32767, 32767)
as int16 with round-half-even, norm2 = sum q^2 as int32 (saturated); d2(x, c) = norm2_x + norm2_c - 2 <q_x, q_c>;

    min_d2[i] = UINT32_MAX for all i;  radius2[0] = UINT32_MAX;  pick[0] = start
    for t = 0 .. n-1:  min_d2 = minimum(min_d2, d2(., pick[t]));  radius2[t+1] = max(min_d2)
                       pick[t+1] = the LOWEST i that attains it (np.argmax)

Five kinds of case, each fp32 unit rows [N, E]:
  clusters    10 planted random unit centres (pairwise distance near sqrt 2), row i = unit(centre[i % 10] + 0.05 * unit
              noise): the noise is small against the separation, so 10 picks hit 10 clusters
  random      random unit rows
  duplicates  5 distinct random unit rows, each repeated 4 times (row i = base[i % 5]; N = 20): the radius is 0 after 5 picks
  antipodal   pairs v, -v (rows 2k, 2k + 1): d2 reaches 2^30
  ties        the signed basis vectors e_0, -e_0, e_1, -e_1, ... (N <= 2E): every pair that is not antipodal is
              equidistant, so the lowest-index rule decides every pick

A smaller case is a prefix of a larger one (one draw per kind and E at the largest N).  definition() is the loop above
with one int64 matrix-vector product per pick; definition_gram() is the same selection from the Gram matrix of the
quantised rows, computed in float64 -- exact, because every partial sum is an integer below 2^53 (|q| < 2^15, E <= 1024:
below 2^40) -- which makes n = N = 2738 affordable; test_coreset_cpu.py holds the two equal."""
import functools
import math

import numpy as np

KINDS = ("clusters", "random", "duplicates", "antipodal", "ties")
NS = (1, 2, 65, 257, 2738)
ES = (32, 128, 768)
N_MAX = max(NS)
CLUSTERS = 10
D2_INIT = 0xFFFFFFFF
NORM2_LIMIT = 1 << 29
SCALE = 16384.0


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------- the definition
def quantise(rows):
    """fp32 rows [N, E] -> (q int16 [N, E], norm2 int32 [N])"""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.rint(np.asarray(rows, np.float32) * np.float32(SCALE))      # the product is exact; rint is half-even
    x = np.where(np.isnan(x), np.float32(0), x)
    q = np.clip(x, -32767, 32767).astype(np.int16)
    norm2 = np.minimum((q.astype(np.int64) ** 2).sum(axis=1), 0x7FFFFFFF).astype(np.int32)
    return q, norm2


def _greedy(n, start, N, column, snapshots=()):
    """the loop of the definition; column(c) -> int64 d2 of every row to row c"""
    min_d2 = np.full(N, D2_INIT, np.int64)
    radius2 = np.full(n + 1, D2_INIT, np.int64)
    picks = np.full(n, start, np.int64)
    kept = {}
    c = start
    for t in range(n):
        np.minimum(min_d2, column(c), out=min_d2)
        c = int(np.argmax(min_d2))                 # the lowest index among equal maxima
        radius2[t + 1] = min_d2[c]
        if t + 1 < n:
            picks[t + 1] = c
        if t + 1 in snapshots:
            kept[t + 1] = min_d2.astype(np.uint32)
    return picks.astype(np.int32), radius2.astype(np.uint32), min_d2.astype(np.uint32), kept


def definition(q, n, start=0):
    """-> (picks int32 [n], radius2 uint32 [n + 1], min_d2 uint32 [N]); int64 arithmetic throughout"""
    q64 = np.asarray(q).astype(np.int64)
    norm2 = (q64 * q64).sum(axis=1)
    return _greedy(n, start, q64.shape[0], lambda c: norm2 + norm2[c] - 2 * (q64 @ q64[c]))[:3]


def gram_d2(q):
    """all pairwise d2 as int64 [N, N], from a float64 Gram matrix that is checked to be exact"""
    qf = np.asarray(q).astype(np.float64)
    g = qf @ qf.T
    assert np.abs(g).max() < 2.0 ** 52 and np.array_equal(g, np.rint(g))
    g = g.astype(np.int64)
    norm2 = np.diagonal(g).copy()
    assert np.array_equal(norm2, (np.asarray(q).astype(np.int64) ** 2).sum(axis=1))
    return norm2[:, None] + norm2[None, :] - 2 * g


def definition_gram(q, n, start=0, snapshots=(), d2=None):
    """definition() from the pairwise distances; snapshots: pick counts at which min_d2 is kept as well
    -> (picks, radius2, min_d2, {count: min_d2})"""
    d2 = gram_d2(q) if d2 is None else d2
    return _greedy(n, start, d2.shape[0], lambda c: d2[c], snapshots)


# ---------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def _pool(kind, E):
    rng = np.random.default_rng([{"clusters": 41, "random": 42, "duplicates": 43, "antipodal": 44, "ties": 45}[kind], E])
    if kind == "clusters":
        centres = unit(rng.standard_normal((CLUSTERS, E)))
        rows = unit(centres[np.arange(N_MAX) % CLUSTERS] + 0.05 * unit(rng.standard_normal((N_MAX, E))))
    elif kind == "random":
        rows = unit(rng.standard_normal((N_MAX, E)))
    elif kind == "duplicates":
        rows = unit(rng.standard_normal((5, E))).astype(np.float32)[np.arange(20) % 5]
    elif kind == "antipodal":
        v = unit(rng.standard_normal(((N_MAX + 1) // 2, E))).astype(np.float32)
        rows = np.stack([v, -v], axis=1).reshape(-1, E)[:N_MAX]
    else:
        rows = np.zeros((2 * E, E), np.float32)
        rows[np.arange(2 * E), np.arange(2 * E) // 2] = np.where(np.arange(2 * E) % 2 == 0, 1.0, -1.0)
    rows = np.ascontiguousarray(rows.astype(np.float32))
    rows.setflags(write=False)
    return rows


def sizes(kind, E):
    """the N of the grid at which the kind exists"""
    if kind == "duplicates":
        return (20,)
    if kind == "ties":
        return tuple(N for N in NS if N <= 2 * E) + (2 * E,)
    return NS


def counts(N):
    """the n of the grid: 1, 2, ceil(N / 10), N where they are distinct and at most N"""
    return tuple(sorted({n for n in (1, 2, math.ceil(N / 10), N) if 1 <= n <= N}))


def starts(N):
    """row 0 and one interior row"""
    return (0,) if N < 3 else (0, (2 * N) // 3)


def case(kind, N, E):
    """-> fp32 unit rows [N, E], read-only"""
    rows = _pool(kind, E)
    assert N <= rows.shape[0], (kind, N, E)
    return rows[:N]


@functools.lru_cache(maxsize=None)
def quantised(kind, N, E):
    q, norm2 = quantise(case(kind, N, E))
    q.setflags(write=False)
    norm2.setflags(write=False)
    return q, norm2


@functools.lru_cache(maxsize=2)       # 60 MB each at N = 2738; a case's starts follow one another
def _pairwise(kind, N, E):
    return gram_d2(quantised(kind, N, E)[0])


@functools.lru_cache(maxsize=None)
def reference(kind, N, E, start):
    """The definition at n = N, once per case: -> (picks [N], radius2 [N + 1], {n: min_d2 after n picks} for the grid's n).
    By the prefix property picks[:n] and radius2[:n + 1] are the selection for n."""
    picks, radius2, _, kept = definition_gram(None, N, start, snapshots=counts(N), d2=_pairwise(kind, N, E))
    for a in (picks, radius2) + tuple(kept.values()):
        a.setflags(write=False)
    return picks, radius2, kept


def grid():
    """every (kind, N, E, n, start) of the grid"""
    for kind in KINDS:
        for E in ES:
            for N in sizes(kind, E):
                for n in counts(N):
                    for start in starts(N):
                        yield kind, N, E, n, start
