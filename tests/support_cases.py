"""Seeded inputs of the support-bank tests and the fp64 brute-force definition of the nearest bank row.

Four kinds of case, each a pair (queries fp32 [M, E], bank fp32 [N, E]) of unit rows:
  planted     bank rows are random unit vectors, query m is unit(bank[j_m] + 0.5 * unit(noise)): the fp64 gap between the
              best and the second-best cosine is >= 0.35 on every row at N = 2738 (test_support_cpu checks it at E = 64
              and 768; at E = 64 a typical seed gives a smallest gap of 0.31 over the 1369 rows, and the seed used here
              is the first of a scan that reaches 0.35), three hundred times the fp16 form's error bar, so the index is
              compared on every row
  random      random unit queries: values only (the top-2 gap is below 2.2e-3 on 7-19 % of the rows)
  antipodal   bank rows unit(c + 0.3 * noise) round one direction c, queries -unit(c + 0.3 * noise'): every cosine is
              near -0.9, and a padding column that contributed its 0 would win
  duplicates  the planted case with bank rows 0, 7 and N - 1 bit-equal (and 20 / 27, 40 / 47, ...): the planted
              queries aim at both copies, and the lower index must come back -- an exact tie in any arithmetic, since
              both columns see the same operands in the same K order

The generator draws the bank and the noise once per (kind, E) at the largest size and cuts them, so a smaller case is
a prefix of a larger one and the whole grid costs a few random draws."""
import functools

import numpy as np

KINDS = ("planted", "random", "antipodal", "duplicates")
MS = (1, 17, 129, 1369)
NS = (1, 127, 130, 2738)
ES = (64, 768)
M_MAX, N_MAX = max(MS), max(NS)

# derived bars against the fp64 definition (unit rows):
#   fp16 form  |fl(a).fl(b) - a.b| <= (2u + u^2) * sum|a_i b_i| <= 2u + u^2 = 9.8e-4 (u = 2^-11), plus E * 2^-24 <= 6.1e-5
#              for the fp32 accumulation; a maximum over j inherits the bound
#   fp32 form  E * 2^-24 <= 6.1e-5 at E <= 1024; the project's standing fp32 bar
BAR = {"fp16": 1.1e-3, "fp32": 1e-4}
PLANTED_GAP = 0.35


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _pool(kind, E):
    rng = np.random.default_rng([{"planted": 91, "random": 12, "antipodal": 13, "duplicates": 91}[kind], E])
    if kind == "antipodal":
        c = unit(rng.standard_normal(E))
        bank = unit(c + 0.3 * unit(rng.standard_normal((N_MAX, E))))
        q = -unit(c + 0.3 * unit(rng.standard_normal((M_MAX, E))))
        return bank, q
    bank = unit(rng.standard_normal((N_MAX, E)))
    return bank, unit(rng.standard_normal((M_MAX, E)))


def targets(M, N):
    """the bank row every planted query aims at: all residues, the first and the last row among them"""
    j = (np.arange(M, dtype=np.int64) * 7919 + (N - 1)) % N
    if M >= 3:
        j[1], j[2] = 0, min(7, N - 1)
    return j


@functools.lru_cache(maxsize=None)
def case(kind, M, N, E):
    """-> (q fp32 [M, E], bank fp32 [N, E]), read-only"""
    pool_bank, pool_q = _pool(kind, E)
    bank = pool_bank[:N].copy()
    if kind == "duplicates":
        for j in range(0, N - 7, 20):
            bank[j + 7] = bank[j]
        bank[N - 1] = bank[0]
    bank = bank.astype(np.float32)
    if kind in ("planted", "duplicates"):
        q = unit(bank[targets(M, N)].astype(np.float64) + 0.5 * pool_q[:M])
    else:
        q = pool_q[:M]
    q = np.ascontiguousarray(q.astype(np.float32))
    q.setflags(write=False)
    bank.setflags(write=False)
    return q, bank


def brute_force(q, bank):
    """The definition: fp64 cosines of the fp32 rows; -> (best fp64 [M], lowest index that attains it int64 [M])"""
    best = np.empty(q.shape[0], np.float64)
    idx = np.empty(q.shape[0], np.int64)
    b = bank.astype(np.float64).T
    for r0 in range(0, q.shape[0], 256):
        q64 = q[r0:r0 + 256].astype(np.float64)
        c = q64 @ b
        top = c.max(axis=1)
        for r in range(c.shape[0]):
            # a matrix product may sum the columns of its edge blocks in another order, so bit-equal bank rows need not
            # give bit-equal cosines there: the near-maxima are recomputed one by one with the same routine, and the
            # first of the equal ones wins
            near = np.flatnonzero(c[r] >= top[r] - 1e-9)
            exact = np.array([np.dot(q64[r], b[:, j]) for j in near])
            at = int(np.argmax(exact))
            best[r0 + r], idx[r0 + r] = exact[at], near[at]
    return best, idx


@functools.lru_cache(maxsize=None)
def reference(kind, M, N, E):
    best, idx = brute_force(*case(kind, M, N, E))
    best.setflags(write=False)
    idx.setflags(write=False)
    return best, idx


def top2_gap(q, bank):
    c = q.astype(np.float64) @ bank.astype(np.float64).T
    part = np.partition(c, -2, axis=1)
    return part[:, -1] - part[:, -2]


def index_is_checked(kind, N):
    return kind in ("planted", "duplicates") and N > 1 or N == 1


# ---- map stage: seeded unit tokens on a g x g grid and a small bank per level
def map_case(B, g, levels, E=64, shots=2, seed=5):
    """-> (seg tokens: per level fp32 [B, g*g, E], bank tokens: per level fp32 [shots, g*g, E]) of unit rows"""
    rng = np.random.default_rng([seed, B, g, levels])
    segs = [unit(rng.standard_normal((B, g * g, E))).astype(np.float32) for _ in range(levels)]
    banks = [unit(rng.standard_normal((shots, g * g, E))).astype(np.float32) for _ in range(levels)]
    return segs, banks
