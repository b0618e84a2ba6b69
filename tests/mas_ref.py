"""fp64 restatement of the monotonic alignment search of csrc/durations.hip (include/t2vae.h has the measure), for the tests.

a(t, j) = max(A[t, j], FLOOR) on the fp32 values (a NaN is the floor), ln in fp64 (np.log of the fp32 value); a path p has
p[0] = 0, p[n-1] = L - 1 and steps in 0..S; Q(0, 0) = ln a(0, 0), Q(t, j) = ln a(t, j) + max_s Q(t-1, j-s); on equal Q the
smallest step wins; cells outside the band j <= t S, L - 1 - j <= (n - 1 - t) S are -inf.  Shares no code with the kernel or
its wrapper; the floor is read from the header's text."""
import itertools
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 't2vae.h')


def _header_floor():
    m = re.search(r'#define\s+T2V_MAS_FLOOR\s+([0-9.eE+-]+)f', open(HEADER).read())
    return float(np.float32(float(m.group(1))))


FLOOR = _header_floor()                 # the fp32 value of the header's literal
LN_FLOOR = abs(float(np.log(np.float64(FLOOR))))


def feasible(n, L, S):
    return n >= 1 and L >= 1 and L - 1 <= (n - 1) * S


def log_weights(A, n, L):
    """ln a(t, j) in fp64 of the fp32 values A[:n, :L]"""
    a = np.asarray(A, dtype=np.float32)[:n, :L]
    a = np.where(a > np.float32(FLOOR), a, np.float32(FLOOR))          # a NaN compares false: the floor
    return np.log(a.astype(np.float64))


def search(A, n, L, S):
    """The best path of one row.  Returns dict(path (n,), durations (L,), starts (L,), score = Q(n-1, L-1) / n, total =
    Q(n-1, L-1)); None for a row without a feasible path."""
    if not feasible(n, L, S):
        return None
    la = log_weights(A, n, L)
    Q = np.full((n, L), -np.inf)
    D = np.zeros((n, L), dtype=np.int64)
    for t in range(n):
        for j in range(L):
            if not (j <= t * S and L - 1 - j <= (n - 1 - t) * S):
                continue
            if t == 0:
                Q[t, j] = la[t, j]
                continue
            best, arg = Q[t - 1, j], 0
            for s in range(1, S + 1):
                if j - s >= 0 and Q[t - 1, j - s] > best:              # strictly larger only: the smallest step wins
                    best, arg = Q[t - 1, j - s], s
            Q[t, j] = la[t, j] + best
            D[t, j] = arg
    path = np.zeros(n, dtype=np.int64)
    j = L - 1
    for t in range(n - 1, -1, -1):
        path[t] = j
        j -= D[t, j]
    assert j == 0 or n == 0
    out = segments(path, L)
    out.update(path=path, score=Q[n - 1, L - 1] / n, total=Q[n - 1, L - 1])
    return out


def segments(path, L):
    """durations (frames per symbol) and starts (their prefix sums) of a monotonic path over L symbols"""
    durations = np.bincount(np.asarray(path, dtype=np.int64), minlength=L)
    starts = np.concatenate([[0], np.cumsum(durations)[:-1]])
    return dict(durations=durations, starts=starts)


def path_score(A, path, L):
    """sum over the frames of ln a(t, path[t]) in fp64, for any path"""
    path = np.asarray(path, dtype=np.int64)
    la = log_weights(A, len(path), L)
    return float(la[np.arange(len(path)), path].sum())


def is_feasible_path(path, n, L, S):
    path = np.asarray(path, dtype=np.int64)
    if len(path) != n or path[0] != 0 or path[-1] != L - 1:
        return False
    step = np.diff(path)
    return bool((step >= 0).all() and (step <= S).all())


def brute_force(A, n, L, S):
    """(best total, every path that reaches it) over all feasible paths, by enumeration of the steps"""
    la = log_weights(A, n, L)
    best, paths = -np.inf, []
    for steps in itertools.product(range(S + 1), repeat=n - 1):
        if sum(steps) != L - 1:
            continue
        path = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
        total = float(la[np.arange(n), path].sum())
        if total > best:
            best, paths = total, [path]
        elif total == best:
            paths.append(path)
    return best, paths


def gap_bound(n):
    """How far the fp64 score of the kernel's path may lie below the fp64 optimum, from the fp32 recurrence alone.  A cell of Q
    is one logf and one add per frame: after t + 1 frames it carries at most (t + 1) (2^-24 M + e_log), where M = n |ln FLOOR|
    bounds |Q| (each term lies in [ln FLOOR, 0] for weights <= 1) so 2^-24 M bounds the rounding of one add, and e_log = one
    ulp of |ln FLOOR| is logf's stated error (1 ulp) on the largest magnitude it returns.  The kernel's optimum is within
    n (2^-24 M + e_log) of the true score of its own path, and the true optimum's fp32 value within the same of its true
    score; the kernel prefers its own, so the gap is at most 2 n (2^-24 M + e_log)."""
    M = n * LN_FLOOR
    e_log = float(np.spacing(np.float32(LN_FLOOR)))
    return 2.0 * n * (2.0 ** -24 * M + e_log)
