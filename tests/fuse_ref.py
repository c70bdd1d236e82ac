"""The fused-search rule (include/vsearch.h "Fused search") in numpy, and the
key-list fixtures the CPU and GPU tests share.

A list is a uint64 array of k_in keys as vs_search_keys writes them (sorted
descending, no repeats, 0-padded); a fused query is an array [n_sub][k_in].
``rrf`` works in np.float32 and adds the terms in ascending l, starting from
the first term; ``dbsf`` forms the per-list statistics and every term in
float64, rounds each term to fp32 once and adds those in the same order, and
also returns the unrounded float64 sums.
"""
import numpy as np

MAX_LISTS = 8
MAX_LIMIT = 128
RRF, DBSF = 0, 1
ROW_MASK = np.uint64(0xFFFFFFFF)


def key_encode(scores, rows):
    """vs_key_encode over arrays (include/vsearch.h "Result key layout")."""
    s = np.asarray(scores, np.float32).copy()
    s[s == 0] = 0.0
    u = s.view(np.uint32)
    o = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return (o.astype(np.uint64) << np.uint64(32)) | (ROW_MASK - np.asarray(rows, np.uint64))


def key_score(keys):
    o = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)
    u = np.where(o & 0x80000000, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return u.view(np.float32)


def key_row(keys):
    return ROW_MASK - (np.asarray(keys, np.uint64) & ROW_MASK)


def _top(fused32, k):
    """{row: np.float32} -> [k] keys, descending, 0-padded."""
    out = np.zeros(k, np.uint64)
    if fused32:
        rows = np.fromiter(fused32.keys(), np.uint64, len(fused32))
        sc = np.array([fused32[int(r)] for r in rows], np.float32)
        keys = np.sort(key_encode(sc, rows))[::-1][:k]
        out[:len(keys)] = keys
    return out


def _sum_terms(lists, term_of, order):
    """{row: fp32 sum of term_of(l)[p] over the lists holding row}, added in
    `order` of l (the rule: ascending), starting from the first term."""
    fused = {}
    ls = range(len(lists)) if order == "asc" else range(len(lists) - 1, -1, -1)
    for l in ls:
        terms = np.asarray(term_of(l)).astype(np.float32)   # each term rounded to fp32 once
        rows = key_row(lists[l]).tolist()
        for p in np.flatnonzero(lists[l]).tolist():
            row, t = rows[p], terms[p]
            fused[row] = t if row not in fused else np.float32(fused[row] + t)
    return fused


def rrf_scores(lists, rrf_k=0, order="asc"):
    K = int(rrf_k) or 2
    lists = np.asarray(lists, np.uint64)
    # fp32 division of exact operands: numpy's float32 divide is IEEE, rounded once
    terms = np.float32(1.0) / (np.arange(lists.shape[1]) + K).astype(np.float32)
    return _sum_terms(lists, lambda l: terms, order)


def rrf(lists, k, rrf_k=0):
    """One fused query: [n_sub][k_in] keys -> [k] keys carrying the fused score."""
    return _top(rrf_scores(np.asarray(lists, np.uint64), rrf_k), k)


def dbsf_terms(lst):
    """The float64 terms of one list's slots (NaN in empty slots)."""
    lst = np.asarray(lst, np.uint64)
    live = lst != 0
    s = key_score(lst).astype(np.float64)
    n = int(live.sum())
    t = np.full(len(lst), np.nan)
    if n == 0:
        return t
    mu = s[live].sum() / n
    sigma = np.sqrt(((s[live] - mu) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    if n == 1 or sigma == 0:
        t[live] = 0.5
    else:
        t[live] = (s[live] - (mu - 3 * sigma)) / (6 * sigma)
    return t


def dbsf(lists, k):
    """([k] keys from the fp32 sums of the once-rounded terms, {row: float64 sum
    of the unrounded terms})."""
    lists = np.asarray(lists, np.uint64)
    terms = [dbsf_terms(l) for l in lists]
    fused32 = _sum_terms(lists, lambda l: np.nan_to_num(terms[l]), "asc")
    fused64 = {}
    for l, lst in enumerate(lists):
        rows = key_row(lst).tolist()
        for p in np.flatnonzero(lst).tolist():
            fused64[rows[p]] = fused64.get(rows[p], 0.0) + float(terms[l][p])
    return _top(fused32, k), fused64


def fuse(lists, k, fusion=RRF, rrf_k=0):
    return rrf(lists, k, rrf_k) if fusion == RRF else dbsf(lists, k)[0]


# ---- fixtures: [nq][n_sub][k_in] key arrays ------------------------------------
def _list(rows, scores=None):
    """A well-formed list over `rows` in rank order (scores default to a
    strictly descending ramp, so the keys are sorted descending)."""
    rows = np.asarray(rows, np.uint64)
    if scores is None:
        scores = 1.0 - np.arange(len(rows), dtype=np.float32) / 256
    return key_encode(scores, rows)


def overlap(nq, n_sub=8, k_in=128, pool=160, seed=1, row0=0):
    """Every list is the first k_in of a random permutation of a pool of rows."""
    rng = np.random.default_rng(seed)
    out = np.zeros((nq, n_sub, k_in), np.uint64)
    for q in range(nq):
        for l in range(n_sub):
            out[q, l] = _list(row0 + rng.permutation(pool)[:k_in])
    return out


def disjoint(nq, n_sub, k_in, seed=2):
    """No row in two lists: every rank-p entry ties with the other lists' rank-p
    entries, so the answer is the rank-0 rows by row ascending, then rank 1, ..."""
    rng = np.random.default_rng(seed)
    out = np.zeros((nq, n_sub, k_in), np.uint64)
    for q in range(nq):
        rows = rng.permutation(n_sub * k_in + 50)[:n_sub * k_in].reshape(n_sub, k_in)
        for l in range(n_sub):
            out[q, l] = _list(rows[l])
    return out


def reversed_pair(nq, k_in=128, seed=3):
    """Two lists holding the same rows in opposite order: rows p and k_in-1-p tie
    exactly (a + b == b + a)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((nq, 2, k_in), np.uint64)
    for q in range(nq):
        rows = rng.permutation(4 * k_in)[:k_in]
        out[q, 0] = _list(rows)
        out[q, 1] = _list(rows[::-1])
    return out


def identical(nq, n_sub, k_in, seed=4):
    rng = np.random.default_rng(seed)
    out = np.zeros((nq, n_sub, k_in), np.uint64)
    for q in range(nq):
        out[q, :] = _list(rng.permutation(3 * k_in)[:k_in])
    return out
