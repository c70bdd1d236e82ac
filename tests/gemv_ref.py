"""Reference and data of the plain one-query scan's stage tests
(tests/test_gemv_stages_gpu.py on the device, tests/test_gemv_ref.py on the
CPU). No GPU, no torch: numpy only. Nothing here models a lane, a chunk or a
summation order: a result key is a function of the row's score and number, a
list is the top k of the rows its workgroup walks, and which workgroup walks
a row follows from the row number alone.

    key(s, row) = image(s) << 32 | (0xFFFFFFFF - row)      (include/vsearch.h)

with image() the order-preserving u32 of the fp32 score, -0.0 as +0.0
(rsel_ref.score_ord; q8_gemv_ref.image is the same function).

Data:
  exact    rows and query are integers in [-3, 3] (exact in bf16), so every
           product and every partial sum in any order is an integer below
           9 * 4096 = 36,864 < 2^24: an exact fp32 number. The device score
           has to equal float32(int64 dot) bit for bit whatever the lane
           layout. Scores tie heavily, so the row word decides most ranks.
           Row 0 is all zero, row 1 the query, row 2 minus the query.
  one-hot  X[r, r mod dim] = 1 and q[d] = d + 1: the score of row r is
           (r mod dim) + 1, and a wrong score names the column that was read.
  real     the oracle's generator rows and a scaled, non-unit query.
"""
import numpy as np

import q8_gemv_ref as G
import rsel_ref as R

U64 = np.uint64
WAVES = 8                      # waves per scan workgroup
TABLE_DIMS = (128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096)  # compiled shapes
EXACT_MAX = 3                  # |entry| of the exact data
MIN_ROWS_PER_WAVE = 2          # the launcher's floor of a small scan's rows per wave


# ---- keys ----------------------------------------------------------------------
def make_key(score_f32, row):
    """vs::make_key: fp32 scores and global row numbers -> uint64 keys."""
    o = R.score_ord(np.asarray(score_f32, np.float32)).astype(U64)
    row = np.asarray(row, U64)
    assert row.size == 0 or int(row.max()) <= 0xFFFFFFFF, "row numbers are 32-bit"
    return (o << U64(32)) | (U64(0xFFFFFFFF) - row)


def key_row(keys):
    return (U64(0xFFFFFFFF) - (np.asarray(keys, U64) & U64(0xFFFFFFFF))).astype(np.int64)


def key_score(keys):
    return G.unimage((np.asarray(keys, U64) >> U64(32)).astype(np.uint32))


def topk_keys(scores, rows, row_base, k):
    """The k largest keys of the local rows `rows` with fp32 scores `scores`
    (one per listed row), descending, zero-padded to k."""
    keys = np.sort(make_key(scores, np.asarray(rows, U64) + U64(row_base)))[::-1][:k]
    out = np.zeros(k, U64)
    out[:keys.size] = keys
    return out


def topk_lists(keys, unit, nunits, k):
    """keys[i] belongs to list unit[i] (< nunits) -> [nunits, k]: each list's k
    largest keys, descending, zero-padded."""
    keys, unit = np.asarray(keys, U64), np.asarray(unit, np.int64)
    out = np.zeros((nunits, k), U64)
    if keys.size == 0:
        return out
    idx = np.argsort(keys, kind="stable")[::-1]
    idx = idx[np.argsort(unit[idx], kind="stable")]
    u = unit[idx]
    first = np.searchsorted(u, u, side="left")  # where each key's list starts
    rank = np.arange(u.size) - first
    keep = rank < k
    out[u[keep], rank[keep]] = keys[idx][keep]
    return out


# ---- who walks a row --------------------------------------------------------------
def rows_per_step(dim, bf16):
    """RB of GemvShape<dim, bf16>: a wave step covers RB whole rows, the fewest
    whose 16-byte chunks fill a multiple of 64 lanes. Table dimensions only."""
    assert dim in TABLE_DIMS
    cpr = dim // (8 if bf16 else 4)  # chunks per row
    return 64 // int(np.gcd(cpr, 64))


def owner(row, RB, nwaves):
    """The workgroup of local row `row` (or position, in a gathered scan) in
    the interleaved walk of `nwaves` waves: step = row // RB, wave = step mod
    nwaves, workgroup = wave // 8. owner_wave() is the middle term."""
    return owner_wave(row, RB, nwaves) // WAVES


def owner_wave(row, RB, nwaves):
    return (np.asarray(row, np.int64) // RB) % nwaves


def slice_grid(n_rows, cus):
    """-> (workgroups, rows per wave) of a scan whose waves take contiguous
    slices (any dimension outside the table): 3 workgroups a CU, fewer while a
    wave would get under MIN_ROWS_PER_WAVE rows."""
    want = min(cus * 3, (n_rows + WAVES * MIN_ROWS_PER_WAVE - 1) // (WAVES * MIN_ROWS_PER_WAVE))
    waves = max(want, 1) * WAVES
    rpw = max((n_rows + waves - 1) // waves, 1)
    return ((n_rows + rpw - 1) // rpw + WAVES - 1) // WAVES, rpw


def owner_slice_wave(row, rpw):
    return np.asarray(row, np.int64) // rpw


# ---- filter bitmaps ----------------------------------------------------------------
def pack_bits(mask, extra_past_end=False):
    """bool[n] -> uint64 words, bit r of word r // 64 = mask[r]; the bits past
    n in the last word are 0, or all 1 with extra_past_end."""
    n = mask.size
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = mask
    if extra_past_end:
        bits[n:] = 1
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").ravel().view(U64).copy()


def compact(words, n):
    """launch_compact_rows: the set bits among the first n, ascending."""
    bits = np.unpackbits(np.asarray(words, U64).view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).astype(np.uint32)


def compact_bitmaps(n, rng):
    """name -> words: the bitmaps launch_compact_rows is run on at n rows."""
    out = {"all ones": pack_bits(np.ones(n, bool)), "all zeros": pack_bits(np.zeros(n, bool)),
           "density 0.02": pack_bits(rng.random(n) < 0.02)}
    m = np.zeros(n, bool)
    m[[b for b in (0, 63, 64, n - 1) if b < n]] = True
    out["bits 0, 63, 64, n - 1"] = pack_bits(m)
    m = np.zeros(n, bool)
    m[n - 1] = True
    out["bit n - 1 alone"] = pack_bits(m)
    # whole 256-word blocks (16384 rows, one workgroup's share) empty between full ones
    blk = np.arange(n) // 16384
    out["alternate blocks"] = pack_bits(blk % 2 == 1)
    out["every third block"] = pack_bits(blk % 3 == 0)
    if n % 64:  # a last word whose bits past n are all set: they must not leak rows
        w = pack_bits(rng.random(n) < 0.5, extra_past_end=True)
        assert int(w[-1]) >> (n % 64) == (1 << (64 - n % 64)) - 1
        out["bits past n set"] = w
    return out


# ---- data ---------------------------------------------------------------------------
def exact_query(dim, negative=False, seed=0):
    """Integers in [-3, 3]; with `negative`, in [-3, -1]: an all-zero row's
    products are then all -0.0."""
    rng = np.random.default_rng([dim, seed, 1])
    q = rng.integers(-EXACT_MAX, 0 if negative else EXACT_MAX + 1, size=dim)
    if not q.any():
        q[0] = 1
    return q.astype(np.float32)


def exact_rows(n, q, seed=0):
    """n rows of integers in [-3, 3] (float32): row 0 all zero, row 1 = q,
    row 2 = -q (as far as n reaches), every odd row after them a copy of row
    r // 2 (itself a copy half the time), so that scores tie in groups whose
    rows lie steps, waves and workgroups apart."""
    dim = q.size
    rng = np.random.default_rng([dim, seed, 2])
    X = rng.integers(-EXACT_MAX, EXACT_MAX + 1, size=(n, dim)).astype(np.float32)
    for r in range(7, n, 2):
        X[r] = X[r // 2]
    special = (np.zeros(dim, np.float32), q, -q)
    for r in range(min(n, 3)):
        X[r] = special[r]
    return X


def exact_scores(X, q):
    """float32(int64 dot) of every row, and the builders' bound |dot| < 2^24."""
    d = X.astype(np.int64) @ q.astype(np.int64)
    assert np.array_equal(X, X.astype(np.int64)) and np.abs(X).max() <= EXACT_MAX
    assert np.abs(q).max() <= EXACT_MAX
    assert int(np.abs(d).max()) <= EXACT_MAX * EXACT_MAX * q.size < 1 << 24
    s = d.astype(np.float32)
    assert np.array_equal(s.astype(np.int64), d)
    return s


def onehot_rows(n, dim):
    X = np.zeros((n, dim), np.float32)
    X[np.arange(n), np.arange(n) % dim] = 1.0
    return X


def onehot_query(dim):
    return np.arange(1, dim + 1, dtype=np.float32)


def onehot_scores(n, dim):
    s = (np.arange(n) % dim + 1).astype(np.float32)
    assert dim < 1 << 24
    return s


def onehot_column(score):
    """The column a one-hot score says was read."""
    return int(round(float(score))) - 1


REAL_SCALE = 1.3  # the real query's length: the scan must not rely on unit queries


def real_rows(orc, n, dim, bf16):
    """The oracle generator's rows, as the collection dtype stores them."""
    return orc.generate(orc.SEED_CORPUS, 0, n, dim, bf16=bool(bf16))


def real_query(orc, dim):
    """Raw fp32 query of length REAL_SCALE (before any preprocessing)."""
    q = orc.generate(orc.SEED_QUERY, 3, 1, dim)[0] * np.float32(REAL_SCALE)
    assert abs(float(np.linalg.norm(q.astype(np.float64))) - REAL_SCALE) < 1e-3
    return q


def bar(s64):
    """The project's precision bar on a score whose fp64 value is s64."""
    return 1e-5 * np.abs(s64) + 1e-6
