"""Reference and input patterns of the large-k selection's stage tests
(tests/test_rsel_stages_gpu.py on the device, tests/test_rsel_patterns.py on
the CPU). No GPU, no torch: numpy only.

A selection's input is `sc`, one u32 score image per row (order-preserving,
0 = masked); its keys are
    key(r) = sc[r] << 32 | (0xFFFFFFFF - (row_base + r))      for sc[r] != 0
and its answer the keff largest of them. csrc/vs_select.hip finds the keff-th
by radix digits of the key: (shift, bits) = (53, 11), (42, 11), (32, 10) over
the image, then (21, 11), (10, 11), (0, 10) over the row word. An image is
written here as (d0, d1, d2) = its bits 31..21, 20..10, 9..0.

Every builder returns a Case and asserts, in numpy, the property it exists
for, so an edit that loses the edge fails test_rsel_patterns.py.
"""
from collections import namedtuple

import numpy as np

U64 = np.uint64
DIGITS = ((53, 11), (42, 11), (32, 10), (21, 11), (10, 11), (0, 10))
BINS = 2048           # first-digit buckets (checked against the library's kRselBins on the device)
PICK_THREADS = 256    # one pick thread owns BINS / PICK_THREADS = 8 consecutive buckets
SORT_CAP = 4096       # keys of the boundary bucket the fused selection's last stage holds in LDS

# name, sc (uint32 [n]), row_base, the keffs to select (each 1 <= keff <= unmasked rows)
Case = namedtuple("Case", "name sc row_base keffs")


# ---- reference -----------------------------------------------------------------
def image(d0, d1, d2):
    d0, d1, d2 = (np.asarray(x, np.uint32) for x in (d0, d1, d2))
    assert np.all(d0 < 2048) and np.all(d1 < 2048) and np.all(d2 < 1024)
    return ((d0 << np.uint32(21)) | (d1 << np.uint32(10)) | d2).astype(np.uint32)


def keys_of(sc, row_base):
    """Every unmasked row's 64-bit key, in row order."""
    sc = np.asarray(sc, np.uint32)
    rows = (np.arange(sc.size, dtype=U64) + U64(row_base))
    assert sc.size == 0 or int(rows[-1]) <= 0xFFFFFFFF, "row numbers are 32-bit"
    keys = (sc.astype(U64) << U64(32)) | (U64(0xFFFFFFFF) - rows)
    return keys[sc != 0]


def select(sc, row_base, keff):
    """The keff largest keys, descending."""
    keys = keys_of(sc, row_base)
    assert 1 <= keff <= keys.size
    return np.sort(keys)[::-1][:keff]


def first_hist(sc):
    """What the score pass leaves in `hist`: counts of the unmasked images' top 11 bits."""
    sc = np.asarray(sc, np.uint32)
    return np.bincount(sc[sc != 0] >> np.uint32(21), minlength=BINS).astype(np.uint32)


def digit(key, p):
    shift, bits = DIGITS[p]
    return int((int(key) >> shift) & ((1 << bits) - 1))


def deciding_digit(sc, row_base, keff):
    """-> (p, thr): the first digit p at which the bucket holding the keff-th
    key is taken whole (it holds exactly the keys still needed; the last digit
    always is), and thr = that key cut to digits 0..p. Exactly keff keys are
    >= thr. This is where the digit chain stops and what it leaves in
    RselState.thr."""
    keys = keys_of(sc, row_base)
    kth = int(np.sort(keys)[::-1][keff - 1])
    for p, (shift, _) in enumerate(DIGITS):
        pre = keys >> U64(shift)
        inb = int(np.count_nonzero(pre == U64(kth >> shift)))
        above = int(np.count_nonzero(pre > U64(kth >> shift)))
        if above + inb == keff or shift == 0:
            thr = (kth >> shift) << shift
            assert int(np.count_nonzero(keys >= U64(thr))) == keff
            return p, thr
    raise AssertionError("unreachable")


def boundary(sc, row_base, keff):
    """-> (b0, b1, h1, need): the (first, second) digit bucket holding the
    keff-th key, its size, and how many of its keys the answer takes -- the
    fused selection's last stage copies the bucket when need == h1, else
    selects inside it (in LDS up to SORT_CAP keys, in global memory past it)."""
    keys = keys_of(sc, row_base)
    kth = int(np.sort(keys)[::-1][keff - 1])
    pre = keys >> U64(42)
    h1 = int(np.count_nonzero(pre == U64(kth >> 42)))
    above = int(np.count_nonzero(pre > U64(kth >> 42)))
    return digit(kth, 0), digit(kth, 1), h1, keff - above


def score_ord(s):
    """vs::score_ord of fp32 scores, -0.0 ranked as +0.0 (vs::make_key)."""
    s = np.array(s, np.float32)
    s[s == 0] = 0.0
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _keffs(n, *ks):
    return sorted({int(k) for k in ks if 1 <= k <= n})


def _nonzero_u32(rng, n):
    return rng.integers(1, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


# ---- sizes -------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 255, 1023, 1025, 4099)


def sizes(n):
    """Uniform random non-zero images at n rows: the 16-byte load's tail
    (n % 4), n under one workgroup, and keff at both ends."""
    sc = _nonzero_u32(np.random.default_rng(n), n)
    assert np.all(sc != 0)
    return Case(f"sizes/{n}", sc, 3, _keffs(n, 1, 2, n // 2, n - 1, n))


def second_round_rows(cus):
    """Rows just past one full round of the widest grid (4 workgroups a CU,
    1024 rows each): the grid-stride loops run a second, partial round of more
    than one workgroup with a ragged tail."""
    return 4 * cus * 1024 + 1029 + 2


def second_round(cus):
    n = second_round_rows(cus)
    assert n > 4 * cus * 1024 + 1029 and n % 4 and (n - 4 * cus * 1024) > 1024
    sc = _nonzero_u32(np.random.default_rng(cus), n)
    sc[::7] = 0
    return Case(f"second_round/{n}", sc, 11, [4321, n // 2])


# ---- full-range images ----------------------------------------------------------
def full_range(masked):
    """Uniform random u32: bucket 0 (0 < o < 2^21) and bucket 2047 hold keys,
    and keff reaches both. masked: half the rows are 0, and keff = the
    unmasked count takes everything."""
    n = 6000
    rng = np.random.default_rng(17 + masked)
    sc = _nonzero_u32(rng, n)
    sc[[10, 11, 12, 13]] = np.array([1, (1 << 21) - 1, 2047 << 21, 0xFFFFFFFF], np.uint32)
    if masked:
        m = rng.random(n) < 0.5
        m[[10, 11, 12, 13]] = False
        sc[m] = 0
    live = int(np.count_nonzero(sc))
    h = first_hist(sc)
    assert h[0] >= 2 and h[2047] >= 2 and int(h.sum()) == live
    assert (live < n) == bool(masked)
    top = int(h[2047])
    keffs = _keffs(live, 1, top, top + 1, live // 2, live - int(h[0]), live - 1, live)
    assert digit(select(sc, 0, live)[-1], 0) == 0 and digit(select(sc, 0, 1)[0], 0) == 2047
    return Case(f"full_range/{'masked' if masked else 'dense'}", sc, 0, keffs)


# ---- pick position ------------------------------------------------------------------
PICK_T = (0, 1, 128, 255)


def pick_position(t, j, level):
    """The keff-th key's digit `level` (0, 1: 2048 buckets; 2: the image's last
    10 bits) lands on bucket g = 8 t + j, the j-th of the 8 buckets pick thread
    t owns, with populated buckets on both sides inside the same thread's 8 and
    in other threads'. keff walks over g's three keys and its two neighbours.
    At level 2 the buckets are g // 2 (1024 of them: 4 a thread in the digit
    chain); the fused selection's last stage reads that digit together with the
    row word's top bit as 2 (g // 2) + bit, and row_base flips that bit with j
    so all 8 of a thread's buckets are reached there too.
    -> (Case, g, na): na keys lie above bucket g."""
    assert 0 <= t < PICK_THREADS and 0 <= j < 8 and level in (0, 1, 2)
    nb = 2048 if level < 2 else 1024
    g = 8 * t + j if level < 2 else (8 * t + j) // 2
    step = 9 if level < 2 else 5  # lands in a neighbouring thread's buckets
    above = sorted({d for d in (g + 1, g + 2, g + 3, g + step, nb - 1) if g < d < nb})
    below = sorted({d for d in (g - 1, g - 2, g - 3, g - step, 0) if 0 <= d < g})
    own = nb // PICK_THREADS  # buckets a pick thread owns
    if g + 1 < nb and (g + 1) // own == g // own:
        assert (g + 1) in above  # a populated bucket above g in the same thread's
    if g >= 1 and (g - 1) // own == g // own:
        assert (g - 1) in below
    buckets = [d for d in above for _ in range(2)]
    na = len(buckets)
    buckets += [g] * 3 + [d for d in below for _ in range(3)]
    buckets = np.array(buckets, np.uint32)
    rng = np.random.default_rng(1000 * level + g)
    m = buckets.size
    if level == 0:
        sc = image(buckets, rng.integers(1, 2048, m), rng.integers(0, 1024, m))
    elif level == 1:
        sc = image(np.full(m, 1500), buckets, rng.integers(1, 1024, m))
    else:
        sc = image(np.full(m, 700), np.full(m, 1300), buckets)
    sc = sc[rng.permutation(m)]
    assert np.all(sc != 0)
    row_base = (1 << 31) if (level == 2 and j % 2) else 5
    keffs = _keffs(m, na, na + 1, na + 2, na + 3, na + 4)
    ref = select(sc, row_base, m)
    for keff in (na + 1, na + 2, na + 3):
        assert digit(ref[keff - 1], level) == g
        for p in range(level):
            assert digit(ref[keff - 1], p) == digit(ref[0], p)  # the digits above are shared
    if na:
        assert digit(ref[na - 1], level) > g
    if na + 4 <= m:
        assert digit(ref[na + 3], level) < g
    # g taken whole (with nothing below g that is every key: decided at once)
    assert deciding_digit(sc, row_base, na + 3)[0] == (level if below else 0)
    assert deciding_digit(sc, row_base, na + 2)[0] > level   # decided below it
    if level == 2:  # the fused last stage's first digit: key bits 41..31
        f = (int(ref[na]) >> 31) & 2047
        assert f == 2 * g + (0 if j % 2 else 1)
    return Case(f"pick/{level}/{t}/{j}", sc, row_base, keffs), g, na


# ---- bucket taken whole ---------------------------------------------------------------
def whole_bucket(level, big=False):
    """above + h[b] == keff at digit `level`: the chain stops there. For the
    fused selection levels 0 and 1 are the copy branch of its last stage (need
    == h1), level 2 an early end of its radix passes (need < h1). big: the
    copied bucket holds more keys than the workgroup has threads."""
    rng = np.random.default_rng(40 + level + 10 * big)
    reps = 900 if big else 1

    def grp(d0, d1, d2, cnt):  # cnt keys with these digits (None: random)
        if (d0, d1, d2) == whole:
            cnt *= reps
        d0, d1, d2 = (rng.integers(1, hi, cnt) if d is None else np.full(cnt, d)
                      for d, hi in ((d0, 2048), (d1, 2048), (d2, 1024)))
        return image(d0, d1, d2)

    if level == 0:
        whole = (1000, None, None)
        parts = [grp(1800, None, None, 5), grp(*whole, 7), grp(10, None, None, 4)]
        keff = 5 + 7 * reps
    elif level == 1:
        whole = (1200, 400, None)
        parts = [grp(1900, None, None, 2), grp(1200, 900, None, 5), grp(*whole, 7),
                 grp(1200, 3, None, 4), grp(100, None, None, 3)]
        keff = 2 + 5 + 7 * reps
    else:
        whole = (1200, 400, 600)
        parts = [grp(1900, None, None, 2), grp(1200, 900, None, 5), grp(1200, 400, 1000, 6),
                 grp(*whole, 7), grp(1200, 400, 2, 4), grp(100, None, None, 3)]
        keff = 2 + 5 + 6 + 7 * reps
    sc = np.concatenate(parts)
    sc = sc[rng.permutation(sc.size)]
    assert deciding_digit(sc, 9, keff)[0] == level
    b0, b1, h1, need = boundary(sc, 9, keff)
    if level < 2:
        # (level 0: the copied bucket is the lowest populated second digit of b0)
        assert need == h1 and (level == 0 or h1 == 7 * reps)
    else:
        assert need < h1
    assert not big or h1 > PICK_THREADS
    # keff - 1 and keff + 1 are decided deeper
    return Case(f"whole/{level}{'/big' if big else ''}", sc, 9, _keffs(sc.size, keff, keff - 1, keff + 1))


# ---- boundary bucket size ---------------------------------------------------------------
H1S = (2, 4095, 4096, 4097, 9000)


def boundary_size(h1):
    """h1 keys share (b0, b1) and the keff-th key lies among them with need in
    {1, h1 / 2, h1 - 1} (never the copy branch): the last stage's keys in LDS up
    to SORT_CAP and in global memory past it. Five keys above the bucket make
    the stage write at an offset into sel."""
    rng = np.random.default_rng(h1)
    sc = np.concatenate([image(np.full(3, 1999), rng.integers(0, 2048, 3), rng.integers(0, 1024, 3)),
                         image(np.full(2, 1234), np.full(2, 1700), rng.integers(0, 1024, 2)),
                         image(np.full(h1, 1234), np.full(h1, 77), rng.integers(0, 1024, h1))])
    sc = sc[rng.permutation(sc.size)]
    keffs = _keffs(sc.size, *(5 + need for need in (1, h1 // 2, h1 - 1)))
    for keff in keffs:
        b0, b1, got, need = boundary(sc, 0, keff)
        assert (b0, b1, got) == (1234, 77, h1) and need == keff - 5 and 1 <= need < h1
    assert (h1 <= SORT_CAP) == (h1 in (2, 4095, 4096))
    return Case(f"boundary/{h1}", sc, 0, keffs)


# ---- ties ------------------------------------------------------------------------------------
def all_equal(n, row_base):
    """One image everywhere: the selection is decided in the row word alone
    (lower rows first). row_base = 2^32 - n makes the last row's word 0."""
    rb = (1 << 32) - n if row_base == "top" else row_base
    sc = np.full(n, 0xB7654321, np.uint32)
    keffs = _keffs(n, 1, 2, n // 2, n - 1, n)
    for keff in keffs:
        ref = select(sc, rb, keff)
        assert np.array_equal(ref & U64(0xFFFFFFFF), U64(0xFFFFFFFF) - U64(rb) - np.arange(keff, dtype=U64))
        if keff < n:
            assert deciding_digit(sc, rb, keff)[0] >= 3
    if row_base == "top":
        assert int(select(sc, rb, n)[-1]) & 0xFFFFFFFF == 0
    return Case(f"equal/{n}/{row_base}", sc, rb, keffs)


def runs():
    """Five images repeated in runs of known length: keff falls on the first
    and on the last row of a run (the run taken from its first key, and whole)."""
    vals = np.sort(_nonzero_u32(np.random.default_rng(5), 5))[::-1]
    counts = [300, 500, 200, 400, 100]
    sc = np.repeat(vals, counts)
    sc = sc[np.random.default_rng(6).permutation(sc.size)]
    cum = np.cumsum(counts)
    keffs = []
    ref = select(sc, 77, sc.size)
    for i in (1, 2, 3):
        first, last = int(cum[i - 1]) + 1, int(cum[i])
        keffs += [first, last]
        run = keys_of(sc, 77)
        run = run[(run >> U64(32)) == U64(vals[i])]
        assert int(ref[first - 1]) == int(run.max()) and int(ref[last - 1]) == int(run.min())
    return Case("runs", sc, 77, keffs)


# ---- realistic -------------------------------------------------------------------------------
def realistic():
    s = (np.random.default_rng(8).standard_normal(20000) * 0.05).astype(np.float32)
    sc = score_ord(s)
    assert np.all(sc != 0) and np.count_nonzero(first_hist(sc)) < BINS // 8  # a sliver of the key space
    return Case("realistic", sc, 0, [1100, 4321, 19999])


def trailer():
    """The second, different selection every device case ends with, on the
    buffers the case left behind."""
    sc = _nonzero_u32(np.random.default_rng(99), 777)
    sc[::5] = 0
    return Case("trailer", sc, 123, [300])
