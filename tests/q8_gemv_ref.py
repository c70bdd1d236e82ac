"""The single-query int8 scan and finish restated in numpy (DESIGN.md §5
"Single query on the int8 copy"; device side csrc/vs_kernels.hip
gemv_q8_scan_kernel / gemv_q8_finish_kernel), on top of tests/q8_ref.py.
tests/test_q8_gemv_bounds.py (CPU: the restatement alone is sound) and
tests/test_q8_gemv_stages_gpu.py (the kernels against it) draw from it.

Per row, with the query's image {q8, sqS, a, c, sigma} and the row's tile
{dt, nt}: dot = q8 . x8 (an exact integer), xs = fl(dot sqS), the half-width
w = a dt + (c + sigma) nt, L = xs - w <= s <= U = xs + w for any fp32
evaluation s of the score. A scan workgroup keeps its KP largest U keys and
its largest L image; the finish takes P = the radix floor of the k-th largest
non-zero L image and rescores every list entry whose U image reaches P (a
list whose last entry does: every row of its workgroup).

Score images: the high word of a result key (include/vsearch.h), an
order-preserving uint32 image of the fp32 score, never 0 for a number.
"""
import numpy as np

import q8_ref as R

F32 = np.float32
U24 = 2.0 ** -24
WAVES = 8  # waves per scan workgroup
STEP = 4   # rows per wave step


def wg_of_row(row, nscan):
    """The scan workgroup of local row `row`: waves are interleaved over
    4-row steps."""
    return ((np.asarray(row, np.int64) // STEP) % (nscan * WAVES)) // WAVES


def image(s):
    """fp32 scores -> their order-preserving uint32 images (-0.0 as +0.0)."""
    s = np.array(s, np.float32, ndmin=1)
    s[s == 0] = 0.0
    u = s.view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def unimage(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & 0x80000000, o & 0x7FFFFFFF, ~o).astype(np.uint32).view(np.float32)


def _fma(a, b, c):
    """fl(a b + c): the product of two floats is exact in fp64; the fp64 sum's
    own rounding (2^-53) moves the float result only at an exact tie."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def width_ref(a, c, sigma, dt, nt):
    """The reference's half-width, as R.bracket forms it:
    fl(fl(fl(a dt) + fl(c nt)) + fl(sigma nt))."""
    dt, nt = dt.astype(F32), nt.astype(F32)
    m = F32(a) * dt + F32(c) * nt
    return (m + F32(sigma) * nt).astype(F32)


def width_dev(a, c, sigma, dt, nt):
    """The scan's half-width mt = pa dt + pc nt with pc = fl(c + sigma), in
    every form a compiler may give it: both products rounded, or either one
    contracted into an FMA -> list of three arrays."""
    dt, nt = dt.astype(F32), nt.astype(F32)
    pa = np.full_like(dt, F32(a))
    pc = np.full_like(nt, F32(F32(c) + F32(sigma)))
    return [(pa * dt + pc * nt).astype(F32), _fma(pa, dt, (pc * nt).astype(F32)),
            _fma(pc, nt, (pa * dt).astype(F32))]


def width_tol(w_ref):
    """|w_dev - w_ref| <= 4 2^-24 w_ref: both are sums of non-negative terms,
    each term through at most four roundings."""
    return 4.0 * U24 * w_ref.astype(np.float64)


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(np.float64)


def edge_tol(w_ref, e_ref, xs):
    """|U_dev - U_ref| (|L_dev - L_ref|) <= 4 2^-24 w + ulp(U) + ulp(xs) / 2.
    The edge is xs +- w with xs = dot sqS. The first term is the half-widths'
    distance (width_tol); ulp(U) is the final rounding of either side, half an
    ulp each; the last term is the reference's own rounding of xs, which a
    device that contracts dot sqS +- w into one FMA does not commit (and which
    is the only term that matters where xs and w cancel)."""
    return width_tol(w_ref) + ulp(e_ref) + 0.5 * ulp(xs)


def edges_dev(dot, sqS, wd):
    """(U, L) for a device half-width wd in both forms of xs +- wd: xs rounded
    first, or contracted into an FMA -> [(U, L), (U, L)]."""
    d, s = dot.astype(F32), np.full(len(dot), F32(sqS))
    xs = (d * s).astype(F32)
    return [((xs + wd).astype(F32), (xs - wd).astype(F32)),
            (_fma(d, s, wd), _fma(d, s, (-wd).astype(F32)))]


def U_floor(dot, r, dt, nt, dim):
    """The smallest U a sound scan can form for these rows: every form of the
    device's arithmetic (width_dev x edges_dev; all non-decreasing in a, c,
    sigma) on the smallest floats that still bound the query's fp64 norms --
    a, c rounded up without q8_norm_up's margin, sigma = (4 dim + 64) 2^-24 |q|
    rounded down. A par rounded down instead of up falls under it."""
    s_lo = (4.0 * dim + 64.0) * U24 * r["qn"]
    sig = F32(s_lo)
    if np.float64(sig) > s_lo:
        sig = np.nextafter(sig, F32(-np.inf))
    lo = None
    for wd in width_dev(R._up(r["an"]), R._up(r["cn"]), sig, dt, nt):
        for U, _ in edges_dev(dot, r["sqS"], wd):
            lo = U if lo is None else np.minimum(lo, U)
    return lo


def dots(X8, q8):
    """The exact integer dots of every row (|dot| < 2^24: exact in fp32, and
    every partial sum exact in the fp64 product used here)."""
    d = X8.astype(np.float64) @ q8.astype(np.float64)
    assert np.abs(d).max(initial=0) < 2 ** 24
    return d.astype(np.int64)


def brackets(X8, dt, nt, qp, S, n=None):
    """L, U, w (fp32, the reference's formation), xs, the query's image
    (R.query_ref) and the integer dots of rows [0, n) for the preprocessed
    query qp; dt / nt per 32-row tile."""
    n = len(X8) if n is None else n
    r = R.query_ref(qp, S)
    tile = np.arange(n) // 32
    d = dots(X8[:n], r["q8"])
    L, U = R.bracket(d, r["sqS"], r["a"], r["c"], r["sigma"], dt[tile], nt[tile])
    w = width_ref(r["a"], r["c"], r["sigma"], dt[tile], nt[tile])
    xs = (d.astype(F32) * r["sqS"]).astype(F32)
    return L, U, w, xs, r, d


def lbest_ref(L, nscan, allow=None):
    """Every scan workgroup's largest L image over its allowed rows (0: none)."""
    n = len(L)
    ok = np.ones(n, bool) if allow is None else np.asarray(allow[:n], bool)
    out = np.zeros(nscan, np.uint32)
    np.maximum.at(out, wg_of_row(np.arange(n), nscan)[ok], image(L)[ok])
    return out


def radix_floor_P(lbest, k):
    """The finish's P: the top-16-bit prefix (low 16 bits zero) of the k-th
    largest non-zero workgroup L image; 0 when fewer than k are non-zero."""
    v = np.sort(np.asarray(lbest, np.uint32)[np.asarray(lbest) != 0])[::-1]
    if len(v) < k:
        return 0
    return int(v[k - 1]) & 0xFFFF0000


def finish_counts(ulist, P, allow, n, nscan, row_base=0):
    """(rows rescored, lists replaced by their workgroup's rows) the finish
    must report for the scan's lists `ulist` [nscan, KP] (uint64 keys): a list
    whose last entry is a key with U image >= P falls back and rescores every
    allowed row of its workgroup; any other rescores its entries with U image
    >= P."""
    ulist = np.asarray(ulist, np.uint64)
    img = (ulist >> np.uint64(32)).astype(np.uint32)
    hit = (ulist != 0) & (img >= np.uint32(P))
    fb = hit[:, -1]
    ok = np.ones(n, bool) if allow is None else np.asarray(allow[:n], bool)
    per_wg = np.bincount(wg_of_row(np.arange(n), nscan)[ok], minlength=nscan)
    rescored = int(hit[~fb].sum()) + int(per_wg[fb].sum())
    return rescored, int(fb.sum())
