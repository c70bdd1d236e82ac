"""(GPU) The single-query int8 path stage by stage (DESIGN.md §5 "Single query
on the int8 copy"; vs_kernels.hip gemv_q8_scan_kernel / gemv_q8_finish_kernel):
launch_gemv_q8 itself through tests/kprobe, one launch at a time, on the
adversarial rows and queries of tests/q8_ref.py, against the numpy
restatement of tests/q8_gemv_ref.py and against the plain GEMV's own keys
(launch_gemv_one + launch_merge on the same device buffers).

  scan     every row's U key in the list of its workgroup, every L image
           (one allowed row a workgroup), truncated lists, the workgroups' L
  finish   alone on the device's scan outputs: P restated from lbest, the
           rescored-row and fallback-list counts, the compacted keys, the keys
           bit for bit the GEMV's
  forced   fallback beside plain lists, every list falling back, P == 0, the
           three final sorts, filters, row_base up to the engine's limit,
           negative scores, clipped and zero rows

Tolerance (derived in tests/test_q8_gemv_bounds.py, q8_gemv_ref.edge_tol): a
device edge lies within 4 2^-24 w + ulp(edge) + ulp(xs) / 2 of the
reference's. The reference uses the device's own int8 rows and tile norms
(their own tests: test_q8_stages_gpu.py) and query_ref of the oracle's
preprocessed query; the scan's query image and par show only through U and L.
Row counts: the grid comes from the shim (it depends on the CU count); below
24k rows a scan workgroup holds 32 rows, below 49k at most 64.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import q8_gemv_ref as G
import q8_gemv_stage as Gs
import q8_ref as R
import q8_stage as St

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-5
N_SMALL = 2003   # 63 workgroups of <= 32 rows on 256 CUs; n % 4 = 3, n % 32 = 19
N_MID = 6003     # > 128 workgroups: P > 0 at every k <= 128
N_TWO = 30011    # two steps a wave, <= 64 rows a workgroup
N_BIG = 50003    # > 64 rows in every workgroup: truncated lists at KP = 64


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


_CASES = {}


def _case(kp, torch, kind, n, dim, f32, row_base=0, rows=None):
    """A collection of make_rows(kind) (or of rows(X) applied to the unit rows)
    on the device with its int8 copy, and what every reference needs of it;
    the last few are kept."""
    key = (kind, n, dim, f32, row_base)
    if key not in _CASES:
        while len(_CASES) >= 2:
            _CASES.pop(next(iter(_CASES)))
        if rows is None:
            X, X0 = R.make_rows(kind, n, dim, f32)
        else:
            X = rows(R.make_rows("unit", n, dim, f32)[0].copy())
            X0 = X
        coll = St.Collection(kp, torch, X, f32, X0=X0 if kind == "clipped" else None, row_base=row_base,
                             poison_pad=True)
        x8, meta, glob = coll.read()
        assert not x8[n:].any(), "dead rows of the last tile are zero bytes"
        _CASES[key] = SimpleNamespace(coll=coll, X=X, n=n, dim=dim, f32=f32, row_base=row_base, x8=x8[:n],
                                      dt=meta[:, 0].copy(), nt=meta[:, 1].copy(), S=glob[3],
                                      nscan=kp.gemv_q8_lists(n))
        c = _CASES[key]
        c.wg = G.wg_of_row(np.arange(n), c.nscan)
        c.per_wg = np.bincount(c.wg, minlength=c.nscan)
    return _CASES[key]


def _qref(c, orc, q, cosine):
    """The reference of one raw query: brackets, tolerances, scores."""
    qp = orc.preprocess(q[None], cosine, not c.f32)[0]
    L, U, w, xs, r, d = G.brackets(c.x8, c.dt, c.nt, qp, c.S, c.n)
    tile = np.arange(c.n) // 32
    return SimpleNamespace(qp=qp, L=L, U=U, w=w, xs=xs, r=r, d=d, tolU=G.edge_tol(w, U, xs),
                           tolL=G.edge_tol(w, L, xs), floor=G.U_floor(d, r, c.dt[tile], c.nt[tile], c.dim),
                           s64=c.X.astype(np.float64) @ qp.astype(np.float64))


def _lists(c, ulist):
    """Structure of the scan's lists -> (local rows, U, workgroup) of every
    key: sorted descending, distinct, 0-padded, rows live."""
    nz = ulist != 0
    for l in range(ulist.shape[0]):
        m = int(nz[l].sum())
        assert nz[l, :m].all() and not nz[l, m:].any(), ("zeros inside list", l)
        assert np.all(ulist[l, 1:m] < ulist[l, :max(m - 1, 0)]), ("list not sorted / not distinct", l)
    rows = St.key_rows(ulist[nz]) - c.row_base
    assert rows.min(initial=0) >= 0 and rows.max(initial=0) < c.n, "a dead row (or one under row_base) in a list"
    return rows, St.key_scores(ulist[nz]), np.nonzero(nz)[0]


def _queries(c, kinds=R.QUERY_KINDS):
    return R.make_queries(c.X, c.f32, 0, kinds)


# ---------------------------------------------------------------------------
# a. scan, every row observable
# ---------------------------------------------------------------------------
def _p(kind, dim, f32, cosine, k, n=N_SMALL):
    return pytest.param(kind, dim, f32, cosine, k, n,
                        id=f"{kind}-{'f32' if f32 else 'bf16'}-{dim}-{'cos' if cosine else 'dot'}-k{k}-n{n}")


SCAN_ALL = [_p(kd, 768, False, i % 2 == 0, (1, 65)[i % 2]) for i, kd in enumerate(R.row_kinds(False))] + [
    _p("unit", 1024, False, True, 65), _p("clipped", 1024, False, False, 1),
    _p("unit", 768, True, False, 65), _p("norm30", 768, True, True, 1), _p("clipped", 768, True, True, 65),
    _p("unit", 1024, True, True, 1), _p("norm30", 1024, True, False, 65),
    _p("unit", 768, False, False, 10, N_TWO)]


@pytest.mark.parametrize("kind,dim,f32,cosine,k,n", SCAN_ALL)
def test_scan_every_row_observable(kp, torch_, orc, kind, dim, f32, cosine, k, n):
    """No workgroup holds more than KP rows, so ulist holds every row's U key:
    each live row once, in the list of wg_of_row(row), row_base added; every U
    within the derived bound of the reference's, no lower than the smallest U
    a sound par can give (U_floor), and an upper bound of the fp64 score, of
    fp32 sums in three orders and of the GEMV's own score.
    Mutations: sigma dropped from pc (U_ref bound); rintf -> truncf in
    q8_query_wave (U_ref bound); q8_norm_up rounding down (U_floor);
    meta[r0 >> 5] read from the next tile (U_ref bound)."""
    row_base = 4096 if n == N_SMALL else 0
    c = _case(kp, torch_, kind, n, dim, f32, row_base)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    assert run.KP == (64 if k <= 64 else 128) and run.nscan == c.nscan >= 2
    assert n % 4 and n % 32 and c.per_wg.max() <= run.KP
    Q, kinds = _queries(c, R.QUERY_KINDS if n == N_SMALL else ("unit", "neg_row", "copy_row"))
    for q, qk in zip(Q, kinds):
        what = (kind, qk)
        ref = _qref(c, orc, q, cosine)
        qd = Gs.query_dev(torch_, q)
        run.launch(1, qd, cosine)
        run.check_guards()
        ulist, lbest = run.scan_out()
        rows, Ud, wg = _lists(c, ulist)
        assert np.array_equal(np.sort(rows), np.arange(n)), (what, "every live row exactly once")
        assert np.array_equal(wg, c.wg[rows]), (what, "a row in another workgroup's list")
        err = np.abs(Ud.astype(np.float64) - ref.U[rows].astype(np.float64))
        print(what, "max |U_dev - U_ref| / tol", float((err / np.maximum(ref.tolU[rows], 1e-300)).max(initial=0)))
        assert np.all(err <= ref.tolU[rows]), (what, "U off the reference", int(rows[np.argmax(err - ref.tolU[rows])]))
        assert np.all(Ud >= ref.floor[rows]), (what, "U under the smallest sound U")
        assert np.all(Ud.astype(np.float64) >= ref.s64[rows]), (what, "U under the fp64 score")
        for s in R._fp32_sums(c.X, ref.qp):
            assert np.all(Ud >= s[rows]), (what, "U under an fp32 score")
        gk = Gs.gemv_keys(kp, torch_, c.coll, qd, cosine, 128)
        grow = St.key_rows(gk[gk != 0]) - row_base
        Uof = np.empty(n, np.float32)
        Uof[rows] = Ud
        assert len(grow) == 128 and np.all(Uof[grow] >= St.key_scores(gk)), (what, "U under the GEMV's score")
        # the workgroups' L images: the largest device L lies within the bound of some row's
        lo = np.full(c.nscan, -np.inf)
        hi = np.full(c.nscan, -np.inf)
        np.maximum.at(lo, c.wg, ref.L.astype(np.float64) - ref.tolL)
        np.maximum.at(hi, c.wg, ref.L.astype(np.float64) + ref.tolL)
        lb = G.unimage(lbest).astype(np.float64)
        assert np.all(lbest != 0) and np.all(lo <= lb) and np.all(lb <= hi), (what, "lbest")


# ---------------------------------------------------------------------------
# b. scan, every L observable
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,f32,cosine,k,n", [
    _p("unit", 768, False, False, 10), _p("clipped", 768, True, True, 65), _p("zero_rows", 1024, False, True, 1),
    _p("norm30", 1024, True, False, 128)])
def test_scan_every_L_observable(kp, torch_, orc, kind, dim, f32, cosine, k, n):
    """Allow masks that leave one row in each scan workgroup (different rows,
    steps and waves from mask to mask; one mask also empties every third
    workgroup): lbest[wg] is then that row's L image -- within the derived
    bound of the reference's L, at most the fp64 score and every fp32 sum --
    and 0 for an emptied workgroup; neg_row and zero queries included.
    Mutations: xs - mt -> xs (L_ref bound)."""
    c = _case(kp, torch_, kind, n, dim, f32, 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    Q, kinds = _queries(c)
    by_wg = [np.nonzero(c.wg == w)[0] for w in range(c.nscan)]
    for m in range(3):
        pick = np.array([r[(5 * w + 11 * m) % len(r)] for w, r in enumerate(by_wg)])
        keep = np.ones(c.nscan, bool) if m < 2 else (np.arange(c.nscan) % 3 != 1)
        keep[-1] = m != 2
        mask = np.zeros(n, bool)
        mask[pick[keep]] = True
        adev, aptr = Gs.allow_dev(torch_, mask, n)
        for q, qk in zip(Q, kinds):
            what = (kind, qk, m)
            ref = _qref(c, orc, q, cosine)
            run.launch(1, Gs.query_dev(torch_, q), cosine, aptr)
            run.check_guards()
            ulist, lbest = run.scan_out()
            rows, Ud, wg = _lists(c, ulist)
            assert np.array_equal(rows, pick[keep]) and np.array_equal(wg, np.nonzero(keep)[0]), what
            assert not lbest[~keep].any() and np.all(lbest[keep] != 0), (what, "emptied workgroups report 0")
            Ld = G.unimage(lbest[keep])
            err = np.abs(Ld.astype(np.float64) - ref.L[rows].astype(np.float64))
            assert np.all(err <= ref.tolL[rows]), (what, "L off the reference", float(err.max()))
            assert np.all(Ld.astype(np.float64) <= ref.s64[rows]), (what, "L over the fp64 score")
            for s in R._fp32_sums(c.X[rows], ref.qp):
                assert np.all(Ld <= s), (what, "L over an fp32 score")
            assert np.all(Ld <= Ud), what
            if qk == "zero":
                assert not Ld.any() and not Ud.any(), what
            if qk == "neg_row":
                assert (Ld < 0).any(), what


# ---------------------------------------------------------------------------
# c. scan, truncated lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim,f32,cosine", [pytest.param(768, False, False, id="bf16-768-dot"),
                                            pytest.param(768, True, True, id="f32-768-cos")])
def test_scan_truncated_lists(kp, torch_, orc, dim, f32, cosine):
    """Every workgroup holds more than KP = 64 rows: each list is the KP
    largest reference U keys of its workgroup, row for row. Two rows may trade
    places only where their reference U values lie within the sum of their
    two bounds (either device U may sit anywhere in its bound); such places
    stay under 1% of the entries. lbest[wg] is the largest L image over the
    workgroup's allowed rows. The second query runs under a 70% filter.
    Mutations: the scan's five (sigma dropped, truncf, q8_norm_up down, the
    wrong tile's meta, L = xs) move U or lbest here as in the two tests
    above, which fail first; none was run against this test alone."""
    n, k = N_BIG, 10
    c = _case(kp, torch_, "unit", n, dim, f32)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    KP = run.KP
    assert KP == 64 and c.per_wg.min() > KP
    Q, kinds = _queries(c, ("unit", "copy_row"))
    rng = np.random.default_rng(4)
    for q, qk in zip(Q, kinds):
        mask = None if qk == "unit" else rng.random(n) < 0.7
        adev, aptr = Gs.allow_dev(torch_, mask, n)
        ref = _qref(c, orc, q, cosine)
        run.launch(1, Gs.query_dev(torch_, q), cosine, aptr)
        run.check_guards()
        ulist, lbest = run.scan_out()
        rows, Ud, wg = _lists(c, ulist)
        assert np.all(np.abs(Ud.astype(np.float64) - ref.U[rows]) <= ref.tolU[rows]), (qk, "U off the reference")
        ok = np.ones(n, bool) if mask is None else mask
        keys = St.make_keys(ref.U, np.arange(n) + c.row_base)
        swapped = total = 0
        for l in range(c.nscan):
            mine = np.nonzero((c.wg == l) & ok)[0]
            want = mine[np.argsort(keys[mine])[::-1][:KP]]
            got = rows[wg == l]
            assert len(got) == len(want), (qk, l, "list length")
            d = np.nonzero(got != want)[0]
            assert ok[got].all(), (qk, l, "a masked row in a list")
            gap = np.abs(ref.U[got[d]].astype(np.float64) - ref.U[want[d]])
            assert np.all(gap <= ref.tolU[got[d]] + ref.tolU[want[d]]), (qk, l, "not the KP largest U keys")
            swapped += len(d)
            total += len(want)
        print(qk, "positions traded inside the bound:", swapped, "of", total)
        assert swapped <= total // 100, (qk, swapped, total)
        lo = np.full(c.nscan, -np.inf)
        hi = np.full(c.nscan, -np.inf)
        np.maximum.at(lo, c.wg[ok], (ref.L.astype(np.float64) - ref.tolL)[ok])
        np.maximum.at(hi, c.wg[ok], (ref.L.astype(np.float64) + ref.tolL)[ok])
        lb = G.unimage(lbest).astype(np.float64)
        assert np.all(lbest != 0) and np.all(lo <= lb) and np.all(lb <= hi), (qk, "lbest")


# ---------------------------------------------------------------------------
# d. finish in isolation
# ---------------------------------------------------------------------------
def _search(kp, torch, c, run, q, cosine, mask=None, what=None):
    """Scan, read its outputs back, zero cand, finish with stats; every check
    that holds for any input -> what the caller needs for its own."""
    k, n = run.k, c.n
    adev, aptr = Gs.allow_dev(torch, mask, n)
    qd = Gs.query_dev(torch, q)
    run.stats[:2] = 0
    run.launch(1, qd, cosine, aptr)
    ulist, lbest = run.scan_out()
    run.zero_cand()
    run.launch(2, qd, cosine, aptr)
    run.check_guards()
    dst, cand, st = run.keys(), run.cand(), run.counts()
    P = G.radix_floor_P(lbest, k)
    gk = Gs.gemv_keys(kp, torch, c.coll, qd, cosine, k, aptr)
    nz = cand[cand != 0]
    print(what, "P", hex(P), "N", len(nz), "stats", st)
    assert np.array_equal(dst, gk), (what, "keys differ from the GEMV's", dst[:4], gk[:4])
    assert np.all((nz >> np.uint64(32)) >= P), (what, "a key under P was kept")
    assert np.all(np.isin(dst[dst != 0], nz)), (what, "a result key is not among the compacted keys")
    assert st == G.finish_counts(ulist, P, mask, n, c.nscan), (what, "rescored rows / fallback lists", st)
    allowed = n if mask is None else int(mask.sum())
    assert np.count_nonzero(dst) == min(k, allowed) and not dst[min(k, allowed):].any(), what
    if allowed >= k:
        assert P <= int(dst[k - 1] >> np.uint64(32)), (what, "P over the k-th score")
    else:
        assert P == 0, what
    # both launches in one call: the same keys, the counters back at zero
    run.launch(3, qd, cosine, aptr)
    run.check_guards()
    assert np.array_equal(run.keys(), gk), (what, "part = 3")
    return SimpleNamespace(dst=dst, P=P, N=len(nz), stats=st, ulist=ulist, lbest=lbest, allowed=allowed)


FINISH = [_p("unit", 768, False, True, 1, N_MID), _p("unit", 768, False, False, 10, N_MID),
          _p("unit", 1024, False, True, 64, N_MID), _p("clipped", 1024, False, False, 65, N_MID),
          _p("unit", 768, True, True, 128, N_MID), _p("norm30", 768, True, False, 10, N_MID),
          _p("unit", 1024, True, True, 65, N_MID), _p("norm30", 1024, True, False, 64, N_MID),
          _p("clipped", 768, False, True, 128, N_MID)]
ORACLE_Q = ("unit", "norm30", "copy_row", "neg_row")  # unit-scale scores: the oracle's 1e-6 absolute floor fits


@pytest.mark.parametrize("kind,dim,f32,cosine,k,n", FINISH)
def test_finish_in_isolation(kp, torch_, orc, kind, dim, f32, cosine, k, n):
    """part = 1, read ulist / lbest back, zero cand, part = 2 with stats. P =
    radix_floor_P of the device's own lbest: dst equals the GEMV's keys bit
    for bit (and passes the oracle's check_topk at 1e-5), every key left in
    cand reaches P and every key of dst is in cand, stats equal the counts the
    restatement derives from ulist, P and n, and P is at most the image of the
    k-th key. The zero query puts every U image exactly at P.
    Mutations: kk = k - 1 in the radix select (k = 1: P above everything, no
    key; else the stats); the fallback condition never true (stats[1] in the
    forced-branch tests); >= P -> > P at the survivor test (zero query: no
    key survives); the finish's workgroup-of-row map with 4 waves (stats[0]
    and keys in test_fallback_beside_plain_lists)."""
    c = _case(kp, torch_, kind, n, dim, f32, 3 * 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    assert c.nscan > 128
    Q, kinds = _queries(c)
    for q, qk in zip(Q, kinds):
        r = _search(kp, torch_, c, run, q, cosine, None, (kind, qk, k))
        assert r.P != 0, (kind, qk)
        if qk == "zero":
            assert r.P == 0x80000000 and np.all(r.ulist[r.ulist != 0] >> np.uint64(32) == r.P)
        if qk in ORACLE_Q and kind in ("unit", "norm30"):
            qp = orc.preprocess(q[None], cosine, not f32)
            s32, s64, rows, cnt = orc.search(c.X, qp, k, c.row_base)
            drows = St.key_rows(r.dst)[None].astype(np.uint64)
            dcnt = np.array([k], np.uint32)
            bad = orc.check_topk(St.key_scores(r.dst)[None], drows, dcnt, s64, rows, cnt,
                                 orc.rescore(c.X, qp, drows, dcnt, c.row_base), SCORE_RTOL)
            assert not bad, (kind, qk, bad[:4])


# ---------------------------------------------------------------------------
# e. forced branches
# ---------------------------------------------------------------------------
def test_fallback_beside_plain_lists(kp, torch_):
    """More than KP rows of three scan workgroups (the first, one inside a
    finishing workgroup, the last) are copies of one vector the query matches:
    their lists are full of keys that reach P and fall back, the others do
    not; the tied keys come back as the lowest rows (fp32 768-d rows: one row
    a wave step in the GEMV, so equal rows score equal bits).
    Mutations: the fallback condition never true (stats[1]); the finish's
    workgroup-of-row map with the wrong wave count (stats[0], keys)."""
    n, dim, k = N_BIG, 768, 10
    nscan = kp.gemv_q8_lists(n)
    wg = G.wg_of_row(np.arange(n), nscan)
    copies = np.nonzero(np.isin(wg, [0, 11, nscan - 1]))[0]

    def rows(X):
        X[copies] = X[5]
        return X
    c = _case(kp, torch_, "copies3", n, dim, True, 0, rows)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    assert c.per_wg.min() > run.KP
    r = _search(kp, torch_, c, run, 2 * c.X[5], False, None, "copies in 3 workgroups")
    nonempty = int((r.ulist[:, 0] != 0).sum())
    assert 0 < r.stats[1] < nonempty and r.stats[1] >= 3, (r.stats, nonempty)
    assert np.array_equal(St.key_rows(r.dst), copies[:k]), "ties: the lowest rows first"
    # under a filter that leaves fewer than KP copies in the middle workgroup: it no longer falls back
    mask = np.ones(n, bool)
    mask[copies[wg[copies] == 11][20:]] = False
    r2 = _search(kp, torch_, c, run, 2 * c.X[5], False, mask, "copies, filtered")
    assert 0 < r2.stats[1] < r.stats[1]


@pytest.mark.parametrize("n,k,dim,f32", [pytest.param(40011, 10, 768, True, id="n40011-k10-f32-768"),
                                         pytest.param(5003, 10, 1024, False, id="n5003-k10-bf16-1024"),
                                         pytest.param(5003, 128, 1024, False, id="n5003-k128-bf16-1024"),
                                         pytest.param(5003, 65, 768, True, id="n5003-k65-f32-768")])
def test_all_rows_equal(kp, torch_, n, k, dim, f32):
    """Every row equal: every U reaches P, so every row is rescored
    (stats[0] = n), and exactly the full lists -- workgroups of at least KP
    rows -- fall back (40011 rows: 64-row workgroups at KP = 64; 5003 rows:
    none). The keys are the k lowest rows. The compacted array holds every
    wave's k best: 64 < N <= 4096 at 5003 rows and k = 10 (the LDS sort), more
    than 4096 at k = 128 and at 40011 rows (merge_query).
    Mutations: the fallback condition never true (stats[1] at 40011 rows)."""
    def rows(X):
        X[:] = X[3]
        return X
    c = _case(kp, torch_, "equal", n, dim, f32, 4096, rows)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    r = _search(kp, torch_, c, run, c.X[3], True, None, ("equal rows", n, k))
    assert r.stats == (n, int((c.per_wg >= run.KP).sum())), r.stats
    assert (r.stats[1] > 0) == (n == 40011)
    assert np.array_equal(St.key_rows(r.dst), np.arange(k) + c.row_base)
    if n == 5003 and k == 10:
        assert 64 < r.N <= 4096, r.N
    if k == 128 or n == 40011:
        assert r.N > 4096, r.N


def test_P_zero_fewer_workgroups_than_k(kp, torch_):
    """k = 128 over fewer than 128 scan workgroups: P = 0, no list is full, so
    every row is rescored and kept (N = n: the LDS sort). Fewer than 128
    workgroups means fewer than 4096 rows (32 a workgroup), so this case
    cannot reach merge_query; test_all_rows_equal does.
    Mutations: P forced non-zero when the radix select finds fewer than k
    values (some = true) would drop rows here; not run."""
    c = _case(kp, torch_, "unit", N_SMALL, 768, False, 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, 128)
    assert 33 <= c.nscan < 128
    Q, kinds = _queries(c, ("unit", "neg_row"))
    for q, qk in zip(Q, kinds):
        r = _search(kp, torch_, c, run, q, False, None, ("P = 0", qk))
        assert r.P == 0 and r.stats == (c.n, 0) and r.N == c.n and 64 < r.N <= 4096


def test_P_zero_fewer_allowed_rows_than_k(kp, torch_):
    """7 allowed rows, k = 10: P = 0, the 7 keys, then zeros."""
    c = _case(kp, torch_, "unit", N_SMALL, 768, False, 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, 10)
    mask = np.zeros(c.n, bool)
    mask[[0, 3, 31, 32, 1000, c.n - 2, c.n - 1]] = True
    r = _search(kp, torch_, c, run, _queries(c, ("unit",))[0][0], True, mask, "7 allowed rows")
    assert r.P == 0 and r.N == 7 and r.stats == (7, 0)
    assert set(St.key_rows(r.dst[:7]) - c.row_base) == set(np.nonzero(mask)[0]) and not r.dst[7:].any()


@pytest.mark.parametrize("kind,qk,k", [("pm_absmax", "pm_amax", 10), ("unit", "unit", 1), ("unit", "copy_row", 1)])
def test_small_final_sort(kp, torch_, kind, qk, k):
    """Tight brackets (exact int8 images of +-A rows and a +-amax query; k = 1
    on unit rows): at most 64 keys reach P and one wave sorts them."""
    c = _case(kp, torch_, kind, N_SMALL, 768, False, 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    r = _search(kp, torch_, c, run, _queries(c, (qk,))[0][0], False, None, ("one-wave sort", kind, qk))
    assert k <= r.N <= 64, r.N


@pytest.mark.parametrize("k", [10, 65])
def test_filters(kp, torch_, k):
    """Density 0.5; a mask that empties whole scan workgroups, the last one
    included; nothing allowed (the engine never sends it: dst all 0, both
    counters left at 0, nothing rescored)."""
    c = _case(kp, torch_, "unit", N_MID, 768, False, 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    Q, kinds = _queries(c, ("unit", "copy_row"))
    half = np.random.default_rng(8).random(c.n) < 0.5
    whole = (c.wg % 2 == 0) & (c.wg != c.nscan - 1)
    for q, qk in zip(Q, kinds):
        for name, mask in (("half", half), ("whole workgroups", whole)):
            r = _search(kp, torch_, c, run, q, True, mask, (name, qk, k))
            assert mask[St.key_rows(r.dst) - c.row_base].all()
            if name != "half":
                assert not r.lbest[1::2].any() and not r.lbest[-1] and r.lbest[0:-1:2].all()
        r = _search(kp, torch_, c, run, q, True, np.zeros(c.n, bool), ("nothing allowed", qk, k))
        assert not r.dst.any() and not r.lbest.any() and not r.ulist.any() and r.stats == (0, 0) and r.N == 0


@pytest.mark.parametrize("row_base", [3 * 4096, None], ids=["3x4096", "largest"])
@pytest.mark.parametrize("k", [10, 65])
def test_row_base(kp, torch_, k, row_base):
    """row_base = 3 * 4096 and 0xFFFFFFFE - n, the largest the engine admits
    (row_base + rows < 2^32 - 1): the keys carry global rows, the finish maps
    them back to local rows and workgroups."""
    n = N_MID
    rb = 0xFFFFFFFE - n if row_base is None else row_base
    c = _case(kp, torch_, "unit", n, 768, True, rb)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    Q, kinds = _queries(c, ("unit", "copy_row", "zero"))
    for q, qk in zip(Q, kinds):
        r = _search(kp, torch_, c, run, q, False, None, ("row_base", hex(rb), qk))
        rows = St.key_rows(r.dst)
        assert rows.min() >= rb and rows.max() < rb + n
        if qk == "zero":
            assert np.array_equal(rows, rb + np.arange(k))
        if qk == "copy_row":
            assert rows[0] == rb + n // 3


@pytest.mark.parametrize("kind,dim,f32,cosine,k,n", [
    _p("negative", 768, False, False, 10, N_MID), _p("negative", 1024, True, False, 65, N_MID),
    _p("clipped", 768, True, False, 10, N_MID), _p("zero_rows", 768, False, True, 64, N_MID),
    _p("zero_rows", 1024, False, False, 128, N_MID)])
def test_negative_clipped_and_zero_rows(kp, torch_, kind, dim, f32, cosine, k, n):
    """All-negative scores (rows -u + noise, query u, dot: every image under
    0x80000000, P included); rows clipped under a stale S (large dt); zero
    rows and a whole zero tile (dt = nt = 0 there)."""
    if kind == "negative":
        rd = (lambda a: a) if f32 else R._bf16
        u = R._unit(np.random.default_rng(12), 1, dim)[0]

        def rows(X):
            return rd((-u[None] + np.float32(0.3) * X).astype(np.float32))
        c = _case(kp, torch_, kind, n, dim, f32, 4096, rows)
        r = _search(kp, torch_, c, Gs.Q8Gemv(kp, torch_, c.coll, k), rd(u), cosine, None, (kind, k))
        assert 0 < r.P < 0x80000000 and np.all(St.key_scores(r.dst) < 0) and np.all(r.lbest < 0x80000000)
        return
    c = _case(kp, torch_, kind, n, dim, f32, 4096)
    run = Gs.Q8Gemv(kp, torch_, c.coll, k)
    Q, kinds = _queries(c)
    for q, qk in zip(Q, kinds):
        _search(kp, torch_, c, run, q, cosine, None, (kind, qk, k))


# ---------------------------------------------------------------------------
# engine-level reachability
# ---------------------------------------------------------------------------
def _smallest_q8_rows(kp):
    """The smallest row count at which the engine keeps an int8 copy
    (q8_wanted: mfma_tiles_per_wg >= 8)."""
    lo, hi = 1, 1 << 22
    assert kp.mfma_tiles_per_wg(hi) >= 8
    while lo < hi:
        mid = (lo + hi) // 2
        if kp.mfma_tiles_per_wg(mid) >= 8:
            hi = mid
        else:
            lo = mid + 1
    assert kp.mfma_tiles_per_wg(lo) >= 8 and kp.mfma_tiles_per_wg(lo - 1) < 8
    return lo


def _one(e, name, Q, k, allow=None):
    out = [e.search(name, Q[i:i + 1], k) if allow is None else e.search_filtered(name, Q[i:i + 1], k, allow)
           for i in range(Q.shape[0])]
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


def _same(a, b):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("how", ["row_base", "dense_filter", "after_delete"])
def test_engine_takes_the_int8_path(kp, pkg, orc, how):
    """The smallest collection that keeps an int8 copy (row count from the
    shim): one-query searches equal the prefilter=False engine bit for bit and
    match the oracle at k = 1, 64, 65, 128 -- in a second collection (so
    row_base != 0), under a dense filter (more than 1/8 of the rows), and
    after a delete that leaves a ragged last tile."""
    n, dim = _smallest_q8_rows(kp), 768
    if how == "after_delete":
        n += 37  # the delete takes 37 rows: the smallest such collection is left
    a = pkg.VectorEngine(device=0)
    b = pkg.VectorEngine(device=0, prefilter=False)
    try:
        X = orc.generate(41, 0, n, dim, bf16=True)
        rb = 3 * 4096 if how == "row_base" else 0
        for e in (a, b):
            e.create_collection("s", dim, pkg.METRIC_COSINE, pkg.DTYPE_BF16, n, rb)
            e.upsert("s", np.arange(n), X)
        assert a.prefilter_bytes("s") > 0 and b.prefilter_bytes("s") == 0
        allow, ids = None, np.arange(n, dtype=np.uint64)  # ids: the oracle's rows -> stored rows
        if how == "dense_filter":
            allow = np.random.default_rng(2).random(n) < 0.3
            assert allow.sum() * 8 > n
            ids = np.nonzero(allow)[0].astype(np.uint64)
        if how == "after_delete":
            gone = np.arange(7, n, 1000)[:37]
            for e in (a, b):
                frm, to = e.delete("s", gone)
            X = X.copy()
            X[to.astype(np.int64)] = X[frm.astype(np.int64)]
            X = X[:n - len(gone)]
            ids = ids[:len(X)]
            assert a.prefilter_bytes("s") > 0 and len(X) % 32 != 0
        Q = orc.generate(orc.SEED_QUERY, 321, 2, dim)
        qp = orc.preprocess(Q, True, True)
        for k in (1, 64, 65, 128):
            ra = _one(a, "s", Q, k, allow)
            _same(ra, _one(b, "s", Q, k, allow))
            _, s64, rows, cnt = orc.search(X[ids.astype(np.int64)] if allow is not None else X, qp, k)
            rows = ids[rows.astype(np.int64)] + np.uint64(rb)
            bad = orc.check_topk(ra[0], ra[1], ra[2], s64, rows, cnt, orc.rescore(X, qp, ra[1], ra[2], rb),
                                 SCORE_RTOL)
            assert not bad, (how, k, bad[:4])
            assert ra[1].min() >= rb
    finally:
        a.close()
        b.close()
