"""(GPU) The 768-d int8 pass's query-half mapping (csrc/vs_kernels.hip, kQH):
waves 2j and 2j+1 share queries 64j .. 64j+63 and wave parity p takes tile
rows 8p .. 8p+7 and 16+8p .. 16+8p+7, so a slab's lower half (rows 4kq+i) and
upper half (16+4kq+i) are computed in lanes l and l ^ 32, joined by one
cross-half exchange for the admission test and once more inside the append.
Nothing the pass writes may show it: every word of the slabs, tile rows,
counts and maxima is compared with numpy on the exact integer dots of the
device's own int8 images, the untouched words against a pattern.

Collection: 768-d, T = 8 tiles a workgroup (the fewest that take the fast
pass), the last workgroup one tile short with 25 live rows in its last tile:
about 65.5k rows at 256 workgroups; row_base != 0. Queries are orthonormal
and background rows short (0.05), so a planted row s * q scores s against q
and next to nothing against the rest; a bound of 0.12 admits exactly the
planted rows. The reference asserts that no slab maximum is within MARGIN
integer units of a threshold, except in the two exact-threshold cases, whose
bounds are placed so that the float expression of q8_dot_threshold lands
0.4 .. 0.6 above an integer (its rounding, a few 2^-24 relative on values of
about 10^6, i.e. under 0.2, decides nothing).
"""
import ctypes

import numpy as np
import pytest

import q8_ref as R
import q8_stage as St

pytestmark = pytest.mark.gpu

T = 8                      # tiles per workgroup
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MARGIN = 1000              # integer dot units between any slab maximum and a threshold
OFF = 1e30                 # a bound nothing reaches (threshold 2^30)
PAT_SLAB, PAT_TILE, PAT_CNT = 0x5A5A5A5A, 0x6B6B6B6B, 0x7C7C7C7C
ROW_BASE = 5 * 4096
DIM = 768
EDGE_Q = [0, 31, 32, 63, 64, 255]     # first / last query of a group, of a wave pair, of the launch
WG_HALF, WG_EXACT, WG_ALL = 2, 10, 12  # first workgroups of the cases
EXACT_Q = [(0, 0, 1), (63, 1, 22), (255, 2, 14)]   # (query, tile, tile row): lower, upper, lower half


def _i32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


class Env:
    def __init__(self, kp, torch):
        self.kp, self.torch = kp, torch
        self.nqk = kp.mfma_queries(DIM, 0)
        assert self.nqk == 256
        self.slots = kp.mfma_query_slots
        wgs = kp.mfma_max_lists(10 ** 6)
        self.n = n = 32 * T * wgs - 32 - 7
        self.nwg, self.rpw = kp.grid(n)
        assert (self.nwg, self.rpw) == (wgs, 32 * T) and wgs > WG_ALL + 4
        assert kp.mfma_tiles_per_wg(n) == T
        self.tiles = (n + 31) // 32
        rng = np.random.default_rng(99)
        qmat, _ = np.linalg.qr(rng.standard_normal((DIM, self.nqk)))
        self.Q = R._bf16(np.ascontiguousarray(qmat.T, np.float32))
        X = R._unit(rng, n, DIM) * np.float32(0.05)
        self._plant(X)
        self.X = R._bf16(X)
        self.coll = St.Collection(kp, torch, self.X, False, row_base=ROW_BASE)
        self.qs = St.Queries(kp, torch, self.Q, False).quantize(self.coll)
        x8, _, self.glob = self.coll.read()
        q8, self.par, _ = self.qs.read()
        # |dot| <= 127^2 dim < 2^24 and so is every partial sum: exact in float32
        d = (x8[:n].astype(np.float32) @ q8.astype(np.float32).T).astype(np.int32)
        # every tile slot of every workgroup; padding rows and tiles never pass
        self.dots = np.full((self.nwg * T * 32, self.nqk), INT_MIN, np.int32)
        self.dots[:n] = d
        self.bufs = {}

    def row(self, wg, tile, r):
        return wg * self.rpw + tile * 32 + r

    def _plant(self, X):
        put = set()

        def plant(wg, tile, r, q, strength):
            i = self.row(wg, tile, r)
            assert i not in put and i < self.n
            put.add(i)
            X[i] = np.float32(strength) * self.Q[q]

        # a slab whose only planted row is in its lower half (tile 2 kq) and one
        # where it is in the upper half (tile 2 kq + 1): each quarter alone in
        # its tile, for every edge query, a workgroup each
        self.half_rows = {}
        for i, q in enumerate(EDGE_Q):
            for kq in range(4):
                lo, up = 4 * kq + i % 4, 16 + 4 * kq + (i + 1) % 4
                plant(WG_HALF + i, 2 * kq, lo, q, 0.6)
                plant(WG_HALF + i, 2 * kq + 1, up, q, 0.6)
                self.half_rows[(q, kq)] = (self.row(WG_HALF + i, 2 * kq, lo),
                                           self.row(WG_HALF + i, 2 * kq + 1, up))
        # the exact-threshold rows: the strongest of their queries by far
        for q, tile, r in EXACT_Q:
            plant(WG_EXACT, tile, r, q, 0.9)
        # one row for every query: 64 queries a workgroup, 8 a tile, rows in
        # every quarter and both halves
        for q in range(self.nqk):
            plant(WG_ALL + q // 64, q % 8, (q // 8 % 8) * 4 + q % 3, q, 0.5)
        # the last workgroup: T - 1 tiles, 25 live rows in the last one
        last = self.nwg - 1
        assert self.n - self.row(last, T - 2, 0) == 25
        plant(last, T - 2, 24, 0, 0.6)     # the last live row: upper half of quarter 2
        plant(last, T - 2, 3, 64, 0.6)
        plant(last, T - 3, 30, 255, 0.6)

    # ---- reference ----------------------------------------------------------
    def t_of(self, bound):
        """q8_dot_threshold's float expression in numpy fp32 -> [nqk] (before the floor)."""
        f = np.float32
        p = self.par.astype(f)
        dmax, nmax = f(self.glob[1]), f(self.glob[2])
        b = np.asarray(bound, f)
        assert np.all(np.isfinite(b)) and np.all(p[:, 0] > 0)
        return ((b - p[:, 1] * dmax - (p[:, 2] + f(2) * p[:, 3]) * nmax) / p[:, 0] - f(1)).astype(f)

    def thresholds(self, bound, nq):
        if bound is None:                          # no bound: every row
            th = np.full(self.nqk, INT_MIN + 2, np.int64)
        else:
            t = self.t_of(bound)
            th = np.floor(np.clip(t.astype(np.float64), -2.0 ** 30, 2.0 ** 30)).astype(np.int64)
            th[t <= -2.0 ** 30] = INT_MIN + 2
        th[nq:] = INT_MAX
        return th

    def bound_for(self, q, target):
        """A bound whose threshold for query q is `target`, the float
        expression landing 0.4 .. 0.6 above it."""
        f = np.float32
        p = self.par.astype(np.float64)[q]
        dmax, nmax = float(self.glob[1]), float(self.glob[2])
        b = f((target + 1.5) * p[0] + p[1] * dmax + (p[2] + 2 * p[3]) * nmax)
        probe = np.full(self.nqk, 1.0, f)
        for _ in range(400):
            probe[q] = b
            fr = float(self.t_of(probe)[q]) - target
            if 0.4 <= fr <= 0.6:
                return b
            b = np.nextafter(b, f(np.inf) if fr < 0.5 else f(-np.inf))
        raise AssertionError(("no bound puts the threshold expression mid-integer", q, target, fr))

    def expected(self, th, cap, mask=None, exact=()):
        nwg, nqk, sub = self.nwg, self.nqk, cap // 4
        d = self.dots
        if mask is not None:
            d = d.copy()
            d[:self.n][~mask] = INT_MIN
        # row 16 h + 4 kq + i of a tile is entry b = 4 h + i of quarter kq's slab
        slab = d.reshape(nwg, T, 2, 4, 4, nqk).transpose(0, 1, 3, 5, 2, 4).reshape(nwg, T, 4, nqk, 8)
        mx = slab.max(-1).astype(np.int64)                   # [wg, tile, quarter, query]
        gap = np.abs(mx - th[None, None, None, :])
        gap[mx == INT_MIN] = MARGIN + 1      # all-dead slabs: below every threshold (>= INT_MIN + 2)
        if len(exact):
            gap[..., list(exact)] = np.where(gap[..., list(exact)] <= 1, MARGIN + 1, gap[..., list(exact)])
        assert gap.min() > MARGIN, ("a slab maximum next to the threshold", int(gap.min()))
        ps = mx >= th[None, None, None, :]
        rank = np.cumsum(ps, axis=1) - ps                    # slabs of the stream before this one
        cnt = ps.sum(1).transpose(2, 0, 1)                   # [query, wg, quarter]
        cmx = np.where(ps, mx, INT_MIN).max(1).transpose(2, 0, 1)
        st = ps & (rank < sub)
        w, t, kq, q = np.nonzero(st)
        e = (w * self.slots + q) * cap + kq * sub + rank[st]
        es = np.full((nwg * self.slots * cap, 8), _i32(PAT_SLAB), np.int32)
        et = np.full(nwg * self.slots * cap, _i32(PAT_TILE), np.int32)
        es[e] = slab[w, t, kq, q]
        et[e] = (ROW_BASE + (w * T + t) * 32).astype(np.uint32).view(np.int32)
        return dict(es=es, et=et, cnt=cnt, cmx=cmx, ps=ps)

    # ---- launch and compare -------------------------------------------------
    def run(self, bound, nq, cap=4 * T, mask=None, exact=()):
        """One int8 pass; bound: [nqk] per-query bounds or None (no bound).
        Compares every output word -> (Slabs, expectation, bound tensor, allow)."""
        kp, torch = self.kp, self.torch
        if cap not in self.bufs:
            self.bufs[cap] = St.Slabs(kp, torch, self.nwg, cap)
        S = self.bufs[cap]
        S.slabs.fill_(_i32(PAT_SLAB)), S.tile.fill_(_i32(PAT_TILE))
        S.cnt.fill_(_i32(PAT_CNT)), S.cmx.fill_(_i32(PAT_CNT))
        bd = None
        if bound is not None:
            bd = torch.full((self.slots,), OFF, dtype=torch.float32, device=St.DEV)
            bd[:self.nqk] = torch.from_numpy(np.asarray(bound, np.float32)).to(St.DEV)
        allow = None
        if mask is not None:
            allow = St._i64(torch, St.pack_allow(mask, self.coll.pad // 64 + 2))
        nl = ctypes.c_uint32(0)
        kp.check(kp.mfma_cand_q8(self.coll.X8d.data_ptr(), DIM, self.n, ROW_BASE, self.qs.q8.data_ptr(),
                                 nq, 10, bd.data_ptr() if bd is not None else 0, self.qs.par.data_ptr(),
                                 self.coll.glob.data_ptr(), S.slabs.data_ptr(), S.tile.data_ptr(), cap,
                                 S.cnt.data_ptr(), S.cmx.data_ptr(), self.nwg, ctypes.byref(nl),
                                 self.qs.gate.data_ptr(), allow.data_ptr() if allow is not None else 0))
        assert nl.value == self.nwg
        torch.cuda.synchronize()
        E = self.expected(self.thresholds(bound, nq), cap, mask, exact)
        what = (nq, cap, mask is not None, bound is None)
        got_cnt = S.cnt.cpu().numpy().view(np.uint32)
        got_cmx = S.cmx.cpu().numpy()
        live = self.nqk * self.nwg * 4                  # [query][workgroup][quarter]
        bad = np.argwhere(got_cnt[:live].reshape(self.nqk, self.nwg, 4) != E["cnt"])
        assert bad.size == 0, ("counts (query, workgroup, quarter)", what, bad[:5].tolist())
        bad = np.argwhere(got_cmx[:live].reshape(self.nqk, self.nwg, 4) != E["cmx"])
        assert bad.size == 0, ("maxima (query, workgroup, quarter)", what, bad[:5].tolist())
        assert np.all(got_cnt[live:] == PAT_CNT) and np.all(got_cmx[live:].view(np.uint32) == PAT_CNT), \
            "counts / maxima written past the launch's queries"
        et = torch.from_numpy(E["et"]).to(St.DEV).view_as(S.tile)
        if not torch.equal(S.tile, et):
            bad = torch.nonzero(S.tile != et)[:5].cpu().tolist()
            raise AssertionError(("tile words (workgroup, query, slot)", what, bad))
        es = torch.from_numpy(E["es"]).to(St.DEV).view_as(S.slabs)
        if not torch.equal(S.slabs, es):
            bad = torch.nonzero(S.slabs != es)[:5].cpu().tolist()
            raise AssertionError(("slabs (workgroup, query, slot, entry)", what, bad))
        return S, E, bd, allow

    def admitted(self, E, q):
        """-> [(workgroup, tile, quarter)] of query q's admitted slabs."""
        return [tuple(int(v) for v in x) for x in np.argwhere(E["ps"][..., q])]


@pytest.fixture(scope="module")
def env(kp, torch_):
    e = Env(kp, torch_)
    yield e
    e.bufs.clear()


def _bounds(e, on, level=0.12):
    b = np.full(e.nqk, OFF, np.float32)
    b[np.array(list(on), np.int64)] = level
    return b


def test_lower_and_upper_half_each_quarter_alone(env):
    """For the queries 0, 31, 32, 63, 64, 255: per quarter one slab whose only
    passing dot is in rows 4kq+i (its owner lane's own accumulators) and one
    where it is in rows 16+4kq+i (the partner lane's), each quarter alone in
    its tile."""
    e = env
    S, E, _, _ = e.run(_bounds(e, EDGE_Q), e.nqk)
    for i, q in enumerate(EDGE_Q):
        got = [x for x in e.admitted(E, q) if x[0] == WG_HALF + i]
        assert got == [(WG_HALF + i, t, t // 2) for t in range(8)], (q, got)
        for kq in range(4):
            lo, up = e.half_rows[(q, kq)]
            sub = T
            sl = S.slabs[WG_HALF + i, q, kq * sub:kq * sub + 2].cpu().numpy()
            th = e.thresholds(_bounds(e, EDGE_Q), e.nqk)[q]
            assert sl[0, lo % 32 % 4] == e.dots[lo, q] >= th and np.all(sl[0, 4:] < th)
            assert sl[1, 4 + up % 32 % 4] == e.dots[up, q] >= th and np.all(sl[1, :4] < th)


@pytest.mark.parametrize("below", [False, True])
def test_dot_at_the_threshold_and_one_below(env, below):
    """The threshold of a query equal to its strongest row's dot: admitted;
    one higher (the dot one below it): nothing admitted. Rows in a lower half,
    an upper half and the launch's last query."""
    e = env
    b = np.full(e.nqk, OFF, np.float32)
    for q, tile, r in EXACT_Q:
        d = int(e.dots[e.row(WG_EXACT, tile, r), q])
        assert d == e.dots[:, q].max()
        b[q] = e.bound_for(q, d + (1 if below else 0))
        assert e.thresholds(b, e.nqk)[q] == d + (1 if below else 0)
    S, E, _, _ = e.run(b, e.nqk, exact=[q for q, _, _ in EXACT_Q])
    for q, tile, r in EXACT_Q:
        want = [] if below else [(WG_EXACT, tile, (r % 16) // 4)]
        assert e.admitted(E, q) == want
    assert int(E["cnt"].sum()) == (0 if below else len(EXACT_Q))


@pytest.mark.parametrize("nq", [256, 200, 33])
def test_every_query_and_invalid_queries_inside_a_wave_pair(env, nq):
    """Every query's planted rows at nq_valid = 256; at 200 and 33 the
    invalid queries share a wave pair (and at 33 a group) with valid ones:
    they append nothing and their slots keep the pattern."""
    e = env
    S, E, _, _ = e.run(_bounds(e, range(e.nqk)), nq)
    per_q = E["cnt"].sum((1, 2))
    assert np.all(per_q[:nq] >= 1) and np.all(per_q[nq:] == 0)
    assert np.all(E["cmx"][nq:] == INT_MIN)
    if nq < e.nqk:
        assert bool((S.slabs[:, nq:e.nqk] == _i32(PAT_SLAB)).all())
    # the last workgroup's partial tile: query 0's row is the last live one
    last = e.nwg - 1
    assert (last, T - 2, 2) in e.admitted(E, 0)
    sl = S.slabs[last, 0, 2 * T].cpu().numpy()
    assert sl[4] == e.dots[e.n - 1, 0] and np.all(sl[5:] == INT_MIN) and np.all(sl[:4] > INT_MIN)


def test_no_bound_every_lane_appends_and_quarters_go_lossy(env):
    """No bound: every lane admits every tile; at 4 slots a quarter the counts
    run on to the tile count, the first 4 slabs are stored, the maxima are
    those of all tiles."""
    e = env
    S, E, _, _ = e.run(None, e.nqk, cap=16)
    assert np.all(E["cnt"][:, :e.nwg - 1] == T) and np.all(E["cnt"][:, e.nwg - 1, :3] == T - 1)
    S, E, _, _ = e.run(None, 200, cap=16)
    assert np.all(E["cnt"][200:] == 0)


def test_filter_of_density_one_half(env):
    """Half the rows hidden (planted ones too): every tile runs the masking
    body, hidden rows are INT_MIN in the slabs and admit nothing."""
    e = env
    mask = np.random.default_rng(11).random(e.n) >= 0.5
    S, E, bd, allow = e.run(_bounds(e, range(e.nqk)), e.nqk, mask=mask)
    hidden = [q for q in EDGE_Q for kq in range(4) for r in e.half_rows[(q, kq)] if not mask[r]]
    assert hidden, "the mask hides none of the planted rows"
    n_adm = int(E["cnt"].sum())
    _, E0, _, _ = e.run(_bounds(e, range(e.nqk)), e.nqk)
    assert 0 < n_adm < int(E0["cnt"].sum())


@pytest.mark.parametrize("k", [10, 100])
def test_search_equals_engine_without_prefilter(env, pkg, k):
    """End to end on the same rows and queries: the keys of an engine with the
    int8 prefilter equal those of one without."""
    e = env
    a = pkg.VectorEngine(device=0)
    b = pkg.VectorEngine(device=0, prefilter=False)
    try:
        for eng in (a, b):
            eng.create_collection("qh", DIM, pkg.METRIC_DOT, pkg.DTYPE_BF16, e.n)
            eng.upsert("qh", np.arange(e.n, dtype=np.uint64), e.X)
        assert a.prefilter_bytes("qh") > 0 and b.prefilter_bytes("qh") == 0
        ra, rb = a.search("qh", e.Q, k), b.search("qh", e.Q, k)
        assert np.array_equal(ra[2], rb[2]) and np.array_equal(ra[1], rb[1])
        assert np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32))
    finally:
        a.close()
        b.close()
