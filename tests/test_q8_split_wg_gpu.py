"""(GPU) The 768-d int8 pass as two 4-wave workgroups a logical workgroup
(csrc/vs_kernels.hip, kSplit): physical block b is logical workgroup b >> 1
with wave parity p = b & 1; it streams only the pieces rg = p and rg = 2 + p
of every 32-row tile (tile rows 8p .. 8p+7 and 16+8p .. 16+8p+7) through a
6-slot ring of its own and writes quarters 2p and 2p + 1 of every (logical
workgroup, query) slab stream. Nothing the pass writes may show it: every
word of the slabs, tile rows, counts and maxima is compared with numpy on the
exact integer dots of the device's own int8 images, the untouched words
against a pattern.

Collections: 768-d, T tiles a logical workgroup at the device's workgroup
count (T = 8 is about 65.5k rows at 256 workgroups), row_base != 0. One
collection serves several row counts: the launch's n_rows cuts the last tile
short, and the rows behind it (live int8 data in memory) must come out as
padding. Queries are orthonormal and background rows short (0.05), so a
planted row s * q scores s against q and next to nothing against the rest; a
bound of 0.12 admits exactly the planted rows. The reference asserts that no
slab maximum is within MARGIN integer units of a threshold.
"""
import ctypes
import os

import numpy as np
import pytest

import q8_ref as R
import q8_stage as St

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MARGIN = 1000              # integer dot units between any slab maximum and a threshold
OFF = 1e30                 # a bound nothing reaches (threshold 2^30)
PAT_SLAB, PAT_TILE, PAT_CNT = 0x5A5A5A5A, 0x6B6B6B6B, 0x7C7C7C7C
ROW_BASE = 3 * 4096
DIM = 768
# the last tile's planted rows: the first row of each 8-row piece (0, 8, 16,
# 24) and the last live row at 8, 16 and 24 live rows (7, 15, 23); the last
# live row at 1, 9, 17 and 25 is the first row of a piece
LAST_ROWS = {0: 3, 7: 40, 8: 77, 15: 130, 16: 200, 23: 255, 24: 64}   # tile row -> query
LIVE = [1, 8, 9, 16, 17, 24, 25]


def _i32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def kpr(kp):
    """The run_if entry point (tests/kprobe/vs_kprobe_runif.cpp)."""
    import __graft_entry__ as ge
    path = os.path.join(ge.PKG_DIR, "lib", "libvs_kprobe_runif.so")
    assert os.path.exists(path), f"{path} not found: run __graft_entry__.build() first"
    fn = ctypes.CDLL(path).kpr_mfma_cand_q8
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    fn.restype = ctypes.c_int
    fn.argtypes = [u64, u32, u32, u32, u64, u32, u32, u64, u64, u64, u64, u64, u32, u64, u64, u32,
                   ctypes.POINTER(u32), u64, u64, u64]
    return fn


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


class Env:
    """A collection of T tiles a logical workgroup (n_max rows: 25 live rows in
    the last tile), or of n_rows rows in one workgroup (T = 1)."""

    def __init__(self, kp, torch, T, n_rows=None):
        self.kp, self.torch, self.T = kp, torch, T
        self.nqk = kp.mfma_queries(DIM, 0)
        assert self.nqk == 256
        self.slots = kp.mfma_query_slots
        wgs = kp.mfma_max_lists(10 ** 6) if n_rows is None else 1
        self.n_max = n = 32 * T * wgs - 7 if n_rows is None else n_rows
        self.nwg, self.rpw = kp.grid(n)
        assert (self.nwg, self.rpw) == (wgs, 32 * T)
        rng = np.random.default_rng(1000 + T)
        qmat, _ = np.linalg.qr(rng.standard_normal((DIM, self.nqk)))
        self.Q = R._bf16(np.ascontiguousarray(qmat.T, np.float32))
        X = rng.standard_normal((n, DIM), dtype=np.float32) * np.float32(0.05 / np.sqrt(DIM))
        self.planted = {}
        self._plant(X)
        self.X = R._bf16(X)
        self.coll = St.Collection(kp, torch, self.X, False, row_base=ROW_BASE)
        self.qs = St.Queries(kp, torch, self.Q, False).quantize(self.coll)
        x8, _, self.glob = self.coll.read()
        q8, self.par, _ = self.qs.read()
        # |dot| <= 127^2 dim < 2^24 and so is every partial sum: exact in float32
        self.d = (x8[:n].astype(np.float32) @ q8.astype(np.float32).T).astype(np.int32)
        self.bufs = {}

    def row(self, wg, tile, r):
        return wg * self.rpw + tile * 32 + r

    def _plant(self, X):
        def plant(wg, tile, r, q, strength):
            i = self.row(wg, tile, r)
            if i >= self.n_max:
                return
            assert i not in self.planted
            self.planted[i] = q
            X[i] = np.float32(strength) * self.Q[q]

        T, last = self.T, self.nwg - 1
        for r, q in LAST_ROWS.items():     # the last tile of the last workgroup
            plant(last, T - 1, r, q, 0.6)
        if self.nwg == 1:
            plant(0, 0, self.n_max - 1, 100, 0.6)   # the last live row of the tiny collection
            return
        if T > 1:
            plant(last, 0, 30, 10, 0.6)
        # one row for every query, in the first tile (even queries) or the last
        # (odd) of a workgroup each: every tile row, so every quarter, both
        # halves and both parities
        for q in range(self.nqk):
            plant(q % last, 0 if q % 2 == 0 else T - 1, (q // 2) % 32, q, 0.5)

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

    def expected(self, th, cap, n, mask=None):
        nwg, nqk, sub, T = self.nwg, self.nqk, cap // 4, self.T
        # every tile slot of every workgroup; rows from n on, padding rows and
        # hidden rows never pass
        d = np.full((nwg * T * 32, nqk), INT_MIN, np.int32)
        d[:n] = self.d[:n]
        if mask is not None:
            d[:n][~mask[:n]] = INT_MIN
        # row 16 h + 4 kq + i of a tile is entry b = 4 h + i of quarter kq's slab
        slab = d.reshape(nwg, T, 2, 4, 4, nqk).transpose(0, 1, 3, 5, 2, 4).reshape(nwg, T, 4, nqk, 8)
        mx = slab.max(-1).astype(np.int64)                   # [wg, tile, quarter, query]
        gap = np.abs(mx - th[None, None, None, :])
        gap[mx == INT_MIN] = MARGIN + 1      # all-dead slabs: below every threshold (>= INT_MIN + 2)
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
    def run(self, bound, nq, cap=None, mask=None, n=None, stand_down=None):
        """One int8 pass over the first n rows; bound: [nqk] per-query bounds or
        None (no bound). stand_down: the run_if entry point, launched with its
        word at 0. Compares every output word -> (Slabs, expectation)."""
        kp, torch = self.kp, self.torch
        n = self.n_max if n is None else n
        assert kp.grid(n) == (self.nwg, self.rpw) and n > self.n_max - 25
        cap = cap or max(16, 4 * self.T)
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
            allow = St._i64(torch, St.pack_allow(mask[:n], self.coll.pad // 64 + 2))
        nl = ctypes.c_uint32(0)
        args = [self.coll.X8d.data_ptr(), DIM, n, ROW_BASE, self.qs.q8.data_ptr(), nq, 10,
                bd.data_ptr() if bd is not None else 0, self.qs.par.data_ptr(),
                self.coll.glob.data_ptr(), S.slabs.data_ptr(), S.tile.data_ptr(), cap,
                S.cnt.data_ptr(), S.cmx.data_ptr(), self.nwg, ctypes.byref(nl),
                self.qs.gate.data_ptr(), allow.data_ptr() if allow is not None else 0]
        if stand_down is not None:
            word = torch.zeros(4, dtype=torch.int32, device=St.DEV)
            kp.check(stand_down(*args, word.data_ptr()))
        else:
            kp.check(kp.mfma_cand_q8(*args))
        assert nl.value == self.nwg
        torch.cuda.synchronize()
        if stand_down is not None:
            for name, t, pat in (("slabs", S.slabs, PAT_SLAB), ("tile words", S.tile, PAT_TILE),
                                 ("counts", S.cnt, PAT_CNT), ("maxima", S.cmx, PAT_CNT)):
                assert bool((t == _i32(pat)).all()), f"a launch standing down wrote {name}"
            return S, None
        E = self.expected(self.thresholds(bound, nq), cap, n, mask)
        what = (self.T, n, nq, cap, mask is not None, bound is None)
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
        return S, E

    def admitted(self, E, q):
        """-> [(workgroup, tile, quarter)] of query q's admitted slabs."""
        return [tuple(int(v) for v in x) for x in np.argwhere(E["ps"][..., q])]

    def planted_admitted(self, E, n, mask=None):
        """Every planted row that is live (and visible) is the admitted slab of
        its query at its place, and nothing else is admitted."""
        want = {}
        for i, q in self.planted.items():
            if i < n and (mask is None or mask[i]):
                want.setdefault(q, set()).add((i // self.rpw, i % self.rpw // 32, i % 16 // 4))
        for q in range(self.nqk):
            assert set(self.admitted(E, q)) == want.get(q, set()), (q, self.admitted(E, q))


@pytest.fixture(scope="module")
def env(kp, torch_):
    e = Env(kp, torch_, 8)
    yield e
    e.bufs.clear()


def _bounds(e, level=0.12):
    return np.full(e.nqk, level, np.float32)


def _mask(e):
    """Density 1/2; in the last tile rows r and 16 + r (the two halves of a
    quarter) always differ, and of the planted rows 0, 8, 23 show while 7, 15,
    16, 24 hide."""
    mask = np.random.default_rng(7).random(e.n_max + 7) >= 0.5
    lo = np.array([1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0], bool)
    t0 = e.row(e.nwg - 1, e.T - 1, 0)
    mask[t0:t0 + 16], mask[t0 + 16:t0 + 32] = lo, ~lo
    return mask[:e.n_max]


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("live", LIVE)
def test_live_row_boundary_in_both_parities(env, live, filtered):
    """The last logical workgroup's last tile with 1 .. 25 live rows: at 1 .. 8
    the parity-1 block has no live row in it, at 9 .. 16 only its lower piece.
    Rows behind the boundary hold live int8 data and must come out INT_MIN."""
    e = env
    n = e.n_max - 25 + live
    mask = _mask(e) if filtered else None
    S, E = e.run(_bounds(e), e.nqk, n=n, mask=mask)
    e.planted_admitted(E, n, mask)
    t0 = e.row(e.nwg - 1, e.T - 1, 0)
    shown = [r for r in LAST_ROWS if r < live and (mask is None or mask[t0 + r])]
    assert (live - 1 in shown) or filtered, "the last live row is planted"
    assert len(shown) >= 1


@pytest.mark.parametrize("T", [1, 5, 6, 7, 13])
def test_tiles_per_logical_workgroup(kp, torch_, T):
    """Below, at and past the 6-slot ring's wrap, and two wraps plus one:
    planted rows in the first and last tile of the workgroups, every output
    word compared."""
    e = Env(kp, torch_, T)
    S, E = e.run(_bounds(e), e.nqk)
    e.planted_admitted(E, e.n_max)
    tiles = {t for q in range(e.nqk) for _, t, _ in e.admitted(E, q)}
    assert tiles == {0, T - 1}


def test_five_rows_one_logical_workgroup(kp, torch_):
    """5 rows: one logical workgroup, two blocks; the parity-1 block streams
    nothing but padding and writes zero counts and INT_MIN maxima."""
    e = Env(kp, torch_, 1, n_rows=5)
    assert e.nwg == 1
    S, E = e.run(_bounds(e), e.nqk, n=5)
    e.planted_admitted(E, 5)
    assert e.admitted(E, 3) == [(0, 0, 0)] and e.admitted(E, 100) == [(0, 0, 1)]
    assert np.all(E["cnt"][:, 0, 2:] == 0) and np.all(E["cmx"][:, 0, 2:] == INT_MIN)
    S, E = e.run(None, e.nqk, n=5)
    assert np.all(E["cnt"][:, 0, :2] == 1) and np.all(E["cnt"][:, 0, 2:] == 0)


@pytest.mark.parametrize("nq", [256, 200, 33, 1])
def test_invalid_queries_in_both_blocks_of_a_pair(env, nq):
    """nq_valid = 200, 33 and 1 leave whole waves of invalid queries in both
    blocks of every pair: they append nothing and their slots keep the pattern."""
    e = env
    S, E = e.run(_bounds(e), nq)
    per_q = E["cnt"].sum((1, 2))
    assert np.all(per_q[:nq] >= 1) and np.all(per_q[nq:] == 0)
    assert np.all(E["cmx"][nq:] == INT_MIN)
    if nq < e.nqk:
        assert bool((S.slabs[:, nq:e.nqk] == _i32(PAT_SLAB)).all())


def test_no_bound_every_lane_appends_and_quarters_go_lossy(env):
    """No bound: every lane of both blocks admits every tile; at 4 slots a
    quarter the counts run on to the tile count, the first 4 slabs are stored,
    the maxima are those of all tiles."""
    e = env
    S, E = e.run(None, e.nqk, cap=16)
    assert np.all(E["cnt"] == e.T)
    S, E = e.run(None, 200, cap=16, n=e.n_max - 24)
    assert np.all(E["cnt"][200:] == 0)
    assert np.all(E["cnt"][:200, e.nwg - 1, 0] == e.T) and np.all(E["cnt"][:200, e.nwg - 1, 1:] == e.T - 1)


@pytest.mark.parametrize("filtered", [False, True])
def test_stand_down_writes_nothing(env, kpr, filtered):
    """run_if pointing at 0: both blocks of every pair return at once, every
    output word keeps its pattern."""
    e = env
    e.run(None, e.nqk, mask=_mask(e) if filtered else None, stand_down=kpr)


@pytest.mark.parametrize("k", [10, 100])
def test_search_equals_engine_without_prefilter(env, pkg, k):
    """End to end on the same rows and queries: the keys of an engine with the
    int8 prefilter equal those of one without."""
    e = env
    a = pkg.VectorEngine(device=0)
    b = pkg.VectorEngine(device=0, prefilter=False)
    try:
        for eng in (a, b):
            eng.create_collection("sw", DIM, pkg.METRIC_DOT, pkg.DTYPE_BF16, e.n_max)
            eng.upsert("sw", np.arange(e.n_max, dtype=np.uint64), e.X)
        assert a.prefilter_bytes("sw") > 0 and b.prefilter_bytes("sw") == 0
        ra, rb = a.search("sw", e.Q, k), b.search("sw", e.Q, k)
        assert np.array_equal(ra[2], rb[2]) and np.array_equal(ra[1], rb[1])
        assert np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32))
    finally:
        a.close()
        b.close()
