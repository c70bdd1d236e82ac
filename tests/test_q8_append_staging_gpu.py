"""(GPU) The int8 pass's append path (csrc/vs_kernels.hip, q8_epi*): one
wave-uniform admission test per tile, and in the one-group pass (1024-d) a
wave stages the slabs it admits in LDS and stores them in batches, at most
kStageCap records at a time; an admission event larger than that goes
straight to the buffers behind a flush; the last records leave by the flush
at the end of the kernel. The two-group pass (768-d) stores every event
directly. What the pass writes must not depend on any of it, so every case
runs at both dimensions and compares the candidate buffers, tile words,
counts and maxima -- every word of them, the untouched ones against a
pattern -- with numpy's on the exact integer dots of the device's own int8
images.

One collection per dimension holds every case's planted rows, each case in
workgroups of its own (a wave's stage never leaves its workgroup), and a case
picks its admissions with the per-query bounds. Queries are orthonormal and
background rows are short, so a planted row strength * q scores its strength
against q and next to nothing against any other query; the bounds lie
between the levels, at least 0.05 in score from any row, against the
threshold's own slack of about 0.02 (q8_dot_threshold: a dmax + (c + 2 sigma)
nmax). The reference asserts that no lane's slab maximum is within MARGIN
integer units of a threshold, so the threshold's rounding decides nothing.

Geometry: T = 9 tiles a workgroup, the last workgroup two tiles short with a
partial last tile (7 rows missing): about 73.6k rows at 256 workgroups.
"""
import copy
import ctypes

import numpy as np
import pytest

import q8_ref as R
import q8_stage as St

pytestmark = pytest.mark.gpu

T = 9                      # tiles per workgroup
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MARGIN = 1000              # integer dot units between any slab maximum and a threshold
OFF = 1e30                 # a bound nothing reaches (threshold 2^30)
PAT_SLAB, PAT_TILE, PAT_CNT = 0x5A5A5A5A, 0x6B6B6B6B, 0x7C7C7C7C
LEVELS = [1.0 - 0.1 * t for t in range(T)]   # the sweep's strength in tile t
ROW_BASE = 3 * 4096
DIMS = [768, 1024]

# workgroups of the cases
WG_SWEEP, WG_BIG, WG_GROUPS, WG_FILTER, WG_LOSSY, WG_NQ = 2, 4, 6, 8, 10, 12


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
    """The collection of one dimension with every case's planted rows, its
    queries, the exact dots and the pattern-filled output buffers."""

    def __init__(self, kp, torch, dim):
        self.kp, self.torch, self.dim = kp, torch, dim
        self.nqk = kp.mfma_queries(dim, 0)          # queries a launch covers
        self.qpw = self.nqk // 8                    # queries per wave
        self.slots = kp.mfma_query_slots
        wgs = kp.mfma_max_lists(10 ** 6)
        self.n = n = 32 * T * wgs - 64 - 7
        self.nwg, self.rpw = kp.grid(n)
        assert (self.nwg, self.rpw) == (wgs, 32 * T) and wgs > WG_NQ + 1
        self.tiles = (n + 31) // 32
        rng = np.random.default_rng(4242 + dim)
        qmat, _ = np.linalg.qr(rng.standard_normal((dim, self.nqk)))
        self.Q = R._bf16(np.ascontiguousarray(qmat.T, np.float32))
        X = R._unit(rng, n, dim) * np.float32(0.05)
        self.masked = []                            # rows the filter case hides
        self._plant(X)
        self.X = R._bf16(X)
        self.coll = St.Collection(kp, torch, self.X, False, row_base=ROW_BASE)
        self.qs = St.Queries(kp, torch, self.Q, False).quantize(self.coll)
        x8, _, self.glob = self.coll.read()
        q8, self.par, _ = self.qs.read()
        # |dot| <= 127^2 dim < 2^24 and so is every partial sum: exact in float32
        d = (x8[:n].astype(np.float32) @ q8.astype(np.float32).T).astype(np.int32)
        self.dots = np.full((self.tiles * 32, self.nqk), INT_MIN, np.int32)   # padding rows
        self.dots[:n] = d
        self.bufs = {}

    # ---- planted rows -------------------------------------------------------
    def row(self, wg, tile, r):
        return wg * self.rpw + tile * 32 + r

    def _plant(self, X):
        Q, qpw = self.Q, self.qpw
        put = {}

        def plant(wg, tile, r, qs_, strength):
            i = self.row(wg, tile, r)
            assert i not in put and i < self.n
            put[i] = True
            X[i] = np.float32(strength) * Q[list(qs_)].sum(0)

        # sweep: wave 3, pair j = (query j // T, tile j % T), strength by tile
        self.sweep_q = [3 * qpw + qi * (qpw // 16) for qi in range(15)]
        for qi, q in enumerate(self.sweep_q):
            for t in range(T):
                plant(WG_SWEEP, t, (2 * qi) % 32, [q], LEVELS[t])
        # oversized events behind a partly filled stage: wave 0
        g0, gl = range(0, 16), range(qpw - 16, qpw)
        for tile, r, q in ((0, 1, 0), (0, 5, 1), (0, 9, 2), (2, 2, 3), (4, 3, 4)):
            plant(WG_BIG, tile, r, [q], 0.6)
        for tile, grp in ((1, g0), (3, gl)):
            for r in (0, 4, 8, 12):        # one row a quarter, 0.25 against each of the 16
                plant(WG_BIG, tile, r, grp, 0.25)
        # both groups in one tile, then group 1 alone, then group 0 alone
        plant(WG_GROUPS, 0, 0, [0], 0.6)
        plant(WG_GROUPS, 0, 5, [16], 0.6)
        plant(WG_GROUPS, 1, 6, [17], 0.6)
        plant(WG_GROUPS, 2, 7, [1], 0.6)
        # filter: a masked row alone in its slab; a masked row beside a live one
        plant(WG_FILTER, 0, 0, [5], 0.6)
        plant(WG_FILTER, 1, 1, [6], 0.6)
        plant(WG_FILTER, 1, 2, [6], 0.5)
        self.masked += [self.row(WG_FILTER, 0, 0), self.row(WG_FILTER, 1, 1)]
        # lossy quarter: 7 slabs for quarter 0 of query 0, the largest in tile 5; one in quarter 1
        for t, s in enumerate([0.5, 0.6, 0.4, 0.7, 0.3, 0.9, 0.8]):
            plant(WG_LOSSY, t, 0, [0], s)
        plant(WG_LOSSY, 2, 4, [0], 0.6)
        # nq_valid: one row for each of the first 48 queries
        for q in range(48):
            plant(WG_NQ, q % T, q % 32, [q], 0.6)
        # the last workgroup: T - 2 tiles, the last one partial (25 live rows)
        last = self.nwg - 1
        assert self.n - self.row(last, T - 3, 0) == 25
        plant(last, T - 3, 24, [0], 0.6)   # the last live row
        plant(last, T - 3, 3, [7], 0.6)
        plant(last, T - 3, 2, [8], 0.6)
        plant(last, T - 4, 30, [7], 0.5)
        self.masked.append(self.row(last, T - 3, 2))

    # ---- reference ----------------------------------------------------------
    def thresholds(self, bound, nq):
        """q8_dot_threshold in numpy fp32 -> int64 [nqk]."""
        f = np.float32
        p = self.par.astype(f)
        dmax, nmax = f(self.glob[1]), f(self.glob[2])
        b = np.asarray(bound, f)
        assert np.all(np.isfinite(b)) and np.all(p[:, 0] > 0)
        t = ((b - p[:, 1] * dmax - (p[:, 2] + f(2) * p[:, 3]) * nmax) / p[:, 0] - f(1)).astype(f)
        th = np.floor(np.clip(t.astype(np.float64), -2.0 ** 30, 2.0 ** 30)).astype(np.int64)
        th[t <= -2.0 ** 30] = INT_MIN + 2
        th[nq:] = INT_MAX
        return th

    def expected(self, bound, nq, cap, mask=None):
        """-> dict of the sparse writes (flat index, value) into the slab and
        tile buffers, the dense counts and maxima, and the events (tile, kq, q)."""
        nwg, nqk, sub = self.nwg, self.nqk, cap // 4
        th = self.thresholds(bound, nq)
        on = np.nonzero(th < 2 ** 30)[0]            # queries that can admit
        d = self.dots[:, on]
        if mask is not None:
            d = d.copy()
            d[:self.n][~mask] = INT_MIN
        # row 16 h + 4 kq + i of a tile is entry b = 4 h + i of quarter kq's slab
        slab = d.reshape(self.tiles, 2, 4, 4, len(on)).transpose(0, 2, 4, 1, 3).reshape(
            self.tiles, 4, len(on), 8)
        mx = slab.max(-1)
        gap = np.abs(mx - th[on][None, None, :])
        assert gap.min() > MARGIN, ("a slab maximum next to the threshold", int(gap.min()))
        ev = np.argwhere(mx >= th[on][None, None, :])   # ascending tiles
        cnt = np.zeros((nqk, nwg, 4), np.int64)
        cmx = np.full((nqk, nwg, 4), INT_MIN, np.int64)
        si, sv, ti, tv = [], [], [], []
        for t, kq, j in ev:
            q, wg = on[j], (t * 32) // self.rpw
            c = cnt[q, wg, kq]
            if c < sub:
                e = (wg * self.slots + q) * cap + kq * sub + c
                si.append(e * 8 + np.arange(8))
                sv.append(slab[t, kq, j])
                ti.append(e)
                tv.append(ROW_BASE + t * 32)
            cnt[q, wg, kq] = c + 1
            cmx[q, wg, kq] = max(cmx[q, wg, kq], mx[t, kq, j])
        cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)
        return dict(si=cat(si), sv=cat(sv), ti=np.array(ti, np.int64), tv=np.array(tv, np.int64),
                    cnt=cnt, cmx=cmx, ev=[(int(t), int(kq), int(on[j])) for t, kq, j in ev])

    # ---- launch and compare -------------------------------------------------
    def buffers(self, cap):
        if cap not in self.bufs:
            S = St.Slabs(self.kp, self.torch, self.nwg, cap)
            self.bufs[cap] = (S, self.torch.empty_like(S.slabs), self.torch.empty_like(S.tile))
        return self.bufs[cap]

    def run(self, bound, nq, cap=4 * T, mask=None):
        """One int8 pass with per-query bounds `bound` ([nqk]); compares every
        output word with the reference -> (Slabs, expectation, allow tensor)."""
        kp, torch = self.kp, self.torch
        i32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
        S, es, et = self.buffers(cap)
        S.slabs.fill_(i32(PAT_SLAB)), S.tile.fill_(i32(PAT_TILE))
        S.cnt.fill_(i32(PAT_CNT)), S.cmx.fill_(i32(PAT_CNT))
        bd = torch.full((self.slots,), OFF, dtype=torch.float32, device=St.DEV)
        bd[:self.nqk] = torch.from_numpy(np.asarray(bound, np.float32)).to(St.DEV)
        allow = None
        if mask is not None:
            allow = St._i64(torch, St.pack_allow(mask, self.coll.pad // 64 + 2))
        nl = ctypes.c_uint32(0)
        kp.check(kp.mfma_cand_q8(self.coll.X8d.data_ptr(), self.dim, self.n, ROW_BASE, self.qs.q8.data_ptr(),
                                 nq, 10, bd.data_ptr(), self.qs.par.data_ptr(), self.coll.glob.data_ptr(),
                                 S.slabs.data_ptr(), S.tile.data_ptr(), cap, S.cnt.data_ptr(),
                                 S.cmx.data_ptr(), self.nwg, ctypes.byref(nl), self.qs.gate.data_ptr(),
                                 allow.data_ptr() if allow is not None else 0))
        assert nl.value == self.nwg
        torch.cuda.synchronize()
        E = self.expected(bound, nq, cap, mask)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(St.DEV)
        to32 = lambda a: np.asarray(a, np.int64).astype(np.uint32).view(np.int32)
        es.fill_(i32(PAT_SLAB)), et.fill_(i32(PAT_TILE))
        if len(E["si"]):
            es.view(-1)[dev(E["si"])] = dev(to32(E["sv"]))
            et.view(-1)[dev(E["ti"])] = dev(to32(E["tv"]))
        got_cnt = S.cnt.cpu().numpy().view(np.uint32)
        got_cmx = S.cmx.cpu().numpy()
        live = self.nqk * self.nwg * 4              # [query][workgroup][quarter]
        what = (nq, cap, mask is not None)
        bad = np.argwhere(got_cnt[:live].reshape(self.nqk, self.nwg, 4) != E["cnt"])
        assert bad.size == 0, ("counts (query, workgroup, quarter)", what, bad[:5].tolist())
        bad = np.argwhere(got_cmx[:live].reshape(self.nqk, self.nwg, 4) != E["cmx"])
        assert bad.size == 0, ("maxima (query, workgroup, quarter)", what, bad[:5].tolist())
        assert np.all(got_cnt[live:] == PAT_CNT) and np.all(got_cmx[live:].view(np.uint32) == PAT_CNT), \
            "counts / maxima written past the launch's queries"
        if not torch.equal(S.tile, et):
            bad = torch.nonzero(S.tile != et)[:5].cpu().tolist()
            raise AssertionError(("tile words (workgroup, query, slot)", what, bad))
        if not torch.equal(S.slabs, es):
            bad = torch.nonzero(S.slabs != es)[:5].cpu().tolist()
            raise AssertionError(("slabs (workgroup, query, slot, entry)", what, bad))
        return S, E, allow, bd

    def check_select(self, S, bd, nq, k, allow=None):
        """The int8 select on the pass's buffers returns the reference pass's keys."""
        kp, torch = self.kp, self.torch
        qs = copy.copy(self.qs)
        qs.nq = nq
        ref, _ = St.ref_pass(kp, torch, self.coll, qs, k, allow=allow)
        kth = St.key_scores(ref[:, k - 1])
        b = bd[:nq].cpu().numpy()
        assert np.all(ref[:, k - 1] != 0) and np.all(kth >= b + 0.05), "the case's bounds admit fewer than k rows"
        keys = St.q8_select(kp, torch, self.coll, qs, S, k, bd, allow=allow)
        bad = np.argwhere(keys != ref)
        assert bad.size == 0, ("select keys differ from the reference pass (query, rank)", bad[:5].tolist())

    def events_in(self, E, wg, wave):
        """The admitted lanes a tile of (workgroup wg, wave) -> {tile: [(group, query, kq)]}."""
        out = {}
        for t, kq, q in E["ev"]:
            if (t * 32) // self.rpw == wg and q // self.qpw == wave:
                out.setdefault(t - wg * T, []).append(((q % self.qpw) // 16, q, kq))
        return out


_ENVS = {}


@pytest.fixture(scope="module")
def env(kp, torch_):
    def get(dim):
        if dim not in _ENVS:
            _ENVS[dim] = Env(kp, torch_, dim)
        return _ENVS[dim]
    yield get
    _ENVS.clear()


def _bounds(e, on, level=0.12):
    b = np.full(e.nqk, OFF, np.float32)
    b[np.array(list(on), np.int64)] = level
    return b


@pytest.mark.parametrize("dim", DIMS)
def test_staging_boundary_sweep(env, dim):
    """P = 1 .. 130 slabs admitted by one wave, each (query, tile) pair one
    lane's: the stage empty, one short of full, full, one over, flushed twice,
    whatever its capacity up to 64; the rest leaves by the final flush."""
    e = env(dim)
    for P in range(1, 131):
        b = np.full(e.nqk, OFF, np.float32)
        full, part = divmod(P, T)
        b[np.array(e.sweep_q[:full], np.int64)] = 0.1                              # every tile's row
        if part:
            b[e.sweep_q[full]] = LEVELS[part - 1] - 0.05       # the first `part` tiles' rows
        S, E, _, _ = e.run(b, e.nqk)
        assert len(E["ev"]) == P and E["cnt"].sum() == P
        ev = e.events_in(E, WG_SWEEP, 3)
        assert sum(len(v) for v in ev.values()) == P, "the sweep's slabs are one wave's"


@pytest.mark.parametrize("dim", DIMS)
def test_oversized_event_behind_partly_filled_stage(env, dim):
    """Three single admissions, then a tile in which all 64 lanes of group 0
    pass (flush, then the direct stores), singles again, then all 64 lanes of
    the wave's last group: nothing lost, nothing twice."""
    e = env(dim)
    S, E, _, bd = e.run(_bounds(e, range(e.qpw)), e.qpw)
    ev = e.events_in(E, WG_BIG, 0)
    assert [len(ev[t]) for t in range(5)] == [3, 64, 1, 64, 1], ev
    assert {g for g, _, _ in ev[1]} == {0} and {g for g, _, _ in ev[3]} == {e.qpw // 16 - 1}
    e.check_select(S, bd, e.qpw, 2)


@pytest.mark.parametrize("dim", DIMS)
def test_both_groups_admit_in_one_tile(env, dim):
    """Queries 0 and 16 admit in the same tile (at 768-d the wave's two
    groups, under its one branch), then query 17 alone, then query 1 alone."""
    e = env(dim)
    S, E, _, _ = e.run(_bounds(e, range(32)), 32)
    by_tile = {}
    for t, kq, q in E["ev"]:
        if (t * 32) // e.rpw == WG_GROUPS:
            by_tile.setdefault(t - WG_GROUPS * T, []).append(q)
    assert {t: sorted(v) for t, v in by_tile.items()} == {0: [0, 16], 1: [17], 2: [1]}
    if dim == 768:  # one wave, its two groups
        ev = e.events_in(E, WG_GROUPS, 0)
        assert sorted(g for g, _, _ in ev[0]) == [0, 1] and [g for g, _, _ in ev[1]] == [1]


@pytest.mark.parametrize("dim", DIMS)
def test_lossy_quarter_keeps_the_first_slabs(env, dim):
    """Four slabs a quarter, seven admitted in one: the count runs on to 7,
    the first four are stored, the maximum is the sixth's; the neighbouring
    quarter's slots hold its one slab and the pattern."""
    e = env(dim)
    S, E, _, bd = e.run(_bounds(e, range(3)), 3, cap=16)
    assert E["cnt"][0, WG_LOSSY].tolist() == [7, 1, 0, 0]
    t5 = WG_LOSSY * T + 5
    assert E["cmx"][0, WG_LOSSY, 0] == e.dots[t5 * 32, 0] > E["cmx"][0, WG_LOSSY, 1]
    tl = S.tile[WG_LOSSY, 0].cpu().numpy().view(np.uint32)
    t0 = ROW_BASE + WG_LOSSY * T * 32
    assert tl[:4].tolist() == [t0, t0 + 32, t0 + 64, t0 + 96]
    assert tl[4:].tolist() == [t0 + 64] + [PAT_TILE] * 11
    e.check_select(S, bd, 3, 2)


@pytest.mark.parametrize("dim", DIMS)
def test_ragged_last_tile_and_short_last_workgroup(env, dim):
    """The last workgroup has two tiles fewer and 25 live rows in its last
    tile; rows planted there are admitted with the padding rows INT_MIN."""
    e = env(dim)
    S, E, _, bd = e.run(_bounds(e, range(e.qpw)), e.qpw)
    last = e.nwg - 1
    ev = e.events_in(E, last, 0)
    assert sorted((q, kq) for _, q, kq in ev[T - 3]) == [(0, 2), (7, 0), (8, 0)] and \
        [(q, kq) for _, q, kq in ev[T - 4]] == [(7, 3)]
    sl = S.slabs[last, 0, 2 * T].cpu().numpy()       # query 0, quarter 2, first slot
    assert sl[4] == e.dots[e.n - 1, 0] and np.all(sl[5:] == INT_MIN) and np.all(sl[:4] > INT_MIN)
    e.check_select(S, bd, e.qpw, 2)


@pytest.mark.parametrize("dim", DIMS)
def test_filtered_rows(env, dim):
    """A planted row the filter hides does not admit its slab; beside a live
    planted row of its quarter it is INT_MIN in the slab. One row in 16 is
    hidden elsewhere, and every tile runs the masking body."""
    e = env(dim)
    rng = np.random.default_rng(7)
    mask = rng.random(e.n) >= 1 / 16
    planted = np.abs(e.X).max(1) > 0.02
    mask[planted] = True
    mask[e.masked] = False
    S, E, allow, bd = e.run(_bounds(e, range(e.qpw)), e.qpw, mask=mask)
    ev = e.events_in(E, WG_FILTER, 0)
    assert 0 not in ev and [(q, kq) for _, q, kq in ev[1]] == [(6, 0)]
    sl = S.slabs[WG_FILTER, 6, 0].cpu().numpy()
    r = e.row(WG_FILTER, 1, 0)
    assert sl[1] == INT_MIN and sl[2] == e.dots[r + 2, 6] and e.dots[r + 1, 6] > e.dots[r + 2, 6]
    last = e.events_in(E, e.nwg - 1, 0)
    assert sorted(q for _, q, _ in last[T - 3]) == [0, 7]     # query 8's row is hidden
    e.check_select(S, bd, e.qpw, 2, allow=allow)


@pytest.mark.parametrize("nq", [5, 33])
@pytest.mark.parametrize("dim", DIMS)
def test_invalid_queries_append_nothing(env, dim, nq):
    """Bounds that would admit rows of 48 queries, nq_valid = 5 and 33: the
    queries past it append nothing and their slots keep the pattern."""
    e = env(dim)
    S, E, _, _ = e.run(_bounds(e, range(48)), nq)
    qs = {q for _, _, q in E["ev"]}
    assert qs == set(range(nq))
    assert E["cnt"][nq:].sum() == 0 and np.all(E["cmx"][nq:] == INT_MIN)
    i32 = PAT_SLAB - (1 << 32) if PAT_SLAB >= 1 << 31 else PAT_SLAB
    assert bool((S.slabs[:, nq:] == i32).all())
