"""(GPU) Every link of the int8 prefilter's proof chain under a test of its
own (DESIGN.md §5 "int8 prefilter"): the launchers themselves, through
tests/kprobe, on the adversarial rows and queries of tests/q8_ref.py, at the
smallest shapes where each can go wrong, against integer or fp64 references.

  store side   launch_q8_absmax / set_scale / quantize: S, every x8 byte, the
               tile norms dt / nt (sound, and no looser than q8_norm_up's two
               roundings), glob's maxima, the tile-list form with a stale S
  query side   launch_q8_query (plain, speculative), launch_sample_bound_q8,
               launch_q8_prep_query: bit-identical images, par within bounds
  int8 pass    no bound: every live row in exactly one admitted slab, every
               value the exact integer dot; with a bound: every row whose U
               reaches b - sigma nmax admitted
  bracket      L <= s <= U on the device's own x8 / meta / par for the fp64
               score and the device's fp32 score of every row
  pipeline     int8 pass + select with bounds the test chooses: the keys are
               the bf16 / f32 pass's, bit for bit; ties; filters

Tolerances. A norm t (fp64) is stored as RU_float(sqrt(sum) (1 + 2^-30))
(vs_bound_dev.h q8_norm_up): never under t (the device's fp64 sum differs
from the reference's by < dim 2^-53 relative, far inside the 2^-30 margin),
and at most t (1 + 2^-30)(1 + 2^-23) < t (1 + 2^-22) (one float ulp is at most
2^-23 relative). Row counts come from mfma_grid (it depends on the CU count).
"""
import numpy as np
import pytest

import q8_ref as R
import q8_stage as St

pytestmark = pytest.mark.gpu

SLACK = R.NORM_SLACK
DT = [pytest.param(False, id="bf16"), pytest.param(True, id="f32")]
# the shapes with an int8 pass (q8_supported), each with the row kinds of its storage dtype
BR = [(768, False), (1024, False), (768, True)]
KIND_BR = [pytest.param(k, d, f, id=f"{k}-{'f32' if f else 'bf16'}-{d}")
           for d, f in BR for k in R.row_kinds(f)]
BR = [pytest.param(d, f, id=f"{'f32' if f else 'bf16'}-{d}") for d, f in BR]


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def shapes(kp):
    return St.interesting_rows(kp)


def _queries(X, f32, nq, seed=0):
    """nq queries: one of every kind of q8_ref first (the +-amax one first of
    all), then unit-norm ones."""
    kinds = ("pm_amax",) + tuple(k for k in R.QUERY_KINDS if k != "pm_amax")
    Q, _ = R.make_queries(X, f32, seed, kinds)
    if nq > len(Q):
        rng = np.random.default_rng(900 + seed)
        extra = R._unit(rng, nq - len(Q), X.shape[1])
        Q = np.concatenate([Q, extra if f32 else R._bf16(extra)])
    return np.ascontiguousarray(Q[:nq], np.float32), kinds


# ---------------------------------------------------------------------------
# store side
# ---------------------------------------------------------------------------
def _check_tiles(X, n, S, x8, meta, tiles, what):
    """x8 bytes and {dt, nt} of the given tiles against the reference with scale S."""
    X8, dn, xn = R.row_norms(X, S)
    for t in tiles:
        lo, hi = 32 * t, min(32 * t + 32, n)
        assert np.array_equal(x8[lo:hi].astype(np.int32), X8[lo:hi]), (what, "x8 of tile", t)
        assert not x8[hi:32 * t + 32].any(), (what, "rows past n_rows must be zero bytes", t)
        for col, v in ((0, dn), (1, xn)):
            want = v[lo:hi].max()  # live rows only
            got = np.float64(meta[t, col])
            # lower side: soundness (mutations: q8_norm_up rounding down, the
            # last live row skipped); upper side: q8_norm_up's two roundings
            # (mutation: dead rows folded in)
            assert want <= got <= want * SLACK, (what, "tile", t, "dt" if col == 0 else "nt", got, want)
    assert x8.min() >= -127, (what, "-128 stored")


def _store_case(kp, torch, kind, n, dim, f32):
    X, X0 = R.make_rows(kind, n, dim, f32)
    coll = St.Collection(kp, torch, X, f32, X0=X0 if kind == "clipped" else None, poison_pad=True)
    x8, meta, glob = coll.read()
    amax = np.float32(np.abs(X0).max())
    assert glob[0].view(np.uint32) == amax.view(np.uint32), ("absmax", glob[0], amax)
    S = np.float32(amax / np.float32(127))
    assert glob[3].view(np.uint32) == S.view(np.uint32), ("S", glob[3], S)
    assert S == R.scale_of(X0)
    _check_tiles(X, n, S, x8, meta, range(coll.tiles), (kind, n, dim, f32))
    # mutation: atomic_max_pos(glob + 1, dt) removed
    assert glob[1] == meta[:, 0].max() and glob[2] == meta[:, 1].max(), (glob, meta.max(0))
    return coll, X8_of(x8, n)


def X8_of(x8, n):
    return x8[:n].astype(np.int32)


@pytest.mark.parametrize("f32", DT)
@pytest.mark.parametrize("dim", [128, 768, 1024, 2048])
@pytest.mark.parametrize("shape", ["a", "b", "few", "c"])
def test_store_side_shapes(kp, torch_, shapes, shape, dim, f32):
    """Rows written after the scale was fixed (clipping), at every row count;
    the largest row is the last live one of a ragged tile at 5 rows, and the
    dead rows of the last tile hold large values on the device.
    Mutations: q8_norm_up rounding down (__double2float_rd); q8_quantize_kernel
    reading dead rows or skipping a tile's last live row; the raise of glob[1]
    removed."""
    _store_case(kp, torch_, "clipped", shapes[shape], dim, f32)


@pytest.mark.parametrize("kind,f32", [pytest.param(k, f, id=f"{k}-{'f32' if f else 'bf16'}")
                                      for f in (False, True) for k in R.row_kinds(f) if k != "clipped"])
def test_store_side_row_kinds(kp, torch_, kind, f32):
    n = 101
    coll, X8 = _store_case(kp, torch_, kind, n, 768, f32)
    if kind == "pm_absmax":
        assert np.all(np.abs(X8) == 127)
    if kind == "tiny":
        assert not X8[1::2].any()
    if kind == "halfway":
        assert np.all(X8.ravel()[1:] % 2 == 0), "half-way points round to even"


@pytest.mark.parametrize("f32", DT)
def test_store_side_all_zero_collection(kp, torch_, f32):
    coll = St.Collection(kp, torch_, np.zeros((37, 256), np.float32), f32, poison_pad=True)
    x8, meta, glob = coll.read()
    assert glob[0] == 0 and glob[3] == 1.0, glob  # S = 1
    assert not x8.any() and not meta.any() and glob[1] == 0 and glob[2] == 0


@pytest.mark.parametrize("f32", DT)
@pytest.mark.parametrize("dim", [128, 768])
def test_store_side_tile_list(kp, torch_, dim, f32):
    """launch_q8_quantize with a tile list and a stale S: only those tiles'
    X8 / meta change, they obey the bounds (clipped), glob[1..2] only rise."""
    n = 32 * 9 + 7
    X, _ = R.make_rows("unit", n, dim, f32)
    coll = St.Collection(kp, torch_, X, f32, poison_pad=True)
    x8_0, meta_0, glob_0 = coll.read()
    S = glob_0[3]
    last = coll.tiles - 1
    tiles = [3, 0, last]
    rows = np.concatenate([np.arange(32 * t, min(32 * t + 32, n)) for t in tiles])
    rng = np.random.default_rng(5)
    new = rng.uniform(-4, 4, (len(rows), dim)) * np.float64(glob_0[0])  # up to 4 x absmax
    new = np.ascontiguousarray(new, np.float32) if f32 else R._bf16(new.astype(np.float32))
    X2 = X.copy()
    X2[rows] = new
    coll.upload(new, rows)
    coll.quantize(tiles)
    x8, meta, glob = coll.read()
    assert glob[0].view(np.uint32) == glob_0[0].view(np.uint32) and glob[3].view(np.uint32) == S.view(np.uint32)
    others = [t for t in range(coll.tiles) if t not in tiles]
    keep = np.concatenate([np.arange(32 * t, 32 * t + 32) for t in others])
    assert np.array_equal(x8[keep], x8_0[keep]), "a tile outside the list changed"
    assert np.array_equal(meta[others].view(np.uint32), meta_0[others].view(np.uint32))
    _check_tiles(X2, n, S, x8, meta, tiles, ("tile list", dim, f32))
    assert np.abs(x8[rows]).max() == 127, "the new rows clip"
    assert meta[tiles, 0].min() > glob_0[1], "clipped rows have a larger error than any before"
    # mutation: atomic_max_pos(glob + 1, dt) removed
    assert glob[1] >= meta[:, 0].max() and glob[2] >= meta[:, 1].max(), (glob, meta.max(0))
    assert glob[1] >= glob_0[1] and glob[2] >= glob_0[2]


# ---------------------------------------------------------------------------
# query side
# ---------------------------------------------------------------------------
def _check_query_side(Q, S, q8, par, dim, what):
    for i, q in enumerate(Q):
        r = R.query_ref(q, S)
        assert np.array_equal(q8[i].astype(np.int32), r["q8"]), (what, i, "q8")
        assert par[i, 0].view(np.uint32) == r["sqS"].view(np.uint32), (what, i, "sqS", par[i, 0], r["sqS"])
        for col, t in ((1, r["an"]), (2, r["cn"])):
            assert t <= np.float64(par[i, col]) <= t * SLACK, (what, i, col, par[i, col], t)
        # sigma = float((4 dim + 64) 2^-24 |q|_up (1 + 2^-20)), |q| <= |q|_up <= |q| (1 + 2^-22):
        # the last conversion rounds to nearest, within (1 +- 2^-24), which the
        # factor (1 + 2^-20) below and the slack of 2^-22 above absorb
        lo = (4.0 * dim + 64.0) * 2.0 ** -24 * r["qn"]
        assert lo <= np.float64(par[i, 3]) <= lo * (1 + 2.0 ** -20) * (1 + 2.0 ** -22), (what, i, "sigma")
        if not q.any():
            assert par[i, 0] == 0 and not q8[i].any() and not par[i, 1:].any(), (what, i, "zero query")


QSIDE = [(768, 1), (768, 5), (768, 64), (768, 256), (1024, 128), (128, 5), (2048, 5)]


@pytest.mark.parametrize("f32", DT)
@pytest.mark.parametrize("dim,nq", QSIDE)
def test_query_side(kp, torch_, dim, nq, f32):
    X, _ = R.make_rows("unit", 64, dim, f32)
    coll = St.Collection(kp, torch_, X, f32)
    S = coll.read()[2][3]
    Q, _ = _queries(X, f32, nq)
    qs = St.Queries(kp, torch_, Q, f32).quantize(coll)
    q8, par, gate = qs.read()
    _check_query_side(Q, S, q8, par, dim, (dim, nq, f32))
    assert gate[kp.gate_verdict] == 0, "the plain form zeroes the verdict word"
    q8_all = qs.q8.cpu().numpy()
    assert np.all(q8_all[nq:] == 0x55) and np.all(qs.par[4 * nq:4 * 256].cpu().numpy() == -7.0), "wrote past nq"
    # the fused sample-bound launch's query half: the same bits
    qs2 = St.Queries(kp, torch_, Q, f32)
    tmax = torch_.zeros(256 * 4, device=St.DEV)
    bound = torch_.zeros(256, device=St.DEV)
    kp.check(kp.sample_bound_q8(tmax.data_ptr(), 4, 2, 1, bound.data_ptr(), qs2.Qd.data_ptr(), int(f32), nq, dim,
                                coll.glob.data_ptr(), qs2.q8.data_ptr(), qs2.par.data_ptr(), qs2.gate.data_ptr()))
    q8b, parb, gateb = qs2.read()
    assert np.array_equal(q8b, q8) and np.array_equal(parb.view(np.uint32), par.view(np.uint32))
    assert gateb[kp.gate_verdict] == 0


class Spec:
    """One k's speculative state inside a collection's glob allocation."""

    def __init__(self, kp, torch, coll, kslot=10):
        self.kp, self.torch, self.coll = kp, torch, coll
        self.off = kp.q8_spec_k_off + kslot * kp.q8_spec_k_size
        self.k_ptr = coll.glob.data_ptr() + self.off
        self.stat_ptr = coll.glob.data_ptr() + kp.q8_spec_stat_off
        self.ratio_ptr = self.k_ptr + kp.spec_k_ratio_off
        self.bound = torch.full((256,), 99.0, dtype=torch.float32, device=St.DEV)

    def _w(self, off, dt):
        return self.coll.glob[off:off + 4].view(dt)

    def set(self, ratio=None, loose=None, since=None):
        t, kp = self.torch, self.kp
        if ratio is not None:
            self._w(self.off + kp.spec_k_ratio_off, t.float32)[0] = float(ratio)
        if loose is not None:
            self._w(self.off + kp.spec_k_loose_off, t.int32)[0] = loose
        if since is not None:
            self._w(self.off + kp.spec_k_since_off, t.int32)[0] = since

    def stat(self):
        kp = self.kp
        g = self.coll.glob.cpu().numpy()
        o = kp.q8_spec_stat_off
        rd = lambda off: int(g[off:off + 8].view(np.uint64)[0])
        return dict(tries=rd(o + kp.spec_stat_tries_off), fails=rd(o + kp.spec_stat_fails_off),
                    skipped=rd(o + kp.spec_stat_skipped_off),
                    since=int(g[self.off + kp.spec_k_since_off:][:4].view(np.uint32)[0]))

    def query(self, qs, force=False):
        kp = self.kp
        kp.check(kp.q8_query_spec(qs.Qd.data_ptr(), int(qs.f32), qs.nq, qs.dim, self.coll.glob.data_ptr(),
                                  qs.q8.data_ptr(), qs.par.data_ptr(), qs.gate.data_ptr(), self.ratio_ptr,
                                  self.bound.data_ptr(), self.k_ptr, self.stat_ptr, int(force)))
        self.torch.cuda.synchronize()
        g = qs.gate.cpu().numpy()
        return int(g[kp.gate_go]), int(g[kp.gate_verdict]), self.bound.cpu().numpy()[:qs.nq]


@pytest.mark.parametrize("f32", DT)
def test_query_side_speculative_form(kp, torch_, f32):
    dim, nq = 768, 17
    X, _ = R.make_rows("unit", 64, dim, f32)
    coll = St.Collection(kp, torch_, X, f32)
    Q, _ = _queries(X, f32, nq)
    plain = St.Queries(kp, torch_, Q, f32).quantize(coll).read()
    qs = St.Queries(kp, torch_, Q, f32)
    sp = Spec(kp, torch_, coll)
    # ratio unset: every bound -inf, the batch stands down and is counted
    go, verdict, b = sp.query(qs)
    assert (go, verdict) == (0, 1) and np.all(b == -np.inf)
    assert sp.stat() == dict(tries=0, fails=0, skipped=1, since=0)
    # ratio set: bound = float(ratio * float(sqrt(nn))), the images unchanged
    ratio = np.float32(0.3125 + 2.0 ** -20)
    sp.set(ratio=ratio)
    go, verdict, b = sp.query(qs)
    assert (go, verdict) == (1, 0)
    q8, par, _ = qs.read()
    assert np.array_equal(q8, plain[0]) and np.array_equal(par.view(np.uint32), plain[1].view(np.uint32))
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(1))
    want = (np.float64(ratio) * qn).astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(np.abs(b.astype(np.float64) - want) <= 2 * ulp), (b, want)  # two fp32 roundings
    assert sp.stat()["tries"] == 1 and sp.stat()["since"] == 1
    # loose: stands down unless forced
    sp.set(loose=1)
    assert sp.query(qs)[:2] == (0, 1)
    assert sp.query(qs, force=True)[:2] == (1, 0)
    sp.set(loose=0, since=0)
    st0 = sp.stat()
    # every kQ8SpecProbe-th consecutive try stands down (the sample path probes)
    probe = kp.q8_spec_probe
    for i in range(1, probe + 1):
        go, verdict, _ = sp.query(qs)
        assert (go, verdict) == ((1, 0) if i < probe else (0, 1)), i
    st1 = sp.stat()
    assert st1["tries"] - st0["tries"] == probe - 1 and st1["skipped"] - st0["skipped"] == 1


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("f32", DT)
@pytest.mark.parametrize("dim,nq", [(768, 17), (1024, 128), (128, 5)])
def test_prep_query_matches_the_two_launches(kp, torch_, dim, nq, f32, cosine):
    """launch_q8_prep_query = launch_query_prep + the speculative launch_q8_query, bit for bit."""
    X, _ = R.make_rows("unit", 64, dim, True)
    coll = St.Collection(kp, torch_, X if f32 else R._bf16(X), f32)
    raw, _ = _queries(X, True, nq)  # raw fp32 queries, unrounded
    raw_d = torch_.from_numpy(raw).to(St.DEV)
    round_qp = not f32
    outs = []
    for fused in (False, True):
        qp = torch_.full((256, dim), 5.0, dtype=torch_.float32, device=St.DEV)
        qb = torch_.full((256, dim), 5, dtype=torch_.int16, device=St.DEV)
        qs = St.Queries(kp, torch_, np.zeros((nq, dim), np.float32), f32)
        sp = Spec(kp, torch_, coll, kslot=20 + fused)
        sp.set(ratio=0.25)
        if fused:
            kp.check(kp.q8_prep_query(raw_d.data_ptr(), int(cosine), int(round_qp), qp.data_ptr(), qb.data_ptr(),
                                      int(f32), nq, dim, coll.glob.data_ptr(), qs.q8.data_ptr(),
                                      qs.par.data_ptr(), qs.gate.data_ptr(), sp.ratio_ptr, sp.bound.data_ptr(),
                                      sp.k_ptr, sp.stat_ptr, 0))
        else:
            kp.check(kp.query_prep(raw_d.data_ptr(), nq, dim, int(cosine), int(round_qp), qp.data_ptr(),
                                   qb.data_ptr()))
            src = qp if f32 else qb
            kp.check(kp.q8_query_spec(src.data_ptr(), int(f32), nq, dim, coll.glob.data_ptr(), qs.q8.data_ptr(),
                                      qs.par.data_ptr(), qs.gate.data_ptr(), sp.ratio_ptr, sp.bound.data_ptr(),
                                      sp.k_ptr, sp.stat_ptr, 0))
        q8, par, gate = qs.read()
        outs.append((qp.cpu().numpy().view(np.uint32), qb.cpu().numpy(), q8, par.view(np.uint32),
                     sp.bound.cpu().numpy().view(np.uint32), gate[:3].copy()))
    for name, a, b in zip(("qp", "qbf", "q8", "q8par", "bound", "gate"), outs[0], outs[1]):
        assert np.array_equal(a, b), name
    # and the images are the reference's for the prepared queries
    qprep = outs[0][0].view(np.float32)[:nq] if f32 else \
        (outs[0][1][:nq].view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    _check_query_side(qprep, coll.read()[2][3], outs[0][2], outs[0][3].view(np.float32), dim, "prep")


# ---------------------------------------------------------------------------
# int8 pass
# ---------------------------------------------------------------------------
def _exact_dots(X8, Q8):
    """X8 @ Q8^T as int64: |dot| <= 127^2 dim < 2^24, so the float64 product is exact."""
    return (X8.astype(np.float64) @ Q8.astype(np.float64).T).astype(np.int64)


I8_CASES = ([(768, s, "unit", rb) for s, rb in (("a", 0), ("b", 0), ("few", 0), ("c", 0), ("c", 3 * 4096))] +
            [(1024, s, "unit", rb) for s, rb in (("a", 0), ("b", 0), ("few", 0), ("c", 0), ("c", 3 * 4096))] +
            [(768, "few", "pm_absmax", 0), (1024, "few", "pm_absmax", 0), (768, "few", "zero_rows", 0)])


@pytest.mark.parametrize("dim,shape,kind,row_base", I8_CASES)
def test_int8_pass_covers_every_row_exactly(kp, torch_, shapes, dim, shape, kind, row_base):
    """No bound (init_score null): for every query every live row sits in exactly
    one admitted slab (what a ragged-tail bug breaks), and every slab value is
    the exact integer dot; padding rows of an admitted slab are INT_MIN."""
    n = shapes[shape]
    X, _ = R.make_rows(kind, n, dim, False)
    coll = St.Collection(kp, torch_, X, False, row_base=row_base)
    X8 = coll.read()[0][:n].astype(np.int32)
    full = kp.mfma_queries(dim, 0)
    assert full == (256 if dim == 768 else 128)
    Qall, _ = _queries(X, False, full)
    cap = St.cap_for(kp, n)
    for nq in (1, 17, full):
        qs = St.Queries(kp, torch_, Qall[:nq], False).quantize(coll)
        Q8 = qs.read()[0].astype(np.int32)
        S = St.q8_pass(kp, torch_, coll, qs, 10, bound=None, cap=cap)
        qq, rows, vals = S.decode(nq, i8=True)
        local = rows - row_base
        assert local.min() >= 0 and local.max() < coll.pad, "a slab outside the collection"
        live = local < n
        seen = np.zeros((nq, n), np.int64)
        np.add.at(seen, (qq[live], local[live]), 1)
        assert seen.min() == 1 and seen.max() == 1, (
            "rows missed / repeated", nq, np.argwhere(seen != 1)[:5].tolist())
        dots = _exact_dots(X8, Q8)  # [n, nq]
        got = np.zeros((nq, n), np.int64)
        got[qq[live], local[live]] = vals[live]
        bad = np.argwhere(got != dots.T)
        assert bad.size == 0, ("dot mismatch (query, row)", bad[:5].tolist())
        assert np.all(vals[~live] == St.INT_MIN), "padding rows of a slab are INT_MIN"
        if kind == "pm_absmax" and nq == 1:  # the +-amax query against the all-plus row
            assert abs(int(got[0, 0])) == 127 * 127 * dim


# ---------------------------------------------------------------------------
# bracket on the device's own quantities
# ---------------------------------------------------------------------------
def _row_scores(kp, torch, coll, qs):
    """The bf16 / f32 pass's own fp32 score of every row (k = 128, -inf bound),
    read from its slabs -> [nq, n]."""
    _, S = St.ref_pass(kp, torch, coll, qs, 128, select=False)
    qq, rows, vals = S.decode(qs.nq, i8=False)
    local = rows - coll.row_base
    live = (local >= 0) & (local < coll.n)
    seen = np.zeros((qs.nq, coll.n), np.int64)
    np.add.at(seen, (qq[live], local[live]), 1)
    assert seen.min() == 1 and seen.max() == 1, "the reference pass did not hold every row once"
    s = np.zeros((qs.nq, coll.n), np.float32)
    s[qq[live], local[live]] = vals[live]
    return s


@pytest.mark.parametrize("kind,dim,f32", KIND_BR)
def test_bracket_and_admission_on_device_quantities(kp, torch_, kind, dim, f32):
    assert kp.q8_supported(dim, int(f32))
    n = 101
    X, X0 = R.make_rows(kind, n, dim, f32)
    coll = St.Collection(kp, torch_, X, f32, X0=X0 if kind == "clipped" else None)
    x8, meta, glob = coll.read()
    X8 = x8[:n].astype(np.int32)
    Q, kinds = _queries(X, f32, len(R.QUERY_KINDS))
    qs = St.Queries(kp, torch_, Q, f32).quantize(coll)
    q8, par, _ = qs.read()
    dots = _exact_dots(X8, q8.astype(np.int32)).T  # [nq, n]
    s_dev = _row_scores(kp, torch_, coll, qs)
    s64 = Q.astype(np.float64) @ X.astype(np.float64).T
    tile = np.arange(n) // 32
    f = np.float32
    dmax, nmax = glob[1], glob[2]
    for i, qk in enumerate(kinds):
        L, U = R.bracket(dots[i], par[i, 0], par[i, 1], par[i, 2], par[i, 3], meta[tile, 0], meta[tile, 1])
        for name, s in (("fp64", s64[i]), ("device fp32", s_dev[i])):
            assert np.all(L <= s) and np.all(s <= U), (kind, qk, name, np.argwhere((L > s) | (s > U))[:3].tolist())
        # (sigma's own premise: an fp32 score is within 2 dim 2^-24 |q| |x| < sigma nmax of exact)
        assert np.all(np.abs(s_dev[i].astype(np.float64) - s64[i]) <=
                      np.float64(par[i, 3]) * np.float64(nmax)), (kind, qk, "a score further than sigma nmax off")
        if not par[i, 0] > 0:
            continue
        # the pass's integer threshold (q8_dot_threshold) in numpy fp32, for a
        # bound equal to any row's own fp32 score: that row is admitted
        b = s_dev[i]
        t = ((b - par[i, 1] * dmax - (par[i, 2] + f(2) * par[i, 3]) * nmax) / par[i, 0] - f(1)).astype(f)
        assert t.dtype == np.float32
        assert np.all(dots[i] >= np.floor(t.astype(np.float64))), (kind, qk, "admission")
    # On the device (bf16 rows: the int8 pass's own dtype switch is the select's).
    # Contract (vs_kernels.hip q8_dot_threshold): a row whose U on the global
    # terms, sqS dot + a dmax + (c + sigma) nmax, reaches b - sigma nmax is
    # admitted. Per query the row of the largest dot, with b half a sigma nmax
    # above its U: inside the window, with 0.5 sigma nmax >= 1500 2^-24 |q| nmax
    # to spare against the threshold's own half dozen fp32 roundings.
    # Mutation: 2.f * p[3] -> p[3] and the - 1.f dropped.
    top = dots.argmax(1)
    p = par.astype(np.float64)
    Ug = p[:, 0] * dots[np.arange(len(Q)), top] + p[:, 1] * np.float64(dmax) + (p[:, 2] + p[:, 3]) * np.float64(nmax)
    b = (Ug + 0.5 * p[:, 3] * np.float64(nmax)).astype(np.float32)
    bd = St.neg_inf(torch_)
    bd[:len(Q)] = torch_.from_numpy(b).to(St.DEV)
    S = St.q8_pass(kp, torch_, coll, qs, 10, bound=bd)
    qq, rows, vals = S.decode(len(Q), i8=True)
    for i, qk in enumerate(kinds):
        assert np.any((qq == i) & (rows == top[i])), (kind, qk, "a row whose U reaches b - sigma nmax was cut")


# ---------------------------------------------------------------------------
# pipeline with bounds the test chooses
# ---------------------------------------------------------------------------
KS = [1, 10, 64, 65, 128]


def _pipeline_bounds(ref_keys, par, glob, k):
    """-inf, s_k, the float under s_k, s_k - sigma nmax (fp32), per query."""
    nq = len(ref_keys)
    kth = ref_keys[:, k - 1]
    sk = np.where(kth != 0, St.key_scores(kth), np.float32(-np.inf)).astype(np.float32)
    return {
        "-inf": np.full(nq, -np.inf, np.float32),
        "s_k": sk,
        "under s_k": np.nextafter(sk, np.float32(-np.inf)),
        "s_k - sigma nmax": (sk - par[:, 3] * glob[2]).astype(np.float32),
    }


def _run_pipeline(kp, torch, coll, qs, ks, allow=None, mask=None):
    _, par, _ = qs.read()
    glob = coll.read()[2]
    for k in ks:
        ref, _ = St.ref_pass(kp, torch, coll, qs, k, allow=allow)
        if mask is not None:
            rows = St.key_rows(ref) - coll.row_base
            nz = ref != 0
            assert np.all(mask[rows[nz]]), "the reference returned a masked row"
            keep = min(k, int(mask.sum()))
            assert np.all(nz[:, :keep]) and not np.any(nz[:, keep:]), "the tail must be zero keys"
        for name, b in _pipeline_bounds(ref, par, glob, k).items():
            bd = St.neg_inf(torch)
            bd[:qs.nq] = torch.from_numpy(b).to(St.DEV)
            S = St.q8_pass(kp, torch, coll, qs, k, bound=bd, allow=allow)
            keys = St.q8_select(kp, torch, coll, qs, S, k, bd, allow=allow)
            bad = np.argwhere(keys != ref)
            assert bad.size == 0, ("keys differ from the reference pass", "k", k, "bound", name,
                                   "(query, rank)", bad[:5].tolist())
    return ref


@pytest.mark.parametrize("kind,dim,f32", KIND_BR)
def test_pipeline_keys_equal_the_reference_pass(kp, torch_, kind, dim, f32):
    n = 333
    X, X0 = R.make_rows(kind, n, dim, f32)
    coll = St.Collection(kp, torch_, X, f32, X0=X0 if kind == "clipped" else None)
    Q, _ = _queries(X, f32, 16)
    qs = St.Queries(kp, torch_, Q, f32).quantize(coll)
    _run_pipeline(kp, torch_, coll, qs, KS)


@pytest.mark.parametrize("row_base", [0, 3 * 4096])
def test_pipeline_several_workgroups(kp, torch_, shapes, row_base):
    n = shapes["c"]
    X, _ = R.make_rows("unit", n, 768, False)
    coll = St.Collection(kp, torch_, X, False, row_base=row_base)
    Q, _ = _queries(X, False, 16)
    qs = St.Queries(kp, torch_, Q, False).quantize(coll)
    ref = _run_pipeline(kp, torch_, coll, qs, [10, 65])
    rows = St.key_rows(ref)
    assert rows.min() >= row_base and rows.max() < row_base + n


@pytest.mark.parametrize("dim,f32", BR)
def test_pipeline_ties_break_by_ascending_row(kp, torch_, dim, f32):
    """Five vectors repeated: equal scores straddle every k-th place."""
    n = 333
    base, _ = R.make_rows("unit", 5, dim, f32)
    X = np.ascontiguousarray(base[np.arange(n) % 5])
    coll = St.Collection(kp, torch_, X, f32)
    Q, _ = _queries(X, f32, 16)
    qs = St.Queries(kp, torch_, Q, f32).quantize(coll)
    s_dev = _row_scores(kp, torch_, coll, qs)
    for k in KS:
        ref = _run_pipeline(kp, torch_, coll, qs, [k])
        for i in range(qs.nq):
            s = s_dev[i].copy()
            s[s == 0] = 0.0
            order = np.lexsort((np.arange(n), -s.astype(np.float64)))[:k]  # score descending, row ascending
            want = St.make_keys(s[order], order)
            assert np.array_equal(ref[i], want), ("ties", k, i)


@pytest.mark.parametrize("dim,f32", BR)
@pytest.mark.parametrize("density", ["half", "few"])
def test_pipeline_filtered(kp, torch_, dim, f32, density):
    n = 333
    X, _ = R.make_rows("unit", n, dim, f32)
    coll = St.Collection(kp, torch_, X, f32)
    Q, _ = _queries(X, f32, 16)
    qs = St.Queries(kp, torch_, Q, f32).quantize(coll)
    rng = np.random.default_rng(3)
    mask = rng.random(n) < 0.5
    if density == "few":  # fewer allowed rows than k
        mask[:] = False
        mask[[2, 31, 32, 100, 200, 301, 332]] = True
    allow = St._i64(torch_, St.pack_allow(mask, coll.pad // 64 + 2))
    s_dev = _row_scores(kp, torch_, coll, qs)
    for k in (10, 65):
        ref = _run_pipeline(kp, torch_, coll, qs, [k], allow=allow, mask=mask)
        for i in range(qs.nq):  # the masked reference itself, from the per-row scores
            s = s_dev[i].copy()
            s[s == 0] = 0.0
            idx = np.nonzero(mask)[0]
            order = idx[np.lexsort((idx, -s[idx].astype(np.float64)))][:k]
            want = np.zeros(k, np.uint64)
            want[:len(order)] = St.make_keys(s[order], order)
            assert np.array_equal(ref[i], want), ("filtered", k, i)
