"""(GPU) The speculative bound's check and record (csrc/vs_spec_dev.h
spec_query_vals / spec_verify_core) through launch_q8_verify_record, on keys,
bounds, sigmas and nmax the test writes, and the soundness implication on a
real pipeline: a verdict word of 0 means the keys are the reference pass's.

The end-to-end tests cannot reach either: the engine picks every bound there,
and a check that accepts a bound a hair too high (or a quantile off by one)
changes a key only when a true top-k row sits inside that sliver.

Synthetic part. A query's threshold is thr = b - sigma nmax in fp32; nmax = 2
here, so sigma nmax is exact and thr has one rounding whether or not the
compiler fuses the multiply. The recorded ratio is compared with
    0.97f x the (1 + nvalid / 64)-th smallest of s / |q|      (fp64)
over the queries with a non-zero k-th key, s > 0 and |q| > 0, within 2^-21
relative: sigma's rounding, the norm recovered from it, the quotient and the
product are one fp32 rounding (2^-24) each, and 0.97f is the code's constant.
Planted ratios are >= 1e-3 apart, so no rounding reorders them.
"""
import numpy as np
import pytest

import q8_ref as R
import q8_stage as St

pytestmark = pytest.mark.gpu

DIM = 768
K = 3
NMAX = np.float32(2.0)
RTOL = 2.0 ** -21
NQS = [1, 63, 64, 65, 256]


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sigma(qn):
    """q8_sigma(DIM, |q|) (vs_bound_dev.h)."""
    return np.asarray((4.0 * DIM + 64.0) * 2.0 ** -24 * np.asarray(qn, np.float64) * (1 + 2.0 ** -20)).astype(np.float32)


def _thr(b, sig):
    return np.asarray(np.asarray(b, np.float32) - np.asarray(sig, np.float32) * NMAX, np.float32)


class Batch:
    """One k's device state and one batch's inputs; run() is one launch."""

    def __init__(self, kp, torch, nq, kslot=K):
        self.kp, self.torch, self.nq = kp, torch, nq
        dev = "cuda:0"
        self.glob = torch.zeros(kp.q8_glob_bytes, dtype=torch.uint8, device=dev)
        self.glob[:16].view(torch.float32)[2] = float(NMAX)
        self.par = torch.zeros(kp.q8_par_bytes // 4, dtype=torch.float32, device=dev)
        self.gate = self.par[4 * kp.mfma_query_slots:].view(torch.int32)
        self.bound = torch.zeros(256, dtype=torch.float32, device=dev)
        self.keys = torch.zeros(256 * K, dtype=torch.int64, device=dev)
        self.advice = torch.full((2 * kp.q8_spec_k_count,), -1, dtype=torch.int32, device=dev)
        self.k_off = kp.q8_spec_k_off + kslot * kp.q8_spec_k_size
        self.kslot = kslot

    # -- the state words -----------------------------------------------------
    def _word(self, off, dt):
        return self.glob[off:off + 4].view(dt)

    def set_k(self, ratio=None, backoff=None, loose=None, since=None):
        t, kp = self.torch, self.kp
        if ratio is not None:
            self._word(self.k_off + kp.spec_k_ratio_off, t.float32)[0] = float(ratio)
        for v, o in ((backoff, kp.spec_k_backoff_off), (loose, kp.spec_k_loose_off),
                     (since, kp.spec_k_since_off)):
            if v is not None:
                self._word(self.k_off + o, t.int32)[0] = int(v)

    def state(self):
        kp = self.kp
        g = self.glob.cpu().numpy()
        rd = lambda off, dt: g[off:off + np.dtype(dt).itemsize].view(dt)[0]
        adv = self.advice.cpu().numpy().view(np.uint32)
        return dict(
            ratio=rd(self.k_off + kp.spec_k_ratio_off, np.float32),
            backoff=int(rd(self.k_off + kp.spec_k_backoff_off, np.uint32)),
            loose=int(rd(self.k_off + kp.spec_k_loose_off, np.uint32)),
            since=int(rd(self.k_off + kp.spec_k_since_off, np.uint32)),
            fails=int(rd(kp.q8_spec_stat_off + kp.spec_stat_fails_off, np.uint64)),
            verdict=int(self.gate.cpu().numpy()[kp.gate_verdict]),
            advice_loose=int(adv[self.kslot]), advice_cool=int(adv[kp.q8_spec_k_count + self.kslot]))

    # -- a batch -------------------------------------------------------------
    def load(self, s, qn, b, key_ok=None):
        """Per query: the k-th key's score s, |q| (its sigma is derived), the bound b."""
        t, nq = self.torch, self.nq
        s, qn, b = (np.asarray(x, np.float32) for x in (s, qn, b))
        rows = np.arange(nq, dtype=np.uint32) * 7 + 5
        kth = St.make_keys(s, rows)
        if key_ok is not None:
            kth = np.where(key_ok, kth, np.uint64(0))
        keys = np.zeros((nq, K), np.uint64)
        keys[:, :K - 1] = St.make_keys(np.float32(9.0) + np.zeros(nq, np.float32), rows)[:, None]
        keys[:, K - 1] = kth
        self.keys[:nq * K] = t.from_numpy(keys.view(np.int64).ravel()).to(self.keys.device)
        par = np.zeros((nq, 4), np.float32)
        par[:, 3] = _sigma(qn)
        self.par[:4 * nq] = t.from_numpy(par.ravel()).to(self.par.device)
        self.bound[:nq] = t.from_numpy(b).to(self.bound.device)

    def run(self, check, verdict0=0):
        kp = self.kp
        self.gate[kp.gate_verdict] = verdict0
        kp.check(kp.q8_verify_record(
            self.keys.data_ptr(), self.nq, K, DIM, self.bound.data_ptr(), self.par.data_ptr(),
            self.glob.data_ptr(), 1 if check else 0, self.gate.data_ptr(),
            self.glob.data_ptr() + self.k_off, self.glob.data_ptr() + kp.q8_spec_stat_off,
            self.advice.data_ptr() + 4 * self.kslot))
        self.torch.cuda.synchronize()
        return self.state()


def _want_ratio(s, qn, key_ok=None):
    """(the ratio a record teaches or None, nvalid) in fp64."""
    s, qn = np.asarray(s, np.float64), np.asarray(qn, np.float64)
    valid = (s > 0) & (qn > 0)
    if key_ok is not None:
        valid &= np.asarray(key_ok, bool)
    nvalid = int(valid.sum())
    if nvalid == 0:
        return None, 0
    r = np.sort(s[valid] / qn[valid])
    return float(np.float32(0.97)) * r[nvalid // 64], nvalid  # the (1 + nvalid / 64)-th smallest


def _spread(nq, rng):
    """Well-separated scores, norms and passing bounds for nq queries."""
    qn = (1.0 + 0.01 * rng.permutation(nq)).astype(np.float32)
    ratio = (0.3 + 0.002 * rng.permutation(nq)).astype(np.float32)
    s = (ratio * qn).astype(np.float32)
    b = (s * np.float32(0.99)).astype(np.float32)
    return s, qn, b


@pytest.mark.parametrize("nq", NQS)
def test_check_raises_on_any_single_query(kp, torch_, nq):
    """Mutation: `s >= b - sig * nmax` widened in spec_query_vals."""
    rng = np.random.default_rng(nq)
    B = Batch(kp, torch_, nq)
    fails = 0
    for idx in sorted({0, nq // 2, nq - 1}):
        for mode in ("one_ulp_under", "zero_key"):
            s, qn, b = _spread(nq, rng)
            key_ok = np.ones(nq, bool)
            if mode == "zero_key":
                key_ok[idx] = False
            else:  # the largest score that is still under the threshold
                b[idx] = s[idx] * np.float32(1.01)
                s[idx] = np.nextafter(_thr(b[idx], _sigma(qn[idx])), np.float32(-np.inf))
            B.set_k(ratio=0.25, backoff=0)
            B.load(s, qn, b, key_ok)
            st = B.run(check=True)
            fails += 1
            assert st["verdict"] == 1, (nq, idx, mode)
            assert st["fails"] == fails and st["backoff"] == 1, (nq, idx, mode, st)
            assert st["ratio"] == np.float32(0.25), "a failed check must leave the ratio to the sample path"


@pytest.mark.parametrize("nq", NQS)
def test_check_passes_at_the_threshold(kp, torch_, nq):
    """Every query at s == b - sigma nmax exactly, as fp32 computes it: verified."""
    rng = np.random.default_rng(100 + nq)
    B = Batch(kp, torch_, nq)
    s, qn, b = _spread(nq, rng)
    b = (s * np.float32(1.0001)).astype(np.float32)
    s = _thr(b, _sigma(qn))  # exactly the threshold
    assert np.all(s < b) and np.all(s > 0)
    B.set_k(ratio=0.25, backoff=8)
    B.load(s, qn, b)
    st = B.run(check=True)
    assert st["verdict"] == 0 and st["fails"] == 0, st
    assert st["backoff"] == 0, "a verified batch clears the back-off"
    want, _ = _want_ratio(s, qn)
    assert abs(float(st["ratio"]) - want) <= RTOL * want, (st["ratio"], want)


def test_backoff_doubles_and_caps(kp, torch_):
    nq = 65
    rng = np.random.default_rng(7)
    B = Batch(kp, torch_, nq)
    s, qn, b = _spread(nq, rng)
    b[nq - 1] = s[nq - 1] * np.float32(1.5)  # far above: fails
    B.load(s, qn, b)
    B.set_k(ratio=0.25, backoff=0)
    cap = kp.q8_spec_max_backoff
    seq, prev = [], 0
    for i in range(10):
        st = B.run(check=True)
        assert st["verdict"] == 1 and st["fails"] == i + 1
        seq.append(st["backoff"])
        # the cool-down the failure starts is the back-off it found (none the first time)
        assert st["advice_cool"] == (prev if prev else 0xFFFFFFFF), (i, st)
        prev = st["backoff"]
    want = [min(1 << i, cap) for i in range(10)]
    assert seq == want and want[-1] == cap, (seq, want)
    b[nq - 1] = s[nq - 1] * np.float32(0.9)
    B.load(s, qn, b)
    st = B.run(check=True)
    assert st["verdict"] == 0 and st["backoff"] == 0 and st["fails"] == 10, st


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("nq", NQS)
def test_ratio_is_the_low_quantile(kp, torch_, nq, check):
    """Mutation: m = 1 + nvalid / 64 -> nvalid / 64."""
    rng = np.random.default_rng(200 + nq)
    B = Batch(kp, torch_, nq)
    s, qn, b = _spread(nq, rng)
    key_ok = np.ones(nq, bool)
    if nq >= 63:  # queries that must not count: no k-th, s <= 0, a zero query
        key_ok[3] = False
        s[10], b[10] = -0.5, -1.0
        s[11], b[11] = 0.0, -1.0
        qn[20] = 0.0
    B.set_k(ratio=0.25, since=17, loose=1)
    B.load(s, qn, b, key_ok)
    if check and nq >= 63:  # the zero key would fail a check: give that query a key, keep it uncounted
        key_ok[3] = True
        s[3], b[3] = -1.0, -2.0
        B.load(s, qn, b, key_ok)
    st = B.run(check=check)
    want, nvalid = _want_ratio(s, qn, key_ok)
    assert nvalid == (nq - 4 if nq >= 63 else nq)
    assert st["verdict"] == 0
    assert abs(float(st["ratio"]) - want) <= RTOL * want, (st["ratio"], want, nvalid)
    if not check:
        assert st["since"] == 0, "a sample-path record resets the probe count"


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("tiny", [4, 5])
def test_quantile_edge_at_256(kp, torch_, tiny, check):
    """256 valid queries: the 5th smallest ratio. Four outliers are ignored, the
    fifth is the answer."""
    nq = 256
    rng = np.random.default_rng(300 + tiny)
    B = Batch(kp, torch_, nq)
    s, qn, b = _spread(nq, rng)
    where = rng.choice(nq, tiny, replace=False)
    s[where] = (np.float32(1e-3) * (1 + np.arange(tiny)) * qn[where]).astype(np.float32)
    b = (s * np.float32(0.5)).astype(np.float32)
    B.set_k(ratio=0.25)
    B.load(s, qn, b)
    st = B.run(check=check)
    want, nvalid = _want_ratio(s, qn)
    assert nvalid == 256
    if tiny == 4:
        assert want > 0.25, "the reference itself ignores four outliers"
    else:
        assert want < 0.01
    assert abs(float(st["ratio"]) - want) <= RTOL * want, (st["ratio"], want)


@pytest.mark.parametrize("check", [True, False])
def test_no_valid_query_leaves_the_ratio(kp, torch_, check):
    nq = 64
    B = Batch(kp, torch_, nq)
    s = np.full(nq, -0.25, np.float32)
    s[::2] = 0.0
    qn = np.ones(nq, np.float32)
    B.set_k(ratio=0.123)
    B.load(s, qn, np.full(nq, -1.0, np.float32))
    st = B.run(check=check)
    assert st["verdict"] == 0 and st["ratio"] == np.float32(0.123), st


@pytest.mark.parametrize("above", [64, 65])
def test_loose_boundary(kp, torch_, above):
    """Check off, 256 valid queries: loose exactly when 4 nloose > nvalid, i.e.
    from 65 sample bounds above R |q|. Mutation: > -> >=."""
    nq = 256
    rng = np.random.default_rng(400 + above)
    B = Batch(kp, torch_, nq)
    s, qn, _ = _spread(nq, rng)
    want, nvalid = _want_ratio(s, qn)
    assert nvalid == 256
    R = np.float32(want)
    b = (np.float32(0.5) * R * qn).astype(np.float32)
    hi = rng.choice(nq, above, replace=False)
    b[hi] = (np.float32(1.25) * R * qn[hi]).astype(np.float32)  # above R |q|, below every s
    B.set_k(ratio=0.25, since=17, loose=1 if above == 64 else 0)
    B.load(s, qn, b)
    st = B.run(check=False)
    assert st["loose"] == (1 if above == 65 else 0), (above, st)
    assert st["advice_loose"] == st["loose"] and st["since"] == 0, st
    assert abs(float(st["ratio"]) - want) <= RTOL * want


# ---------------------------------------------------------------------------
# the soundness implication on a real pipeline
# ---------------------------------------------------------------------------
DELTAS = ["-1e-2", "-1e-4", "0", "ulp", "+1e-6", "+1e-4", "+1e-2", "+0.3"]


def _scaled(sk, d):
    """b = s_k (1 + delta) in fp32 (s_k > 0); 'ulp': the next float above s_k."""
    if d == "ulp":
        return np.nextafter(sk, np.float32(np.inf))
    return (sk.astype(np.float64) * (1.0 + float(d))).astype(np.float32)


@pytest.mark.parametrize("f32", [pytest.param(False, id="bf16"), pytest.param(True, id="f32")])
def test_verdict_zero_implies_reference_keys(kp, torch_, f32):
    """int8 pass + select + check with per-query bounds b = s_k (1 + delta)
    around the reference pass's k-th score s_k: whenever the verdict word stays
    0 the keys are the reference pass's, bit for bit; delta <= 0 never raises it
    (a false failure costs a second pass), delta = +0.3 always does. The same
    through the select's last workgroup (SpecVerifyArgs), which must give the
    same verdict and record the same ratio as the separate launch."""
    torch = torch_
    dim, n, nq, k = 768, 333, 16, 10
    X, _ = R.make_rows("unit", n, dim, f32)
    coll = St.Collection(kp, torch, X, f32)
    Q, _ = R.make_queries(X, f32, 0, ("unit", "copy_row", "norm30", "onehot"))
    rng = np.random.default_rng(12)
    extra = R._unit(rng, nq - len(Q), dim)
    Q = np.concatenate([Q, extra if f32 else R._bf16(extra)])
    qs = St.Queries(kp, torch, Q, f32).quantize(coll)
    ref, _ = St.ref_pass(kp, torch, coll, qs, k)
    sk = St.key_scores(ref[:, k - 1])
    assert np.all(ref != 0) and np.all(sk > 0)
    glob_ptr = coll.glob.data_ptr()
    advice = torch.zeros(2 * kp.q8_spec_k_count, dtype=torch.int32, device=St.DEV)

    def slot(kslot):
        off = kp.q8_spec_k_off + kslot * kp.q8_spec_k_size
        return off, glob_ptr + off

    def run(b, in_select):
        off, k_ptr = slot(11 if in_select else 10)
        coll.glob[off:off + kp.q8_spec_k_size] = 0
        coll.glob[off + kp.spec_k_ratio_off:][:4].view(torch.float32)[0] = 0.25
        qs.gate[kp.gate_verdict] = 0
        bd = St.neg_inf(torch)
        bd[:nq] = torch.from_numpy(b).to(St.DEV)
        S = St.q8_pass(kp, torch, coll, qs, k, bound=bd)
        stat_ptr = glob_ptr + kp.q8_spec_stat_off
        adv = advice.data_ptr() + 4 * 10
        if in_select:
            keys = St.q8_select(kp, torch, coll, qs, S, k, bd,
                                verify=(1, k_ptr, stat_ptr, adv, qs.vq_ptr, qs.ticket_ptr))
        else:
            keys = St.q8_select(kp, torch, coll, qs, S, k, bd)
            out = St._i64(torch, keys)
            kp.check(kp.q8_verify_record(out.data_ptr(), nq, k, dim, bd.data_ptr(), qs.par.data_ptr(), glob_ptr,
                                         1, qs.gate.data_ptr(), k_ptr, stat_ptr, adv))
            torch.cuda.synchronize()
        verdict = int(qs.gate.cpu().numpy()[kp.gate_verdict])
        ratio = coll.glob[off + kp.spec_k_ratio_off:][:4].cpu().numpy().view(np.uint32)[0]
        return verdict, keys, ratio

    base = _scaled(sk, "-1e-2")
    cases = [(d, "all", _scaled(sk, d)) for d in DELTAS]
    for idx in (0, nq - 1):
        for d in DELTAS:
            b = base.copy()
            b[idx] = _scaled(sk, d)[idx]
            cases.append((d, f"query {idx}", b))
    for d, who, b in cases:
        v0, keys0, ratio0 = run(b, in_select=False)
        v1, keys1, ratio1 = run(b, in_select=True)
        for v, keys in ((v0, keys0), (v1, keys1)):
            assert v in (0, 1)
            if v == 0:  # the implication
                assert np.array_equal(keys, ref), ("verified, but the keys differ", d, who)
            if d in ("-1e-2", "-1e-4", "0"):
                assert v == 0, ("a bound at or under the k-th score failed its check", d, who)
            if d == "+0.3":
                assert v == 1, ("a bound 30% over the k-th score verified", d, who)
        assert v0 == v1 and ratio0 == ratio1, ("the select's own check differs from the launch", d, who,
                                               v0, v1, ratio0, ratio1)
        assert np.array_equal(keys0, keys1)
