"""(GPU) The sample bound's radix select (csrc/vs_bound_dev.h
sample_bound_block / wave_digit_pick) against an integer restatement, bit for
bit, through launch_sample_bound and the bound half of launch_sample_bound_q8.

Final keys only need the bound to be a lower bound on the k-th score, so no
end-to-end test sees a pick that lands a digit too low (it costs speed) and
one that lands too high shows only on adversarial tile maxima. Reference:
    o = ord_f32(k-th largest of tmax[q, :m])   (order-preserving image)
    o &= ~0 << (32 - 8 passes)                 (the radix passes kept)
    bound = -inf if o <= ord_f32(-inf) else the float of image o
and -inf when m < k. `passes` is read from the library.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF_ORD = 0x007FFFFF  # ord_f32(-inf)


def _ord(f):
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint32)


def _unord(o):
    o = np.asarray(o, np.uint64)
    u = np.where(o & 0x80000000, o & 0x7FFFFFFF, ~o & 0xFFFFFFFF).astype(np.uint32)
    return u.view(np.float32)


def _reference(tmax, k, passes):
    """-> (bound bits as uint32 [nq], the true k-th largest as float [nq])."""
    nq, m = tmax.shape
    if m < k:
        return np.full(nq, np.float32(-np.inf)).view(np.uint32), np.full(nq, -np.inf, np.float32)
    o = np.sort(_ord(tmax), axis=1)[:, m - k]
    kept = np.uint32((0xFFFFFFFF << (32 - 8 * passes)) & 0xFFFFFFFF)
    p = o & kept
    out = np.where(p <= NEG_INF_ORD, np.float32(-np.inf), _unord(p)).astype(np.float32)
    return out.view(np.uint32), _unord(o)


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def _run(kp, torch, tmax, k):
    """Both launchers on tmax [nq, m] -> (bound, bound of the fused launch) as uint32."""
    nq, m = tmax.shape
    dev = "cuda:0"
    t = torch.from_numpy(np.ascontiguousarray(tmax, np.float32)).to(dev)
    if t.numel() == 0:
        t = torch.zeros(1, device=dev)
    b1 = torch.full((256,), 123.0, device=dev)
    b2 = torch.full((256,), 456.0, device=dev)
    kp.check(kp.sample_bound(t.data_ptr(), m, nq, k, b1.data_ptr()))
    # the fused launch needs a query half: one 128-d query of a throw-away collection
    q = torch.zeros((4, 128), dtype=torch.float32, device=dev)
    glob = torch.ones(kp.q8_glob_bytes // 4, device=dev)
    q8 = torch.zeros((4, 128), dtype=torch.int8, device=dev)
    par = torch.zeros(kp.q8_par_bytes // 4, device=dev)
    gate = par[4 * kp.mfma_query_slots:].view(torch.int32)
    kp.check(kp.sample_bound_q8(t.data_ptr(), m, nq, k, b2.data_ptr(), q.data_ptr(), 1, 1, 128,
                                glob.data_ptr(), q8.data_ptr(), par.data_ptr(), gate.data_ptr()))
    torch.cuda.synchronize()
    o1, o2 = b1.cpu().numpy(), b2.cpu().numpy()
    assert np.all(o1[nq:] == 123.0) and np.all(o2[nq:] == 456.0), "wrote past nq"
    return o1[:nq].view(np.uint32), o2[:nq].view(np.uint32)


def _check(kp, torch, tmax, k, what):
    passes = kp.sample_bound_passes()
    assert 2 <= passes <= 4
    want, kth = _reference(tmax, k, passes)
    got, got8 = _run(kp, torch, tmax, k)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, k, tmax.shape, "query", int(bad[0]), "got",
                           got.view(np.float32)[bad[0]], "want", want.view(np.float32)[bad[0]])
    assert np.array_equal(got8, got), (what, "launch_sample_bound_q8 differs from launch_sample_bound")
    assert np.all(got.view(np.float32) <= kth), (what, "above the true k-th")


def _from_first_bytes(bytes_, low=None):
    """Finite floats whose order image has the given first bytes (and low 24 bits)."""
    b = np.asarray(bytes_, np.uint32)
    lo = np.where(b >= 128, 0x400000, 0xC00000).astype(np.uint32) if low is None else np.asarray(low, np.uint32)
    f = _unord((b << 24) | lo)
    assert np.all(np.isfinite(f))
    return f


@pytest.mark.parametrize("k", [1, 2, 64, 128])
@pytest.mark.parametrize("m", [1, 255, 257, 4099])
@pytest.mark.parametrize("nq", [1, 256])
def test_random_maxima(kp, torch_, nq, m, k):
    """m not a multiple of the 256 threads, m < k (-inf) included."""
    rng = np.random.default_rng(m * 1000 + k)
    t = (rng.standard_normal((nq, m)) * 0.2).astype(np.float32)
    _check(kp, torch_, t, k, "random")


@pytest.mark.parametrize("k", [1, 2, 64, 128])
def test_m_equals_k(kp, torch_, k):
    rng = np.random.default_rng(k)
    t = rng.standard_normal((5, k)).astype(np.float32)
    _check(kp, torch_, t, k, "m == k")  # the bound is the floor of the minimum
    t[:, k // 2] = -np.inf  # m == k with -inf among them: no k finite maxima
    want, _ = _reference(t, k, kp.sample_bound_passes())
    assert np.all(want.view(np.float32) == -np.inf)
    _check(kp, torch_, t, k, "m == k with -inf")


@pytest.mark.parametrize("k", [1, 2, 64, 128])
def test_value_patterns(kp, torch_, k):
    m = 300
    rng = np.random.default_rng(50 + k)
    # all equal (a value with bits below the kept digits, so the floor differs from it)
    _check(kp, torch_, np.full((3, m), np.float32(0.3337), np.float32), k, "all equal")
    # all negative
    _check(kp, torch_, -np.abs(rng.standard_normal((3, m))).astype(np.float32) - 0.01, k, "negative")
    # values that differ only below the kept digits (the top 16 bits shared)
    base = np.float32(0.5).view(np.uint32)
    t = (base + rng.integers(0, 1 << 8, (3, m)).astype(np.uint32)).view(np.float32)
    _check(kp, torch_, t, k, "equal above the kept digits")
    # values that differ in the second digit only
    t = (base + (rng.integers(0, 256, (3, m)).astype(np.uint32) << 16)).view(np.float32)
    _check(kp, torch_, t.astype(np.float32), k, "second digit")
    # a block of -inf at the end, as a workgroup's missing tiles leave: fewer
    # than k finite values, exactly k, and more
    for finite in (k - 1, k, k + 1, m - 7):
        t = rng.standard_normal((3, m)).astype(np.float32)
        t[:, max(finite, 0):] = -np.inf
        _check(kp, torch_, t, k, f"-inf tail after {finite}")
    # +-0 around the k-th place (-0 orders below +0)
    t = np.zeros((3, m), np.float32)
    t[:, ::2] = -0.0
    t[0, :k] = 1.0
    t[1, : k - 1] = 1.0
    _check(kp, torch_, t, k, "signed zeros")
    t = np.full((2, m), np.float32(-0.0))
    t[1, 0] = 0.0
    _check(kp, torch_, t, k, "negative zeros")


@pytest.mark.parametrize("lane", [0, 1, 31, 62, 63])
@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_kth_in_each_sub_digit_of_a_lane(kp, torch_, lane, j):
    """wave_digit_pick: lane l owns digits 255 - 4l .. 252 - 4l; the k-th value
    sits in its j-th, with values in the lane's other digits and in other lanes'
    on both sides. Then the same layout in the second digit.
    Mutation: the `a + oz < kk` step of wave_digit_pick skipped (the k-th in
    sub-digits j = 2, 3 then lands a digit too high)."""
    g = 255 - 4 * lane - j
    above = [d for d in (g + 1, g + 2, g + 3, g + 5, 255) if g < d <= 255]
    below = [d for d in (g - 1, g - 2, g - 3, g - 6, 0) if 0 <= d < g]
    bytes_ = []
    for d in above:
        bytes_ += [d, d]
    na = len(bytes_)
    bytes_ += [g, g, g]
    for d in below:
        bytes_ += [d, d, d]
    bytes_ = np.array(bytes_, np.uint32)
    low = np.where(bytes_ >= 128, 0x400000, 0xC00000).astype(np.uint32)
    low[na:na + 3] += np.array([0x030000, 0x020000, 0x010000], np.uint32)  # second digits differ
    rng = np.random.default_rng(g)
    rows = []
    for _ in range(4):
        p = rng.permutation(len(bytes_))
        rows.append(_from_first_bytes(bytes_[p], low[p]))
    t = np.stack(rows)
    for k in (na + 1, na + 2, na + 3):  # each of the three values inside digit g
        _check(kp, torch_, t, k, f"first digit {g}")
    for k in {max(na, 1), na + 4} - {0}:  # the neighbours: the last above, the first below
        if k <= t.shape[1]:
            _check(kp, torch_, t, k, f"beside first digit {g}")
    # second digit: one first byte (0xBF: floats in [0.5, 2)), second bytes as above
    sec = (np.uint32(0xBF) << 24) | (bytes_ << 16) | np.uint32(0x1234)
    t2 = np.stack([_unord(sec[rng.permutation(len(sec))]) for _ in range(4)])
    assert np.all(np.isfinite(t2))
    for k in (na + 1, na + 2, na + 3):
        _check(kp, torch_, t2, k, f"second digit {g}")
