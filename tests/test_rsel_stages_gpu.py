"""(GPU) Both large-k selections (csrc/vs_select.hip: launch_rsel, the digit
chain, and launch_rsel_fused, three launches) against a sort, on score images
the test builds (tests/rsel_ref.py; tests/test_rsel_patterns.py checks on the
CPU that every pattern has the edge it is named for).

Through the engine the selections only ever see cosine / dot scores of unit
vectors: a handful of the 2048 first-digit buckets, and a k-th key decided in
the first digit or among exact ties. Here `sc` and its first-digit histogram
are written by the test, and for every (pattern, keff), for both launchers:
  * the keff keys in sel, sorted, equal the keff largest keys exactly;
  * sel past keff, and every scratch buffer past its documented size, is
    untouched;
  * hist, hist1 and ctr[0..3) are zero afterwards; the chain's state.count is
    keff and state.thr the keff-th key cut to the digit that decided it;
  * the next selection runs on the same hist / hist1 / ctr / state without
    clearing them (the next score pass only adds to hist), and every case ends
    with one more, different selection on them.

Mutations of vs_select.hip each tried once on a scratch build (they change
values only, never an address or a loop bound); the family that fails:
  * pick position: the in-thread bucket walk of fused_pick skipped (the
    second `for` of it) -> every test here fails in the fused selection
    (test_pick_position at every level and thread);
  * bucket taken whole: `h[b] == need ||` dropped from rsel_pick_kernel's stop
    (the chain then walks all six digits; its keys stay right, state.thr is no
    longer the prefix) -> test_whole_bucket and every other chain case, at
    the state.thr check;
  * LDS / global switch: the LDS copy of f3 stores `cand[i] | 1` ->
    test_boundary_size fails at h1 = 4095 and 4096 and passes at 4097 and
    9000. (`<` for `<=` against kFusedSortCap changes no value: at 4096 keys
    both sources hold the same keys, so no test can see it.)
  * ties: `key > thr` for `key >= thr` in f3's final append and in
    rsel_compact_kernel -> test_all_equal, test_runs and every other case
    decided in the key's last digit come back one key short;
  * zero on exit: `hist1[i] = 0` dropped from f3 -> every fused case, at the
    check after its first selection.
"""
import numpy as np
import pytest

import rsel_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
P32 = 0x5A5A5A5A
P64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def kp():
    import kprobe
    k = kprobe.load()
    assert k.rsel_bins == R.BINS
    return k


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def _u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def _poisoned(torch, n, dtype):
    return torch.full((n + GUARD,), P32 if dtype == torch.int32 else P64, dtype=dtype, device=DEV)


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _np64(t):
    return t.cpu().numpy().view(np.uint64)


class Buffers:
    """hist / hist1 / ctr / state of one stream of selections: zero once (the
    state is poisoned: pass 0 of the chain initialises it), never cleared again."""

    def __init__(self, kp, torch):
        self.kp, self.torch = kp, torch
        self.hist = _poisoned(torch, R.BINS, torch.int32)
        self.hist1 = _poisoned(torch, R.BINS, torch.int32)
        self.ctr = _poisoned(torch, 3, torch.int32)
        self.hist[:R.BINS] = 0
        self.hist1[:R.BINS] = 0
        self.ctr[:3] = 0
        assert kp.rsel_state_size % 8 == 0
        self.state = _poisoned(torch, kp.rsel_state_size // 8, torch.int64)

    def check_clean(self, what):
        for name, t, n in (("hist", self.hist, R.BINS), ("hist1", self.hist1, R.BINS), ("ctr", self.ctr, 3)):
            a = _np32(t)
            assert not a[:n].any(), (what, name, "not left zero", np.nonzero(a[:n])[0][:8])
            assert np.all(a[n:] == P32), (what, "wrote past", name)
        assert np.all(_np64(self.state)[self.kp.rsel_state_size // 8:] == P64), (what, "wrote past the state")

    def state_field(self, off, size):
        b = self.state.cpu().numpy().view(np.uint8)[off:off + size]
        return int(b.view(np.uint32 if size == 4 else np.uint64)[0])

    def select(self, fused, scd, hist_add, n, row_base, keff, want, thr, what):
        """One selection of keff keys from the uploaded images scd[:n]."""
        kp, torch = self.kp, self.torch
        self.hist[:R.BINS] += hist_add  # as the score pass leaves it: added to a zeroed hist
        sel = _poisoned(torch, keff, torch.int64)
        if fused:
            cand = _poisoned(torch, n, torch.int64)
            kp.check(kp.rsel_fused(scd.data_ptr(), n, row_base, keff, self.hist.data_ptr(),
                                   self.hist1.data_ptr(), self.ctr.data_ptr(), sel.data_ptr(),
                                   cand.data_ptr()))
        else:
            kp.check(kp.rsel(scd.data_ptr(), n, row_base, keff, self.hist.data_ptr(),
                             self.state.data_ptr(), sel.data_ptr()))
        torch.cuda.synchronize()
        self.check_clean(what)
        got = _np64(sel)
        assert np.all(got[keff:] == P64), (what, "wrote past sel[keff]")
        if fused:
            assert np.all(_np64(cand)[n:] == P64), (what, "wrote past cand[n_rows]")
        got = np.sort(got[:keff])[::-1]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, "first wrong key at", int(bad[0]), hex(int(got[bad[0]])),
                               hex(int(want[bad[0]])), "wrong keys", bad.size)
        if not fused:
            assert self.state_field(kp.rsel_state_count_off, 4) == keff, (what, "state.count")
            assert self.state_field(kp.rsel_state_done_off, 4) == 1, (what, "state.done")
            assert self.state_field(kp.rsel_state_thr_off, 8) == thr, (what, "state.thr")


def _run(kp, torch, cases, which=(False, True)):
    """Every keff of every case with both launchers, each launcher on its own
    uncleared Buffers; then the trailer selection on the same buffers."""
    bufs = {f: Buffers(kp, torch) for f in which}
    for case in list(cases) + [R.trailer()]:
        n = case.sc.size
        # poisoned (non-zero) images behind row n: a read past n changes the answer
        scd = _poisoned(torch, n, torch.int32)
        scd[:n] = _u32(torch, case.sc)
        hist = _u32(torch, R.first_hist(case.sc))
        ordered = np.sort(R.keys_of(case.sc, case.row_base))[::-1]
        for keff in case.keffs:
            want = ordered[:keff]
            _, thr = R.deciding_digit(case.sc, case.row_base, keff)
            for fused in which:
                what = (case.name, "fused" if fused else "chain", "keff", keff)
                bufs[fused].select(fused, scd, hist, n, case.row_base, keff, want, thr, what)
        assert np.all(_np32(scd)[n:] == P32)


@pytest.mark.parametrize("n", R.SIZES)
def test_sizes(kp, torch_, n):
    """n under one workgroup and the 16-byte load's tail, keff from 1 to n."""
    _run(kp, torch_, [R.sizes(n)])


def test_second_round(kp, torch_):
    """Rows past one round of the widest grid (CUs read from the device)."""
    cus = kp.device_cu_count()
    assert 1 <= cus <= 4096
    _run(kp, torch_, [R.second_round(cus)])


@pytest.mark.parametrize("masked", [0, 1])
def test_full_range(kp, torch_, masked):
    """Uniform u32 images: buckets 0 and 2047 hold keys; half the rows masked;
    keff = the unmasked count."""
    _run(kp, torch_, [R.full_range(masked)])


@pytest.mark.parametrize("t", R.PICK_T)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_pick_position(kp, torch_, level, t):
    """The keff-th key's digit on each of the 8 buckets pick thread t owns, in
    the first, second and third digit of the image."""
    _run(kp, torch_, [R.pick_position(t, j, level)[0] for j in range(8)])


def test_whole_bucket(kp, torch_):
    """above + h[b] == keff at the first, second and third digit; the copy
    branch of the fused last stage with 7 and with 6300 keys."""
    _run(kp, torch_, [R.whole_bucket(0), R.whole_bucket(1), R.whole_bucket(2), R.whole_bucket(1, big=True)])


@pytest.mark.parametrize("h1", R.H1S)
def test_boundary_size(kp, torch_, h1):
    """The boundary bucket's keys in LDS (<= 4096) and in global memory."""
    _run(kp, torch_, [R.boundary_size(h1)])


@pytest.mark.parametrize("row_base", [0, 77, "top"])
def test_all_equal(kp, torch_, row_base):
    """Every image equal: decided in the row word; the last row's word 0."""
    _run(kp, torch_, [R.all_equal(700, row_base), R.all_equal(4500, row_base)])


def test_runs(kp, torch_):
    """keff on the first and on the last row of a run of equal images."""
    _run(kp, torch_, [R.runs()])


def test_realistic(kp, torch_):
    _run(kp, torch_, [R.realistic()])
