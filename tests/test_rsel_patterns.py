"""(CPU) Every input pattern of tests/rsel_ref.py is built and its stated
property checked, so an edit to a builder cannot quietly lose the edge the
device test (tests/test_rsel_stages_gpu.py) relies on it for: which digit
decides, the boundary bucket's size and `need`, and where the reference's
keff-th key lies. The builders assert most of it themselves; what is asserted
here is the reference and the cross-pattern coverage."""
import numpy as np
import pytest

import rsel_ref as R


def _valid(case):
    live = int(np.count_nonzero(case.sc))
    assert case.sc.dtype == np.uint32 and case.keffs
    assert all(1 <= k <= live for k in case.keffs), (case.name, case.keffs, live)
    assert case.row_base + case.sc.size - 1 <= 0xFFFFFFFF


def test_reference_on_a_hand_case():
    sc = np.array([5, 0, 9, 5, 1], np.uint32)
    got = R.select(sc, 10, 3)
    want = [(9 << 32) | (0xFFFFFFFF - 12), (5 << 32) | (0xFFFFFFFF - 10), (5 << 32) | (0xFFFFFFFF - 13)]
    assert [int(x) for x in got] == want
    assert R.first_hist(sc)[0] == 4 and int(R.first_hist(sc).sum()) == 4
    # keff = 2: the two rows of image 5 differ in the row word's last digit only
    p, thr = R.deciding_digit(sc, 10, 2)
    assert p == 5 and thr == want[1]
    # keff = 1: image 9 alone in its bucket of the third digit
    assert R.deciding_digit(sc, 10, 1) == (2, 9 << 32)
    assert R.boundary(sc, 10, 2) == (0, 0, 4, 2)
    assert R.digit((1234 << 53) | (77 << 42) | (1000 << 32), 0) == 1234
    assert int(R.image(1234, 77, 1000)) == (1234 << 21) | (77 << 10) | 1000
    assert [int(x) for x in R.score_ord(np.array([1.0, -1.0, -0.0], np.float32))] == \
        [0xBF800000, 0x407FFFFF, 0x80000000]


@pytest.mark.parametrize("n", R.SIZES)
def test_sizes(n):
    c = R.sizes(n)
    _valid(c)
    assert c.sc.size == n and {1, n} <= set(c.keffs)


def test_second_round():
    for cus in (8, 256, 304):
        n = R.second_round_rows(cus)
        full = 4 * cus * 1024  # rows of one round of 4 workgroups a CU, 4 rows a thread
        assert full + 1029 < n < full + 2048
    c = R.second_round(8)
    _valid(c)


@pytest.mark.parametrize("masked", [0, 1])
def test_full_range(masked):
    c = R.full_range(masked)
    _valid(c)
    live = int(np.count_nonzero(c.sc))
    assert live in c.keffs  # takes everything, bucket 0 included
    firsts = {R.digit(R.select(c.sc, c.row_base, k)[-1], 0) for k in c.keffs}
    assert {0, 2047} <= firsts and len(firsts) >= 4


@pytest.mark.parametrize("level", [0, 1, 2])
def test_pick_positions_cover_every_owned_bucket(level):
    seen = set()
    for t in R.PICK_T:
        for j in range(8):
            c, g, na = R.pick_position(t, j, level)
            _valid(c)
            kth = R.select(c.sc, c.row_base, na + 2)[-1]
            assert R.digit(kth, level) == g
            # the bucket as the fused selection's picks see it (level 2: with the row word's top bit)
            seen.add((t, g % 8 if level < 2 else ((int(kth) >> 31) & 2047) % 8))
            assert {na + 1, na + 2, na + 3} <= set(c.keffs)
            assert 0 < len(c.keffs) <= 5
    assert seen == {(t, j) for t in R.PICK_T for j in range(8)}
    # first and last bucket of the digit are reached
    assert R.pick_position(0, 0, level)[1] == 0
    assert R.pick_position(255, 7, level)[1] == (2047 if level < 2 else 1023)


@pytest.mark.parametrize("level,big", [(0, False), (1, False), (2, False), (1, True)])
def test_whole_bucket(level, big):
    c = R.whole_bucket(level, big)
    _valid(c)
    keff = c.keffs[1]
    assert c.keffs == [keff - 1, keff, keff + 1]
    assert R.deciding_digit(c.sc, c.row_base, keff)[0] == level
    assert R.deciding_digit(c.sc, c.row_base, keff - 1)[0] > level
    _, _, h1, need = R.boundary(c.sc, c.row_base, keff)
    assert (need == h1) == (level < 2)


@pytest.mark.parametrize("h1", R.H1S)
def test_boundary_size(h1):
    c = R.boundary_size(h1)
    _valid(c)
    needs = sorted({1, h1 // 2, h1 - 1} - {0})
    assert [k - 5 for k in c.keffs] == needs
    for k in c.keffs:
        assert R.boundary(c.sc, c.row_base, k)[2:] == (h1, k - 5)
    assert {h <= R.SORT_CAP for h in R.H1S} == {True, False}
    assert {R.SORT_CAP - 1, R.SORT_CAP, R.SORT_CAP + 1} <= set(R.H1S)


@pytest.mark.parametrize("row_base", [0, 77, "top"])
@pytest.mark.parametrize("n", [700, 4500])
def test_all_equal(n, row_base):
    c = R.all_equal(n, row_base)
    _valid(c)
    assert len(set(c.sc.tolist())) == 1
    if row_base == "top":
        assert c.row_base + n == 1 << 32


def test_runs_and_realistic_and_trailer():
    c = R.runs()
    _valid(c)
    assert len(set(c.sc.tolist())) == 5 and len(c.keffs) == 6
    for k in c.keffs:  # every keff of the runs case is decided inside the row word or takes a run whole
        assert R.deciding_digit(c.sc, c.row_base, k)[0] <= 5
    _valid(R.realistic())
    t = R.trailer()
    _valid(t)
    assert np.count_nonzero(t.sc == 0) > 0
