"""CPU checks of tests/fuse_ref.py, the numpy statement of the fused-search rule
(include/vsearch.h "Fused search") that the GPU tests compare the device with:
hand-computed cases, and proof that the shared fixtures exercise what they are
meant to (summation order, rows in several lists, exact ties)."""
import numpy as np

import fuse_ref as FR

f32 = np.float32


def _rows_scores(keys):
    n = int(np.count_nonzero(keys))
    assert not keys[n:].any()
    return FR.key_row(keys[:n]).tolist(), FR.key_score(keys[:n])


def test_key_round_trip():
    s = np.array([1.5, -2.25, 0.0, -0.0, 3e-9], f32)
    r = np.array([0, 7, 2 ** 32 - 2, 5, 123456], np.uint64)
    k = FR.key_encode(s, r)
    assert np.array_equal(FR.key_row(k), r)
    assert np.array_equal(FR.key_score(k), s)
    assert FR.key_encode([2.0], [9])[0] > FR.key_encode([1.0], [3])[0]
    assert FR.key_encode([1.0], [3])[0] > FR.key_encode([1.0], [4])[0]   # equal score: lower row first


def test_rrf_by_hand():
    """2 lists x 3 slots, K = 2: terms 1/2, 1/3, 1/4 by rank."""
    lists = np.stack([FR._list([10, 20, 30]), FR._list([20, 40, 10])])
    rows, sc = _rows_scores(FR.rrf(lists, 5))
    assert rows == [20, 10, 40, 30]
    third = f32(1) / f32(3)
    want = np.array([f32(third + f32(0.5)),      # row 20: list 0's term first
                     f32(0.75),                  # row 10: 1/2 + 1/4
                     third, f32(0.25)], f32)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))
    # the cut, and K = 60 (terms 1/60, 1/61, 1/62)
    assert FR.key_row(FR.rrf(lists, 2)).tolist() == [20, 10]
    rows, sc = _rows_scores(FR.rrf(lists, 4, 60))
    assert rows == [20, 10, 40, 30]
    assert sc[0] == f32(f32(1) / f32(61) + f32(1) / f32(60))
    assert sc[1] == f32(f32(1) / f32(60) + f32(1) / f32(62))


def test_dbsf_by_hand():
    """List 0 scores {2, 0, -2}: mu 0, sigma 2, terms 2/3, 1/2, 1/3. List 1 has
    three equal scores: sigma 0, every term 0.5."""
    lists = np.stack([FR._list([10, 20, 30], [2.0, 0.0, -2.0]),
                      FR._list([20, 40, 50], [1.0, 1.0, 1.0])])
    keys, f64 = FR.dbsf(lists, 6)
    rows, sc = _rows_scores(keys)
    assert rows == [20, 10, 40, 50, 30]
    want = np.array([1.0, f32(2 / 3), 0.5, 0.5, f32(1 / 3)], f32)
    assert np.array_equal(sc.view(np.uint32), want.view(np.uint32))
    assert f64[20] == 1.0 and abs(f64[10] - 2 / 3) < 1e-15
    # a single entry: n_l = 1, term 0.5
    one = np.zeros((1, 3), np.uint64)
    one[0, 0] = FR.key_encode([7.0], [4])[0]
    rows, sc = _rows_scores(FR.dbsf(one, 3)[0])
    assert rows == [4] and sc[0] == f32(0.5)


def test_single_list_keeps_its_order():
    lst = FR.overlap(1, 1, 100)[0]
    for k in (1, 37, 100):
        assert FR.key_row(FR.rrf(lst, k)).tolist() == FR.key_row(lst[0, :k]).tolist()
    # DBSF is monotone in the score, which falls strictly along the list
    assert FR.key_row(FR.dbsf(lst, 100)[0]).tolist() == FR.key_row(lst[0]).tolist()


def test_empty_slots_contribute_nothing():
    lists = FR.overlap(1, 3, 16, pool=20)[0]
    cut = lists.copy()
    cut[1, 5:] = 0
    cut[2, :] = 0
    a = FR.rrf_scores(cut)
    b = FR.rrf_scores(np.stack([lists[0], np.concatenate([lists[1, :5], np.zeros(11, np.uint64)])]))
    assert a == b
    assert not FR.rrf(np.zeros((4, 9), np.uint64), 7).any()
    assert not FR.dbsf(np.zeros((4, 9), np.uint64), 7)[0].any()


def test_overlap_fixture_fixes_the_summation_order():
    """Every query has a row whose fp32 sum differs when the lists are added in
    descending l, so a device that sums in another order cannot pass."""
    Q = FR.overlap(32)
    for q in range(32):
        asc, desc = FR.rrf_scores(Q[q]), FR.rrf_scores(Q[q], order="desc")
        assert asc.keys() == desc.keys()
        assert any(asc[r].view(np.uint32) != desc[r].view(np.uint32) for r in asc), q


def test_overlap_fixture_top_rows_sit_in_several_lists():
    Q = FR.overlap(32)
    for q in range(32):
        top = FR.key_row(FR.rrf(Q[q], 10)).tolist()
        rows = [set(FR.key_row(l).tolist()) for l in Q[q]]
        assert all(sum(r in s for s in rows) >= 2 for r in top), q


def test_reversed_pair_fixture_has_exact_ties():
    Q = FR.reversed_pair(4)
    for q in range(4):
        sc = FR.rrf_scores(Q[q])
        assert len(sc) == 128
        assert len({float(v) for v in sc.values()}) == 64
        # ... which the key order breaks by the lower row
        rows = FR.key_row(FR.rrf(Q[q], 128)).tolist()
        assert all(rows[i] < rows[i + 1] for i in range(0, 128, 2))


def test_disjoint_fixture_answer_is_rank_major():
    Q = FR.disjoint(2, 5, 17)
    for q in range(2):
        want = sum((sorted(FR.key_row(Q[q][:, p]).tolist()) for p in range(17)), [])
        assert FR.key_row(FR.rrf(Q[q], 85)).tolist() == want
