"""(CPU) tests/groups_ref.py, the numpy restatement of grouped search, on cases
written out by hand."""
import numpy as np

import groups_ref as G

NONE = G.GROUP_NONE


def _ranking(scores, row_base=0):
    return G.ranking_of_images(G.score_image(np.asarray(scores, np.float32)), row_base)


def _rows(ref, row_base=0):
    return [(g, [int(G.key_rows(np.uint64(k))) - row_base for k in ks]) for g, ks in ref]


def test_image_round_trip_and_order():
    s = np.array([-2.0, -0.0, 0.0, 1e-30, 0.5, 3.0], np.float32)
    im = G.score_image(s)
    assert np.all(np.diff(im.astype(np.int64)) >= 0) and im[1] == im[2]
    back = G.image_score(im)
    assert back[1] == 0.0 and not np.signbit(back[1])
    assert np.array_equal(np.delete(back, 1), np.delete(s, 1))
    assert np.all(im != 0)


def test_plain_groups():
    #        row:  0    1    2    3    4    5
    scores = [0.9, 0.1, 0.8, 0.7, 0.2, 0.95]
    gor = np.array([0, 0, 1, 1, 2, 2], np.uint32)
    ref = G.groups_ref(_ranking(scores), gor, 2, 2)
    assert _rows(ref) == [(2, [5, 4]), (0, [0, 1])]
    ref = G.groups_ref(_ranking(scores), gor, 5, 1)
    assert _rows(ref) == [(2, [5]), (0, [0]), (1, [2])]


def test_score_tie_across_groups_goes_to_the_lower_row():
    scores = [0.5, 0.75, 0.75, 0.1]
    gor = np.array([3, 1, 0, 1], np.uint32)
    ref = G.groups_ref(_ranking(scores), gor, 3, 2)
    # rows 1 and 2 tie; row 1 is lower, so group 1 comes first
    assert _rows(ref) == [(1, [1, 3]), (0, [2]), (3, [0])]


def test_empty_group_is_absent_and_limit_above_groups():
    scores = [0.2, 0.4]
    gor = np.array([0, 2], np.uint32)  # group 1 of n_groups = 3 has no rows
    ref = G.groups_ref(_ranking(scores), gor, 8, 4)
    assert _rows(ref) == [(2, [1]), (0, [0])]
    groups, hits, keys, count = G.as_arrays(ref, 8, 4)
    assert count == 2 and list(groups[:3]) == [2, 0, 0] and list(hits[:3]) == [1, 1, 0]
    assert np.count_nonzero(keys) == 2


def test_ungrouped_row_on_top_is_skipped():
    scores = [0.99, 0.5, 0.6]
    gor = np.array([NONE, 0, 0], np.uint32)
    ref = G.groups_ref(_ranking(scores), gor, 1, 16)
    assert _rows(ref) == [(0, [2, 1])]


def test_masked_rows_and_row_base():
    im = G.score_image(np.array([0.3, 0.9, 0.8], np.float32))
    im[1] = 0  # masked: no key
    keys = G.ranking_of_images(im, row_base=1000)
    assert list(G.key_rows(keys)) == [1002, 1000]
    gor = np.array([0, 0, 1], np.uint32)
    ref = G.groups_ref(keys, gor, 2, 2, row_base=1000)
    assert _rows(ref, 1000) == [(1, [2]), (0, [0])]
