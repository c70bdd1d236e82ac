"""(GPU) The grouped-search stages of csrc/vs_group.hip on score images the
test builds, against tests/groups_ref.py, exactly. No scan is involved: `sc`
(what launch_gemv_scores would leave) and the first-digit histogram are written
here, and the stages run in the engine's order through the shim
tests/kprobe/vs_kprobe_groups.cpp:

    group_best -> group_heads -> merge -> group_members -> merge -> group_clear

For every case:
  * best after group_best is every group's largest key (0: no eligible row);
  * the returned groups, their order and their hits equal groups_ref;
  * the outputs are zero past the counts (VS_GROUP_NONE in the group ids);
  * best and the histogram read zero afterwards, sc and the ids are unchanged,
    and no buffer is written past its stated extent (guard words behind each).

Layouts: contiguous runs that straddle wave (64) and workgroup-step (1024)
boundaries, the same ids permuted, one group for all rows, one group per row,
every third row without a group. Images: few distinct values (so most
decisions fall to the row word), a whole group masked, and ascending ones (the
worst case of the workgroup lists: every row displaces an earlier one). The two
1.7 M-row cases are the smallest at which a workgroup walks enough 1024-row
steps (4 with a 128-key table, 3 with a 2048-key one) to flush its candidate
buffer inside the loop and not only at the end.
"""
import numpy as np
import pytest

import groups_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
P32 = 0x5A5A5A5A
P64 = 0x5A5A5A5A5A5A5A5A
NONE = G.GROUP_NONE
SIZES = [1, 63, 64, 65, 4097, 200003]
LAYOUTS = ["runs", "permuted", "one_group", "own_group", "third_none"]


@pytest.fixture(scope="module")
def kg():
    from kprobe import groups
    k = groups.load()
    assert (k.group_none, k.max_limit, k.max_size) == (NONE, G.MAX_LIMIT, G.MAX_SIZE)
    return k


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev32(torch, a, guard=P32):
    a = np.concatenate([np.ascontiguousarray(a, np.uint32), np.full(GUARD, guard, np.uint32)])
    return torch.from_numpy(a.view(np.int32)).to(DEV)


def _dev64(torch, a):
    a = np.concatenate([np.ascontiguousarray(a, np.uint64), np.full(GUARD, P64, np.uint64)])
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _np64(t):
    return t.cpu().numpy().view(np.uint64)


def layout(name, n, rng):
    """(group_of_row, n_groups)"""
    if name == "one_group":
        return np.zeros(n, np.uint32), 1
    if name == "own_group":
        return rng.permutation(n).astype(np.uint32), n
    # runs of 1..300 rows: they straddle the 64-row waves and the 1024-row steps
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(1, 301)))
    g = np.repeat(np.arange(len(lens), dtype=np.uint32), lens)[:n]
    ng = int(g.max()) + 2  # the last group has no rows
    if name == "permuted":
        g = g[rng.permutation(n)]
    if name == "third_none":
        g = g.copy()
        g[::3] = NONE
    return g, ng


def images(kind, n, gor, rng):
    if kind == "few":  # ties in the image: the row word decides
        vals = G.score_image(np.array([-0.5, 0.0, 0.25, 0.25000003, 0.9], np.float32))
        sc = vals[rng.integers(0, len(vals), n)]
    elif kind == "ascending":
        sc = (np.uint32(0x80000000) + np.arange(n, dtype=np.uint32) * np.uint32(3))
    else:
        sc = G.score_image(rng.standard_normal(n).astype(np.float32))
    sc = sc.astype(np.uint32)
    assert np.all(sc != 0)
    if kind != "ascending" and n > 2:  # a whole group masked, and a few single rows
        grouped = gor[gor != NONE]
        if grouped.size:
            sc[gor == grouped[grouped.size // 2]] = 0
        sc[rng.integers(0, n, max(1, n // 50))] = 0
    return sc


def run_stages(kg, torch, sc, gor, n_groups, limit, S, row_base):
    n = sc.size
    L = kg.group_lists(n)
    assert 1 <= L <= kg.max_lists
    T = limit * S
    rng = np.random.default_rng(n + limit)
    d_sc, d_gid = _dev32(torch, sc), _dev32(torch, gor)
    d_best = _dev64(torch, np.zeros(n_groups, np.uint64))
    # what a score pass leaves: counts; the stages must hand it back zeroed
    d_hist = _dev32(torch, rng.integers(0, 1000, kg.rsel_bins))
    d_lists = _dev64(torch, np.full(L * T, P64, np.uint64))
    d_heads = _dev64(torch, np.full(limit, P64, np.uint64))
    d_out = _dev64(torch, np.full(T, P64, np.uint64))
    d_groups = _dev32(torch, np.full(limit, P32, np.uint32), guard=0x3C3C3C3C)
    p = lambda t: t.data_ptr()
    kg.check(kg.group_best(p(d_sc), p(d_gid), n, row_base, n_groups, p(d_best), p(d_hist)))
    torch.cuda.synchronize()
    best = _np64(d_best)
    kg.check(kg.group_heads(p(d_sc), p(d_gid), p(d_best), n, row_base, n_groups, limit,
                            p(d_lists)))
    kg.check(kg.merge(p(d_lists), L, limit, 0, 1, limit, limit, p(d_heads)))
    kg.check(kg.group_members(p(d_sc), p(d_gid), p(d_best), n, row_base, n_groups, p(d_heads),
                              limit, S, p(d_lists), p(d_groups)))
    kg.check(kg.merge(p(d_lists), L, T, S, limit, S, S, p(d_out)))
    kg.check(kg.group_clear(p(d_best), n_groups))
    torch.cuda.synchronize()
    # extents
    assert np.all(best[n_groups:] == P64) and np.all(_np64(d_best)[n_groups:] == P64)
    assert np.all(_np64(d_lists)[L * T:] == P64)
    assert np.all(_np64(d_heads)[limit:] == P64)
    assert np.all(_np64(d_out)[T:] == P64)
    assert np.all(_np32(d_groups)[limit:] == 0x3C3C3C3C)
    assert np.all(_np32(d_hist)[kg.rsel_bins:] == P32)
    # inputs untouched, scratch handed back zeroed
    assert np.array_equal(_np32(d_sc)[:n], sc) and np.array_equal(_np32(d_gid)[:n], gor)
    assert not _np64(d_best)[:n_groups].any(), "best is not zero after the run"
    assert not _np32(d_hist)[:kg.rsel_bins].any(), "the histogram is not zero after the run"
    return (best[:n_groups], _np64(d_heads)[:limit], _np32(d_groups)[:limit],
            _np64(d_out)[:T].reshape(limit, S))


def check_case(kg, torch, sc, gor, n_groups, limit, S, row_base):
    best, heads, groups, out = run_stages(kg, torch, sc, gor, n_groups, limit, S, row_base)
    ranking = G.ranking_of_images(sc, row_base)
    # best: every group's largest key
    want_best = np.zeros(n_groups, np.uint64)
    g_of_key = gor[(G.key_rows(ranking) - np.uint64(row_base)).astype(np.int64)]
    on = g_of_key != NONE
    np.maximum.at(want_best, g_of_key[on].astype(np.int64), ranking[on])
    assert np.array_equal(best, want_best)
    ref = G.groups_ref(ranking, gor, limit, S, row_base)
    w_groups, w_hits, w_keys, count = G.as_arrays(ref, limit, S)
    assert np.array_equal(heads[:count], w_keys[:count, 0]) and not heads[count:].any()
    assert np.array_equal(groups[:count], w_groups[:count])
    assert np.all(groups[count:] == NONE)
    assert np.array_equal(out, w_keys)
    return count, w_hits


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_layouts(kg, torch_, n, name):
    rng = np.random.default_rng(1000 * n + LAYOUTS.index(name))
    gor, ng = layout(name, n, rng)
    row_base = [0, 1000, 0xFFFFFFFF - n - 1][(n + LAYOUTS.index(name)) % 3]
    for kind in ("few", "random"):
        sc = images(kind, n, gor, rng)
        for limit, S in ((1, 1), (5, 3), (128, 16)):
            count, hits = check_case(kg, torch_, sc, gor, ng, limit, S, row_base)
            if name == "one_group":
                assert count <= 1
            if name == "own_group":
                assert np.all(hits[:count] == 1)  # group_size above a group's members


def test_limit_above_the_groups_and_size_above_the_members(kg, torch_):
    rng = np.random.default_rng(7)
    n = 1500
    gor = np.repeat(np.arange(3, dtype=np.uint32), 500)
    gor[rng.integers(0, n, 100)] = NONE
    gor[1000:] = 2
    gor[1003:] = NONE  # group 2 has exactly 3 members
    sc = images("random", n, np.full(n, NONE, np.uint32), rng)
    sc[1000:1003] = G.score_image(np.array([0.1, 0.2, 0.3], np.float32))
    count, hits = check_case(kg, torch_, sc, gor, 7, 128, 16, 5)
    assert count == 3 and sorted(hits[:3]) == [3, 16, 16]


def test_nothing_eligible(kg, torch_):
    n = 3000
    gor = np.full(n, NONE, np.uint32)
    sc = images("random", n, gor, np.random.default_rng(3))
    assert check_case(kg, torch_, sc, gor, 4, 5, 3, 0)[0] == 0
    gor = np.zeros(n, np.uint32)
    assert check_case(kg, torch_, np.zeros(n, np.uint32), gor, 1, 5, 3, 0)[0] == 0


def test_ids_out_of_range_are_no_group(kg, torch_):
    """An id >= n_groups never indexes best (vs_grouping_create refuses such a
    grouping; the kernels do not depend on that)."""
    rng = np.random.default_rng(11)
    n = 5000
    gor, ng = layout("runs", n, rng)
    sc = images("random", n, gor, rng)
    cut = ng // 2
    best, heads, groups, out = run_stages(kg, torch_, sc, gor, cut, 16, 4, 0)
    masked = np.where(gor >= cut, NONE, gor).astype(np.uint32)
    ref = G.groups_ref(G.ranking_of_images(sc, 0), masked, 16, 4, 0)
    w_groups, _, w_keys, count = G.as_arrays(ref, 16, 4)
    assert np.array_equal(out, w_keys) and np.array_equal(groups[:count], w_groups[:count])


@pytest.mark.parametrize("name", ["one_group", "own_group"])
def test_flush_inside_the_loop(kg, torch_, name):
    n = 1_700_003
    rng = np.random.default_rng(5)
    if name == "own_group":
        gor, ng = np.arange(n, dtype=np.uint32), n
    else:
        gor, ng = np.zeros(n, np.uint32), 1
    sc = images("ascending", n, gor, rng)
    assert kg.group_lists(n) == kg.max_lists and n > 3 * 1024 * kg.max_lists
    count, hits = check_case(kg, torch_, sc, gor, ng, 128, 16, 17)
    assert count == (128 if name == "own_group" else 1)
    assert hits[0] == (1 if name == "own_group" else 16)
