"""(GPU) The plain one-query scan of csrc/vs_kernels.hip, each launcher on
inputs of the test's own through tests/kprobe, against tests/gemv_ref.py (a
numpy reference that knows keys, top-k and which workgroup walks a row, and
nothing about lanes):

  launch_gemv          gemv_topk_kernel at all ten compiled dimensions and
                       gemv_topk_generic_kernel (100, 8, 772), both dtypes:
                       every workgroup's (k <= 128) or wave's (k > 128) own
                       list against the top k of the rows it walks, and the
                       merge of the lists against the top k of all rows;
                       once more with about 70 rows a wave (deep lists);
  launch_gemv (rows)   the gathered instantiations, on row lists that
                       launch_compact_rows made and on hand-made ones;
  launch_gemv_one      lists bit for bit those of launch_query_prep +
                       launch_gemv, from a device query and from one in the
                       kernel arguments; its refusals;
  launch_gemv_small    the k final keys, one workgroup and partitioned: the
                       `part` lists, `counter` left zero, a second launch on
                       the same buffers; its refusals;
  launch_compact_rows  against np.flatnonzero, up to the last size of one
                       chunk of 256 block counts (4,194,304 rows) and past it,
                       where compact_scan_kernel's second chunk starts from
                       the first one's carry;
  the engine           3,000 rows at 2048, 3072 and 4096 against the oracle.

Before these tests no test, fuzz case or benchmark ran the scan at a
dimension above 1536, and no filtered collection was large enough for the
compaction's carry.

Exact data (integers in [-3, 3]: every partial sum in any order is an exact
fp32 integer) has to come back bit for bit, one-hot data names the column a
wrong score was read from, real data (generator rows, a query of length 1.3)
is held to the project's bar |s - fp64 dot| <= 1e-5 |dot| + 1e-6. Every
buffer carries a poisoned guard tail that is checked after the launch.

Mutations each tried once on a scratch build (values only, never an address,
a bound or a loop count), and what they showed:
  * gemv_emit counting ties for the waves after its own (`>=` in the search
    when ow > w, which places a key one slot down per tied key): NOT seen, and
    equivalent: the keys of a scan are distinct (distinct rows) and a zero
    never compares >= a nonzero key, so no tie exists to count. The blunt
    form, `r += pos + 1` for every ow > w, fails everything that goes through
    gemv_emit: test_gemv_lists (all 26), test_gemv_deep_lists, test_gemv_one,
    test_gemv_gathered, and test_gemv_small on real data (its reference is
    the three-launch chain).
  * `top` starting at 2: NOT seen, and equivalent: for k >= 2 the loop ends
    at the same power of two, and at k = 1 the first step (st = 2) is refused
    by `pos + st <= k`, after which st = 1 does what top = 1 did. A search
    that starts too low instead (`while (top * 4 <= k)`: half the power of
    two) was first seen only by chance (2 of 3 shapes, 2-3 entries): up to
    12,288 rows a wave walks two steps and its list holds a handful of
    keys, and on evenly spread data no wave holds many of its workgroup's
    best. test_gemv_deep_lists was added for it (about 70 rows a wave, the
    best rows of a workgroup in one wave's hands); it now fails at all three
    of its shapes.
  * make_key without the -0.0 fold (for the kernels of vs_kernels.hip): NOT
    seen, and unreachable in this family: the fp32 chunk_dot does start from
    a product, and a zero row under a negative query does give it -0.0, but
    every row sum is accumulated into `p = 0.f` (gemv_topk_body,
    gemv_small_body and the generic kernel alike), +0 + -0 is +0 in round to
    nearest, a sum that is not -0 never becomes -0 by adding, and wave_sum
    adds numbers none of which is -0. The tests still pin what a caller
    sees: the all-zero rows of the negative-query corpus come back with the
    key of +0.0, between the positive and the negative scores. The fold
    itself is held on the CPU (test_gemv_ref.py, against the oracle's order).
  * compact_scan_kernel not adding `carry`: test_compact_rows[4195082] fails
    at its first bitmap (row 0 of the list is 4,194,304: the second chunk's
    blocks start from 0 again). n = 4,194,304 passes either way: it is
    exactly 256 blocks, the last size of one chunk; only sizes past it run
    the second.
  * gemv_small's last workgroup ranking with `>=`: every partitioned launch of
    test_gemv_small fails at entry 0 (all 14 cases; the one-workgroup launches
    pass).
"""
import ctypes

import numpy as np
import pytest

import gemv_ref as GR
import q8_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
P32 = 0x5A5A5A5A
P64 = 0x5A5A5A5A5A5A5A5A
U64 = np.uint64

N_MAX = 4103
NS = (1, 2, 63, 64, 65, 257, 4103)
KS = (1, 10, 64, 65, 128, 129, 1000, 1024)
GENERIC_DIMS = (100, 8, 772)
ALLOWS = ("none", "half", "one row", "no row")


@pytest.fixture(scope="module")
def kp():
    import kprobe
    return kprobe.load()


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def _i64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(DEV)


def _np64(t):
    return t.cpu().numpy().view(np.uint64)


def _rows_dev(torch, X, bf16):
    if bf16:
        return torch.from_numpy(q8_ref.bf16_bits(X).view(np.int16)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(DEV)


def _f32_dev(torch, q):
    return torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)


def _row_bases(n):
    return (0, 12345, 0xFFFFFFFE - n)


def _masks(n, rng):
    """The four filters at n rows, by ALLOWS' names: None or bool[n]."""
    one = np.zeros(n, bool)
    one[n // 2] = True
    return {"none": None, "half": rng.random(n) < 0.5, "one row": one, "no row": np.zeros(n, bool)}


class Data:
    """One kind of rows for one (dim, dtype): on the device, with the query
    launch_gemv takes as given and every row's reference score (exact fp32 for
    `exact` and `onehot`, fp64 for `real`)."""

    def __init__(self, torch, kind, X, q, s, bf16, q_raw=None):
        self.kind, self.n, self.s = kind, X.shape[0], s
        self.Xd, self.qd = _rows_dev(torch, X, bf16), _f32_dev(torch, q)
        self.q_raw = q if q_raw is None else q_raw  # what the one-launch forms take


@pytest.fixture(scope="module")
def corpus(orc, torch_):
    """(dim, bf16) -> {kind: Data}; the last two shapes stay cached (the tests
    run shape by shape), each built and uploaded once."""
    cache = {}

    def get(dim, bf16):
        if (dim, bf16) in cache:
            return cache[(dim, bf16)]
        while len(cache) >= 2:
            cache.pop(next(iter(cache)))
        torch_.cuda.empty_cache()
        q = GR.exact_query(dim)
        X = GR.exact_rows(N_MAX, q)
        out = {"exact": Data(torch_, "exact", X, q, GR.exact_scores(X, q), bf16)}
        qn = GR.exact_query(dim, negative=True)
        X = GR.exact_rows(65, qn)
        X[40] = 0  # a second all-zero row, in another step
        out["neg"] = Data(torch_, "exact", X, qn, GR.exact_scores(X, qn), bf16)
        out["onehot"] = Data(torch_, "onehot", GR.onehot_rows(N_MAX, dim), GR.onehot_query(dim),
                             GR.onehot_scores(N_MAX, dim), bf16)
        X = GR.real_rows(orc, N_MAX, dim, bf16)
        q_raw = GR.real_query(orc, dim)
        qp = orc.preprocess(q_raw[None], False, bool(bf16))[0]  # dot: rounded to the dtype, not normalised
        out["real"] = Data(torch_, "real", X, qp, X.astype(np.float64) @ qp.astype(np.float64), bf16,
                           q_raw=q_raw)
        cache[(dim, bf16)] = out
        return out
    return get


# ---- launching -------------------------------------------------------------------------
def _scan(kp, torch, how, Xd, bf16, dim, n, row_base, q, k, allow=0, rows=0, cosine=0):
    """One scan launch -> (the lists on the device [maxl * k + GUARD], nlists).
    how: "gemv" (q: device, preprocessed), "gather" (rows: device row list),
    "one" (q: device, raw), "one_host" (q: numpy, raw)."""
    maxl = kp.gemv_max_lists(dim, bf16, n, k)
    lists = torch.full((maxl * k + GUARD,), P64, dtype=torch.int64, device=DEV)
    nl = ctypes.c_uint32(0)
    if how == "gemv":
        rc = kp.gemv(Xd.data_ptr(), bf16, dim, n, row_base, q.data_ptr(), k, lists.data_ptr(), maxl,
                     ctypes.byref(nl), allow)
    elif how == "gather":
        rc = kp.gemv_gather(Xd.data_ptr(), bf16, dim, n, row_base, q.data_ptr(), k, lists.data_ptr(),
                            maxl, ctypes.byref(nl), rows)
    elif how == "one":
        rc = kp.gemv_one(Xd.data_ptr(), bf16, dim, n, row_base, q.data_ptr(), cosine, allow, k,
                         lists.data_ptr(), maxl, ctypes.byref(nl))
    else:
        rc = kp.gemv_one_host(Xd.data_ptr(), bf16, dim, n, row_base, q.ctypes.data, cosine, allow, k,
                              lists.data_ptr(), maxl, ctypes.byref(nl))
    kp.check(rc)
    torch.cuda.synchronize()
    assert 1 <= nl.value <= maxl, ("nlists", nl.value, "gemv_max_lists", maxl)
    assert bool((lists[nl.value * k:] == P64).all()), "wrote past the lists it reported"
    return lists, nl.value


def _merge(kp, torch, lists, nl, k):
    out = torch.full((k + GUARD,), P64, dtype=torch.int64, device=DEV)
    kp.check(kp.merge(lists.data_ptr(), nl, k, 0, 1, k, k, out.data_ptr()))
    torch.cuda.synchronize()
    o = _np64(out)
    assert np.all(o[k:] == P64), "merge wrote past out[k]"
    return o[:k].copy()


def _host_lists(lists, nl, k):
    return _np64(lists[:nl * k]).reshape(nl, k)


def _check_sorted(L, what):
    nz = L != 0
    assert np.all(nz[:, :-1] | ~nz[:, 1:]), (what, "a key after a zero")
    assert np.all((L[:, :-1] > L[:, 1:]) | ~nz[:, 1:]), (what, "a list is not strictly descending")


def _wave_of(kp, dim, bf16, n, nl, per_wave, pos):
    """The wave that walks position pos of a scan over [0, n) which reported nl lists."""
    if dim in GR.TABLE_DIMS:
        nwaves = nl if per_wave else nl * GR.WAVES
        return GR.owner_wave(pos, GR.rows_per_step(dim, bf16), nwaves)
    nwg, rpw = GR.slice_grid(n, kp.device_cu_count())
    assert nl == nwg * (GR.WAVES if per_wave else 1), ("lists of a sliced scan", nl, nwg)
    return GR.owner_slice_wave(pos, rpw)


def _want_lists(kp, dim, bf16, n, k, nl, pos, keys):
    """The lists of a scan over positions [0, n): keys[i] is the key of
    position pos[i]. One list per workgroup up to k = 128, per wave past it."""
    per_wave = k > 128
    wave = _wave_of(kp, dim, bf16, n, nl, per_wave, pos)
    return GR.topk_lists(keys, wave if per_wave else wave // GR.WAVES, nl, k)


def _first_diff(got, want):
    bad = np.nonzero(got != want)
    return tuple(int(x[0]) for x in bad), int(bad[0].size)


def _check_exact(kp, torch, D, dim, bf16, n, k, row_base, lists, nl, pos, local, what):
    """Lists and merge of a scan whose position pos[i] is local row local[i]
    with reference score D.s[local[i]] (every unmasked position listed)."""
    keys = GR.make_key(D.s[local], local.astype(U64) + U64(row_base))
    L = _host_lists(lists, nl, k)
    _check_sorted(L, what)
    want = _want_lists(kp, dim, bf16, n, k, nl, pos, keys)
    if not np.array_equal(L, want):
        at, cnt = _first_diff(L, want)
        g, w = int(L[at]), int(want[at])
        msg = (what, "list, entry", at, "got", hex(g), "want", hex(w), "entries differing", cnt)
        if D.kind == "onehot" and g:
            r = int(GR.key_row(g)) - row_base
            msg += ("row", r, "read column", GR.onehot_column(GR.key_score(g)), "its own", r % dim)
        raise AssertionError(msg)
    got = _merge(kp, torch, lists, nl, k)
    want = GR.topk_keys(D.s[local], local, row_base, k)
    if not np.array_equal(got, want):
        at, cnt = _first_diff(got, want)
        g = int(got[at])
        msg = (what, "merge, entry", at, "got", hex(g), "want", hex(int(want[at])), "differing", cnt)
        if D.kind == "onehot" and g:
            r = int(GR.key_row(g)) - row_base
            msg += ("row", r, "read column", GR.onehot_column(GR.key_score(g)), "its own", r % dim)
        raise AssertionError(msg)


def _check_real(kp, torch, D, k, row_base, lists, nl, local, what):
    """The merged answer over the local rows `local` of real data: as many keys
    as there are rows (up to k), distinct listed rows, every score within the
    bar of its row's fp64 dot, and the i-th score within the bar of the i-th
    largest fp64 dot by the largest bar among the listed rows (if every row's
    score is within e of its dot, so are the order statistics; a missing top
    row shifts every rank below it by a gap far above 1e-5 on this data)."""
    _check_sorted(_host_lists(lists, nl, k), what)
    got = _merge(kp, torch, lists, nl, k)
    m = min(k, local.size)
    assert np.all(got[:m] != 0) and not got[m:].any(), (what, "count")
    if m == 0:
        return
    rows = GR.key_row(got[:m]) - row_base
    assert np.unique(rows).size == m and np.all(np.isin(rows, local)), (what, "rows")
    sc = GR.key_score(got[:m]).astype(np.float64)
    err = np.abs(sc - D.s[rows]) - GR.bar(D.s[rows])
    assert np.all(err <= 0), (what, "row", int(rows[np.argmax(err)]), "over the bar by", float(err.max()))
    true = np.sort(D.s[local])[::-1][:m]
    err = np.abs(sc - true) - GR.bar(D.s[local]).max()
    assert np.all(err <= 0), (what, "rank", int(np.argmax(err)), "over the bar by", float(err.max()))


# ---- launch_gemv, ungathered ----------------------------------------------------------------
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("dim", GR.TABLE_DIMS + GENERIC_DIMS)
def test_gemv_lists(kp, torch_, corpus, dim, bf16):
    C = corpus(dim, bf16)
    rng = np.random.default_rng(dim * 2 + bf16)
    ci = 0
    for n in NS:
        masks = _masks(n, rng)
        allow_dev = {a: (None if m is None else _i64(torch_, GR.pack_bits(m))) for a, m in masks.items()}
        for ki, k in enumerate(KS):
            # exact data under every filter; one-hot and real under one filter each, in turn
            plan = [("exact", a) for a in ALLOWS]
            plan += [("onehot", ALLOWS[ki % 2]), ("real", ALLOWS[(ki + n) % 3])]
            for kind, a in plan:
                row_base = _row_bases(n)[(ci + ci // len(plan)) % 3]  # each slot of the plan meets all three
                ci += 1
                D, mask = C[kind], masks[a]
                what = (kind, dim, bf16, "n", n, "k", k, "row_base", row_base, "allow", a)
                ap = 0 if mask is None else allow_dev[a].data_ptr()
                lists, nl = _scan(kp, torch_, "gemv", D.Xd, bf16, dim, n, row_base, D.qd, k, allow=ap)
                local = np.arange(n) if mask is None else np.nonzero(mask)[0]
                if kind == "real":
                    _check_real(kp, torch_, D, k, row_base, lists, nl, local, what)
                else:
                    _check_exact(kp, torch_, D, dim, bf16, n, k, row_base, lists, nl, local, local, what)
                if a == "no row":
                    assert not _np64(lists[:nl * k]).any(), (what, "a key with no row allowed")
    # the sign of zero: all-zero rows under an all-negative query (every product is -0.0)
    D = C["neg"]
    for k in (1, 10, 65, 129):
        what = ("negative query", dim, bf16, "k", k)
        lists, nl = _scan(kp, torch_, "gemv", D.Xd, bf16, dim, D.n, 7, D.qd, k)
        _check_exact(kp, torch_, D, dim, bf16, D.n, k, 7, lists, nl, np.arange(D.n), np.arange(D.n), what)
        zero = GR.make_key(np.float32(0), U64(7))
        got = _merge(kp, torch_, lists, nl, k)
        if k >= D.n:
            assert int(zero) in [int(x) for x in got], (what, "the zero row's key is not that of +0.0")


@pytest.mark.parametrize("dim,bf16", [(128, 1), (8, 0), (8, 1)])
def test_gemv_deep_lists(kp, torch_, dim, bf16):
    """Up to 12,288 rows a wave walks two steps, so its list holds a handful of
    keys and gemv_emit's search never goes deep. Here every wave of the device
    walks about 70 rows (430,087 rows on 256 CUs), and in every workgroup one
    wave -- the first in one workgroup, the second in the next, ... -- walks
    the rows that score high (the query with a few entries zeroed, from 40
    patterns: ties), the others random rows. That wave's list is full at k =
    64 and holds more than 64 keys at k = 128, nearly all of them the
    workgroup's best: the other waves' keys are placed below them by a search
    that runs its full depth, and keys past k are cut in the merge. One narrow
    table shape and the generic kernel (its rows are 32 and 16 bytes)."""
    n = kp.device_cu_count() * 3 * GR.WAVES * 70 + 7
    q = GR.exact_query(dim, seed=1)
    rng = np.random.default_rng([dim, bf16])
    zeros = torch_.zeros((n * dim,), dtype=torch_.int16 if bf16 else torch_.float32, device=DEV)
    _, nwg = _scan(kp, torch_, "gemv", zeros, bf16, dim, n, 0, _f32_dev(torch_, q), 1)  # the grid only
    del zeros
    wave = _wave_of(kp, dim, bf16, n, nwg, False, np.arange(n))
    assert n / (nwg * GR.WAVES) > 64, "a wave has to walk more than 64 rows"
    hot = wave % GR.WAVES == (wave // GR.WAVES) % GR.WAVES
    assert np.bincount(wave[hot]).max() > 64
    X = rng.integers(-GR.EXACT_MAX, GR.EXACT_MAX + 1, size=(n, dim)).astype(np.float32)
    patterns = q * (rng.random((40, dim)) < 0.85)
    X[hot] = patterns[rng.integers(0, 40, int(hot.sum()))]
    D = Data(torch_, "exact", X, q, GR.exact_scores(X, q), bf16)
    local = np.arange(n)
    for i, k in enumerate((10, 64, 65, 100, 128, 129)):
        row_base = (0, 12345, 0xFFFFFFFE - n)[i % 3]
        what = ("deep", dim, bf16, "k", k, "row_base", row_base)
        lists, nl = _scan(kp, torch_, "gemv", D.Xd, bf16, dim, n, row_base, D.qd, k)
        _check_exact(kp, torch_, D, dim, bf16, n, k, row_base, lists, nl, local, local, what)


# ---- launch_gemv over a row list --------------------------------------------------------------
def _hand_list(ng, rng):
    if ng == 1:
        return np.array([N_MAX - 1], np.uint32)
    must = np.array([0, 1, 2, N_MAX - 1][:min(ng, 4)])
    rest = rng.choice(np.arange(3, N_MAX - 1), ng - must.size, replace=False)
    return np.sort(np.concatenate([must, rest])).astype(np.uint32)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("dim", [128, 768, 2048, 4096, 100])
def test_gemv_gathered(kp, torch_, corpus, dim, bf16):
    C = corpus(dim, bf16)
    rng = np.random.default_rng(dim + bf16)
    ci = 0
    for ng in (1, 3, 65, 513):
        # the same kind of list twice: made on the device from a bitmap, and by hand
        m = np.zeros(N_MAX, bool)
        m[rng.choice(N_MAX, ng, replace=False)] = True
        words = _i64(torch_, GR.pack_bits(m))
        sw = kp.compact_scratch_words(N_MAX)
        rows_c = torch_.full((ng + GUARD,), P32, dtype=torch_.int32, device=DEV)
        scratch = torch_.full((sw + GUARD,), P32, dtype=torch_.int32, device=DEV)
        kp.check(kp.compact_rows(words.data_ptr(), N_MAX, rows_c.data_ptr(), scratch.data_ptr()))
        torch_.cuda.synchronize()
        got = rows_c.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:ng], np.nonzero(m)[0]) and np.all(got[ng:] == P32), ("compact", ng)
        hand = _hand_list(ng, rng)
        rows_h = torch_.from_numpy(hand.view(np.int32)).to(DEV)
        for src, rd, local in (("compacted", rows_c, np.nonzero(m)[0]), ("hand", rows_h, hand.astype(np.int64))):
            for k in (1, 100, 1024):
                for kind in ("exact", "real"):
                    row_base = (12345, 0xFFFFFFFE - N_MAX, 1)[ci % 3]
                    ci += 1
                    D = C[kind]
                    what = (kind, "gathered", src, dim, bf16, "rows", ng, "k", k, "row_base", row_base)
                    lists, nl = _scan(kp, torch_, "gather", D.Xd, bf16, dim, ng, row_base, D.qd, k,
                                      rows=rd.data_ptr())
                    if kind == "real":
                        _check_real(kp, torch_, D, k, row_base, lists, nl, local, what)
                    else:
                        _check_exact(kp, torch_, D, dim, bf16, ng, k, row_base, lists, nl, np.arange(ng),
                                     local, what)


# ---- launch_gemv_one ---------------------------------------------------------------------
def _prep(kp, torch, q_raw_d, dim, cosine, bf16):
    qp = torch.full((dim + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    kp.check(kp.query_prep(q_raw_d.data_ptr(), 1, dim, cosine, bf16, qp.data_ptr(), 0))
    torch.cuda.synchronize()
    assert bool((qp[dim:] == 7.0).all())
    return qp


ONE_DIMS = (128, 256, 384, 512, 768, 1024)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("dim", ONE_DIMS)
def test_gemv_one(kp, torch_, corpus, dim, bf16):
    C = corpus(dim, bf16)
    rng = np.random.default_rng(dim * 2 + bf16 + 1)
    assert all(kp.gemv_one_ok(dim, k) for k in (1, 64, 65, 128))
    ci = 0
    for cosine, kind in ((0, "exact"), (0, "real"), (1, "real")):
        D = C[kind]
        q_raw = np.ascontiguousarray(D.q_raw, np.float32)
        q_raw_d = _f32_dev(torch_, q_raw)
        qp = _prep(kp, torch_, q_raw_d, dim, cosine, bf16)
        if kind == "exact":  # integers: the dot metric's preparation leaves them as they are
            assert np.array_equal(qp[:dim].cpu().numpy(), q_raw)
        for n in (1, 65, N_MAX):
            masks = _masks(n, rng)
            for k in (1, 64, 65, 128):
                for how in ("one", "one_host")[:2 if dim <= kp.gemv_small_arg_dim else 1]:
                    a = ALLOWS[ci % 4]
                    row_base = _row_bases(n)[ci % 3]
                    ci += 1
                    mask = masks[a]
                    allow = None if mask is None else _i64(torch_, GR.pack_bits(mask))
                    ap = 0 if mask is None else allow.data_ptr()
                    what = (how, kind, "cosine", cosine, dim, bf16, "n", n, "k", k, "row_base", row_base,
                            "allow", a)
                    lists, nl = _scan(kp, torch_, how, D.Xd, bf16, dim, n, row_base,
                                      q_raw_d if how == "one" else q_raw, k, allow=ap, cosine=cosine)
                    ref, nlr = _scan(kp, torch_, "gemv", D.Xd, bf16, dim, n, row_base, qp, k, allow=ap)
                    assert nl == nlr, (what, "lists", nl, nlr)
                    L, Lr = _host_lists(lists, nl, k), _host_lists(ref, nlr, k)
                    assert np.array_equal(L, Lr), (what, "differs from query prep + gemv at",
                                                   _first_diff(L, Lr))
                    if kind == "exact":
                        local = np.arange(n) if mask is None else np.nonzero(mask)[0]
                        _check_exact(kp, torch_, D, dim, bf16, n, k, row_base, lists, nl, local, local, what)


def test_gemv_one_refuses(kp, torch_, corpus):
    """By return value only: the argument checks come before any launch."""
    D = corpus(128, 0)["exact"]
    q = np.ascontiguousarray(D.q_raw, np.float32)
    qd = _f32_dev(torch_, q)
    lists = torch_.full((4096,), P64, dtype=torch_.int64, device=DEV)
    nl = ctypes.c_uint32(0)
    X = D.Xd.data_ptr()
    assert not kp.gemv_one_ok(1536, 10) and not kp.gemv_one_ok(128, 129) and not kp.gemv_one_ok(128, 0)
    assert kp.gemv_one(X, 0, 1536, 8, 0, qd.data_ptr(), 0, 0, 10, lists.data_ptr(), 16, ctypes.byref(nl)) != 0
    assert kp.gemv_one(X, 0, 128, 8, 0, qd.data_ptr(), 0, 0, 129, lists.data_ptr(), 16, ctypes.byref(nl)) != 0
    assert kp.gemv_one(X, 0, 128, 0, 0, qd.data_ptr(), 0, 0, 10, lists.data_ptr(), 16, ctypes.byref(nl)) != 0
    q1024 = np.zeros(1024, np.float32)
    assert kp.gemv_one_host(X, 0, 1024, 8, 0, q1024.ctypes.data, 0, 0, 10, lists.data_ptr(), 16,
                            ctypes.byref(nl)) != 0
    torch_.cuda.synchronize()
    assert bool((lists == P64).all()) and nl.value == 0


# ---- launch_gemv_small ------------------------------------------------------------------------
SMALL_DIMS = (128, 256, 384, 512, 768, 1024, 1536)


def _small(kp, torch, D, bf16, dim, n, row_base, q_raw_d, q_host, cosine, k, part, counter):
    out = torch.full((k + GUARD,), P64, dtype=torch.int64, device=DEV)
    kp.check(kp.gemv_small(D.Xd.data_ptr(), bf16, dim, n, row_base, q_raw_d.data_ptr(), cosine, k,
                           out.data_ptr(), 0 if part is None else part.data_ptr(),
                           0 if counter is None else counter.data_ptr(),
                           0 if q_host is None else q_host.ctypes.data))
    torch.cuda.synchronize()
    o = _np64(out)
    assert np.all(o[k:] == P64), "wrote past out[k]"
    return o[:k].copy()


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("dim", SMALL_DIMS)
def test_gemv_small(kp, torch_, corpus, dim, bf16):
    C = corpus(dim, bf16)
    maxp, maxk = kp.gemv_small_max_parts, kp.gemv_small_max_k
    assert (kp.gemv_small_max_rows, maxk, maxp, kp.gemv_small_arg_dim) == (256, 16, 16, 768)
    RB = GR.rows_per_step(dim, bf16)
    ci = 0
    for cosine, kind in ((0, "exact"), (0, "neg"), (0, "real"), (1, "real")):
        D = C[kind]
        q_raw = np.ascontiguousarray(D.q_raw, np.float32)
        q_raw_d = _f32_dev(torch_, q_raw)
        qp = _prep(kp, torch_, q_raw_d, dim, cosine, bf16)
        for n in (1, 5, 31, 32, 33, 221, 256):
            if n > D.n:
                continue  # the negative-query corpus has 65 rows
            parts = kp.gemv_small_parts(dim, bf16, n)
            assert 1 <= parts <= maxp and kp.gemv_small_ok(dim, n, 16)
            for k in (1, 5, 16):
                row_base = (_row_bases(n) + (77,))[ci % 4]
                ci += 1
                if kind == "real":  # query prep + gemv + merge, bit for bit
                    ref, nlr = _scan(kp, torch_, "gemv", D.Xd, bf16, dim, n, row_base, qp, k)
                    want = _merge(kp, torch_, ref, nlr, k)
                else:
                    want = GR.topk_keys(D.s[:n], np.arange(n), row_base, k)
                for host in (False, True)[:2 if dim <= kp.gemv_small_arg_dim else 1]:
                    what = (kind, "cosine", cosine, dim, bf16, "n", n, "k", k, "row_base", row_base,
                            "q in the arguments" if host else "q on the device")
                    qh = q_raw if host else None
                    got = _small(kp, torch_, D, bf16, dim, n, row_base, q_raw_d, qh, cosine, k, None, None)
                    assert np.array_equal(got, want), (what, "one workgroup", _first_diff(got, want))
                    # partitioned: the same keys; each part its owner's top k; counter left zero
                    part = torch_.full((maxp * maxk + GUARD,), P64, dtype=torch_.int64, device=DEV)
                    counter = torch_.full((1 + GUARD,), P32, dtype=torch_.int32, device=DEV)
                    counter[0] = 0
                    for launch in (1, 2):
                        got = _small(kp, torch_, D, bf16, dim, n, row_base, q_raw_d, qh, cosine, k, part,
                                     counter)
                        assert np.array_equal(got, want), (what, "partitioned, launch", launch,
                                                           _first_diff(got, want))
                        c = counter.cpu().numpy().view(np.uint32)
                        assert c[0] == 0 and np.all(c[1:] == P32), (what, "counter", int(c[0]), "launch", launch)
                        p = _np64(part)
                        used = parts * k if parts > 1 else 0  # one workgroup writes `out` itself
                        assert np.all(p[used:] == P64), (what, "more than gemv_small_parts lists", parts)
                        if parts > 1:
                            P = p[:used].reshape(parts, k)
                            assert not np.any(P == P64), (what, "fewer than gemv_small_parts lists", parts)
                            _check_sorted(P, what)
                            if kind != "real":
                                keys = GR.make_key(D.s[:n], np.arange(n, dtype=U64) + U64(row_base))
                                wantp = GR.topk_lists(keys, GR.owner(np.arange(n), RB, parts * GR.WAVES),
                                                      parts, k)
                                assert np.array_equal(P, wantp), (what, "part", _first_diff(P, wantp))
                            else:  # the parts hold the answer between them, each key once
                                nzp = P[P != 0]
                                assert np.unique(nzp).size == nzp.size and np.all(np.isin(want[want != 0], nzp))


def test_gemv_small_refuses(kp, torch_, corpus):
    """By return value only: gemv_small_ok is checked before any launch."""
    D = corpus(128, 0)["exact"]
    qd = _f32_dev(torch_, D.q_raw)
    out = torch_.full((64,), P64, dtype=torch_.int64, device=DEV)
    X = D.Xd.data_ptr()
    assert not kp.gemv_small_ok(128, 257, 5) and not kp.gemv_small_ok(128, 5, 17)
    assert not kp.gemv_small_ok(2048, 5, 5) and not kp.gemv_small_ok(128, 0, 5)
    for dim, n, k in ((128, 257, 5), (128, 5, 17), (2048, 1, 5)):
        assert kp.gemv_small(X, 0, dim, n, 0, qd.data_ptr(), 0, k, out.data_ptr(), 0, 0, 0) != 0, (dim, n, k)
    torch_.cuda.synchronize()
    assert bool((out == P64).all())


# ---- launch_compact_rows ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 16384, 16385, 4_194_304, 4_194_305 + 777])
def test_compact_rows(kp, torch_, n):
    """One block count per 16384 rows, scanned 256 at a time: past 4,194,304
    rows the scan's second chunk starts from the first one's carry."""
    rng = np.random.default_rng(n)
    sw = kp.compact_scratch_words(n)
    assert sw == (n + 16383) // 16384
    for name, words in GR.compact_bitmaps(n, rng).items():
        want = GR.compact(words, n)
        allow = _i64(torch_, words)
        rows = torch_.full((want.size + GUARD,), P32, dtype=torch_.int32, device=DEV)
        scratch = torch_.full((sw + GUARD,), P32, dtype=torch_.int32, device=DEV)
        kp.check(kp.compact_rows(allow.data_ptr(), n, rows.data_ptr(), scratch.data_ptr()))
        torch_.cuda.synchronize()
        got = rows.cpu().numpy().view(np.uint32)
        assert np.all(got[want.size:] == P32), (n, name, "wrote past rows[popcount]")
        assert np.all(scratch.cpu().numpy().view(np.uint32)[sw:] == P32), (n, name, "wrote past the scratch")
        assert np.array_equal(_np64(allow), words), (n, name, "bitmap changed")
        bad = np.nonzero(got[:want.size] != want)[0]
        assert bad.size == 0, (n, name, "first wrong at", int(bad[0]), "got", int(got[bad[0]]), "want",
                               int(want[bad[0]]), "wrong", bad.size, "of", want.size)


# ---- the engine at the widths nothing else runs ------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("dim", [2048, 3072, 4096])
def test_engine_wide_dims(pkg, orc, dim, dtype):
    """search_core's own dispatch at 2048 / 3072 / 4096: the scan, its query
    preparation past 1536 and (k = 200) the large-k score pass."""
    n = 3000
    with pkg.VectorEngine(device=0) as eng:
        eng.create_collection("w", dim, 0, dtype)
        eng.generate("w", n, orc.SEED_CORPUS)
        X = orc.generate(orc.SEED_CORPUS, 0, n, dim, bf16=bool(dtype))
        Q = orc.generate(orc.SEED_QUERY, 11, 3, dim) * np.float32(1.7)
        Qp = orc.preprocess(Q, True, bool(dtype))
        for nq in (1, 3):
            for k in (10, 200):
                s, r, c = eng.search("w", Q[:nq], k)
                assert np.all(c == k)
                _, s64, rows, cnt = orc.search(X, Qp[:nq], k)
                bad = orc.check_topk(s, r, c, s64, rows, cnt, orc.rescore(X, Qp[:nq], r, c), 1e-5)
                assert not bad, (dim, dtype, nq, k, bad[:5])
