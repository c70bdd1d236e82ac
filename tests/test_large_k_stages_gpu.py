"""(GPU) The pieces around the large-k selection, each launcher on inputs of
the test's own through tests/kprobe (the selections themselves:
tests/test_rsel_stages_gpu.py):

  launch_gemv_scores     every row's score image and the first-digit histogram
                         against an fp64 dot, the numpy bincount, and the list
                         path's keys (launch_gemv + launch_merge) bit for bit;
  launch_sort_keys_desc  against np.sort;
  launch_merge_large     against np.unique, in both list layouts of the engine;
  launch_remap_keys      against its formula, up to row 2^32 - 1.

Mutations each tried once on a scratch build (values only, never an address
or a loop bound):
  * score bits: the score mode of gemv_topk_body / gemv_topk_generic_kernel
    forming its image from `s * 1.0000001f` -> the bit comparison with the
    list path fails at every size; the 1e-5 precision check does not see it;
  * sort merge: merge_unique_kernel ending its walk at the first chunk that
    keeps nothing (`if (total == 0) break`, as it did before) -> replicated
    lists with L = 300 return 6 of 8 keys (1 key at L = 512 and 1000, 6 of
    1100 at kin = 1100). L = 257 passes either way: a key's 257 slots cover a
    whole chunk and the slot before it only where they start one slot before
    a chunk, which is not among the first 8 keys.
"""
import ctypes

import numpy as np
import pytest

import q8_ref
import rsel_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
P32 = 0x5A5A5A5A
P64 = 0x5A5A5A5A5A5A5A5A
U64 = np.uint64


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


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _ord_score(o):
    o = np.asarray(o, np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return u.view(np.float32)


def _pack_allow(mask):
    n = mask.size
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = mask
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").ravel().view(np.uint64).copy()


# ---- launch_gemv_scores -------------------------------------------------------------
N_ROWS = (1, 63, 64, 65, 1000, 4103)  # 4103: odd, so no multiple of a wave's 2-, 4- or 8-row step


@pytest.fixture(scope="module")
def corpora(orc, torch_):
    """(dim, bf16) -> rows on the device in the collection dtype, the
    preprocessed query on the device, and every row's fp64 dot (computed once)."""
    cache = {}

    def get(dim, bf16):
        if (dim, bf16) not in cache:
            n = max(N_ROWS)
            X = orc.generate(orc.SEED_CORPUS, 0, n, dim, bf16=bool(bf16))
            q = orc.preprocess(orc.generate(orc.SEED_QUERY, 3, 1, dim) * 1.3, True, bool(bf16))[0]
            if bf16:
                Xd = torch_.from_numpy(q8_ref.bf16_bits(X).view(np.int16)).to(DEV)
            else:
                Xd = torch_.from_numpy(np.ascontiguousarray(X, np.float32)).to(DEV)
            qd = torch_.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
            cache[(dim, bf16)] = (Xd, qd, X.astype(np.float64) @ q.astype(np.float64))
        return cache[(dim, bf16)]
    return get


def _list_path_keys(kp, torch, Xd, bf16, dim, n, qd, allow_ptr):
    """Every row's key on the list path: launch_gemv with k = n, then launch_merge."""
    k = n
    maxl = kp.gemv_max_lists(dim, bf16, n, k)
    lists = torch.full((maxl * k + GUARD,), P64, dtype=torch.int64, device=DEV)
    out = torch.full((k + GUARD,), P64, dtype=torch.int64, device=DEV)
    nl = ctypes.c_uint32(0)
    kp.check(kp.gemv(Xd.data_ptr(), bf16, dim, n, 0, qd.data_ptr(), k, lists.data_ptr(), maxl,
                     ctypes.byref(nl), allow_ptr))
    assert 1 <= nl.value <= maxl
    kp.check(kp.merge(lists.data_ptr(), nl.value, k, 0, 1, k, k, out.data_ptr()))
    torch.cuda.synchronize()
    o = _np64(out)
    assert np.all(o[k:] == P64) and np.all(_np64(lists)[maxl * k:] == P64)
    return o[:k].copy()


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("dim", [768, 1024, 1536, 100, 2048, 3072, 4096])
def test_gemv_scores(kp, torch_, corpora, dim, bf16):
    Xd, qd, s64 = corpora(dim, bf16)
    rng = np.random.default_rng(dim + bf16)
    for n in N_ROWS:
        half = rng.random(n) < 0.5
        one = np.zeros(n, bool)
        one[n // 2] = True
        for ai, mask in enumerate((None, half, one)):
            what = (dim, bf16, n, ("all", "half", "one")[ai])
            live = np.ones(n, bool) if mask is None else mask
            allow = _i64(torch_, _pack_allow(mask)) if mask is not None else None
            ap = allow.data_ptr() if allow is not None else 0
            fill = 0 if (ai + n) % 2 else 7  # hist accumulates: from zero, and from a known fill
            sc = torch_.full((n + GUARD,), P32, dtype=torch_.int32, device=DEV)
            hist = torch_.full((kp.rsel_bins + GUARD,), P32, dtype=torch_.int32, device=DEV)
            hist[:kp.rsel_bins] = fill
            kp.check(kp.gemv_scores(Xd.data_ptr(), bf16, dim, n, qd.data_ptr(), ap, sc.data_ptr(),
                                    hist.data_ptr()))
            torch_.cuda.synchronize()
            o, h = _np32(sc), _np32(hist)
            assert np.all(o[n:] == P32), (what, "wrote past sc[n_rows]")
            assert np.all(h[kp.rsel_bins:] == P32), (what, "wrote past hist")
            o = o[:n]
            assert np.array_equal(o != 0, live), (what, "sc == 0 exactly at the masked rows")
            assert np.array_equal(h[:kp.rsel_bins], R.first_hist(o) + np.uint32(fill)), (what, "hist")
            # precision, every unmasked row: the project's bar
            s = _ord_score(o[live]).astype(np.float64)
            err = np.abs(s - s64[:n][live])
            tol = 1e-5 * np.abs(s64[:n][live]) + 1e-6
            assert np.all(err <= tol), (what, "row", int(np.nonzero(live)[0][np.argmax(err - tol)]),
                                        float(np.max(err - tol)))
            # bits: the list path's key of every row
            if n <= kp.max_k:
                keys = _list_path_keys(kp, torch_, Xd, bf16, dim, n, qd, ap)
                nz = keys[keys != 0]
                assert nz.size == int(live.sum()) and np.all(keys[nz.size:] == 0), (what, "list path count")
                rows = (U64(0xFFFFFFFF) - (nz & U64(0xFFFFFFFF))).astype(np.int64)
                assert np.array_equal(np.sort(rows), np.nonzero(live)[0]), (what, "list path rows")
                hi = (nz >> U64(32)).astype(np.uint32)
                bad = np.nonzero(o[rows] != hi)[0]
                assert bad.size == 0, (what, "row", int(rows[bad[0]]), hex(int(o[rows[bad[0]]])),
                                       hex(int(hi[bad[0]])), "rows differing", bad.size)


# ---- launch_sort_keys_desc ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 129, 4097, 100_000])
def test_sort_keys_desc(kp, torch_, n):
    rng = np.random.default_rng(n)
    full = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    full[0] = 0xFFFFFFFFFFFFFFFF
    full[-1] = 0
    same_hi = (U64(0xBF800000) << U64(32)) | rng.permutation(n).astype(U64)  # equal high words
    tb = kp.sort_keys_temp_bytes(n)
    for what, keys in (("full range", full), ("equal high word", same_hi)):
        src = _i64(torch_, keys)
        out = torch_.full((n + GUARD,), P64, dtype=torch_.int64, device=DEV)
        temp = torch_.full((tb + 8 * GUARD,), 0x5A, dtype=torch_.uint8, device=DEV)
        kp.check(kp.sort_keys_desc(src.data_ptr(), out.data_ptr(), n, temp.data_ptr(), tb))
        torch_.cuda.synchronize()
        o = _np64(out)
        assert np.all(o[n:] == P64), (what, "wrote past out[n]")
        assert np.all(temp.cpu().numpy()[tb:] == 0x5A), (what, "wrote past the temp storage")
        assert np.array_equal(_np64(src), keys), (what, "input changed")
        assert np.array_equal(o[:n], np.sort(keys)[::-1]), (what, n)


# ---- launch_merge_large --------------------------------------------------------------------
def _pool(rng, m):
    p = np.unique(rng.integers(1, 1 << 64, size=2 * m + 8, dtype=np.uint64))
    return rng.permutation(p)[:m]


def _fill(lists, l, q, keys):
    keys = np.sort(np.asarray(keys, np.uint64))[::-1][:lists.shape[2]]  # a sorted list, 0-padded
    lists[l, q, :keys.size] = keys


def _merge_case(name):
    """-> lists [L, nq, kin] uint64 (0 = empty entry), k."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one_list":
        lists = np.zeros((1, 1, 1500), U64)
        _fill(lists, 0, 0, _pool(rng, 1400))
        return lists, 1200
    if name == "kin_1":
        lists = np.zeros((40, 2, 1), U64)
        p = _pool(rng, 25)
        lists[:, 0, 0] = rng.choice(p, 40)
        lists[::3, 1, 0] = rng.choice(p, 14)
        return lists, 1100
    if name == "k_above_distinct":
        lists = np.zeros((4, 1, 100), U64)
        p = _pool(rng, 150)
        for l in range(4):
            _fill(lists, l, 0, rng.choice(p, 100, replace=False))
        return lists, 1100
    if name == "fill_per_query":  # full, half-empty lists, all zero
        lists = np.zeros((7, 3, 400), U64)
        p = _pool(rng, 3000)
        for l in range(7):
            _fill(lists, l, 0, rng.choice(p, 400, replace=False))
            _fill(lists, l, 1, rng.choice(p, int(rng.integers(0, 200)), replace=False))
        return lists, 1300
    if name == "disjoint":
        lists = np.zeros((6, 1, 300), U64)
        p = _pool(rng, 1800)
        for l in range(6):
            _fill(lists, l, 0, p[300 * l:300 * (l + 1)])
        return lists, 1100
    if name == "disjoint_k_above":
        lists, _ = _merge_case("disjoint")
        return lists, 2000
    if name == "heavy_overlap":
        lists = np.zeros((8, 2, 500), U64)
        for q in range(2):
            p = _pool(rng, 700)
            for l in range(8):
                _fill(lists, l, q, rng.choice(p, 500, replace=False))
        return lists, 1100
    if name.startswith("replicated_"):  # every list the same keys; query 1 (L = 300) its own
        _, L, kin = name.split("_")
        L, kin = int(L), int(kin)
        nq = 2 if L == 300 else 1
        lists = np.zeros((L, nq, kin), U64)
        for q in range(nq):
            one = np.zeros((1, 1, kin), U64)
            _fill(one, 0, 0, _pool(rng, kin - (3 if kin > 8 and q else 0)))
            lists[:, q, :] = one[0, 0]
        if kin == 8:
            # the defect this case is for: a key fills a whole 256-key chunk of the sorted segment
            assert L > 256 and np.unique(lists[:, 0, :]).size == 8
        return lists, 1100
    raise KeyError(name)


MERGE_CASES = ["one_list", "kin_1", "k_above_distinct", "fill_per_query", "disjoint", "disjoint_k_above",
               "heavy_overlap", "replicated_257_8", "replicated_300_8", "replicated_512_8",
               "replicated_1000_8", "replicated_300_1100"]


@pytest.mark.parametrize("name", MERGE_CASES)
def test_merge_large(kp, torch_, name):
    lists, k = _merge_case(name)
    L, nq, kin = lists.shape
    want = np.zeros((nq, k), U64)
    for q in range(nq):
        u = np.unique(lists[:, q, :][lists[:, q, :] != 0])[::-1][:k]
        want[q, :u.size] = u
    slots = kp.mfma_query_slots
    layouts = [("shard lists", nq * kin, kin)]
    if L * slots * kin * 8 <= 64 << 20:  # (the MFMA lists' layout at L = 300, kin = 1100 is 675 MB)
        layouts.append(("MFMA lists", slots * kin, kin))
    sb = kp.merge_large_scratch(L, nq, kin)
    assert sb % 8 == 0
    for what, lstride, qstride in layouts:
        d = torch_.full((L * lstride + GUARD,), P64, dtype=torch_.int64, device=DEV)
        d[:L * lstride].view(L, lstride // kin, kin)[:, :nq, :] = _i64(torch_, lists)
        out = torch_.full((nq * k + GUARD,), P64, dtype=torch_.int64, device=DEV)
        scratch = torch_.full((sb // 8 + GUARD,), P64, dtype=torch_.int64, device=DEV)
        kp.check(kp.merge_large(d.data_ptr(), L, lstride, qstride, nq, kin, k, out.data_ptr(),
                                scratch.data_ptr(), sb))
        torch_.cuda.synchronize()
        o = _np64(out)
        assert np.all(o[nq * k:] == P64), (name, what, "wrote past out")
        assert np.all(_np64(scratch)[sb // 8:] == P64), (name, what, "wrote past the scratch")
        for q in range(nq):
            got = o[q * k:(q + 1) * k]
            bad = np.nonzero(got != want[q])[0]
            assert bad.size == 0, (name, what, "query", q, "first wrong at", int(bad[0]),
                                   "distinct keys returned", int(np.count_nonzero(got)),
                                   "of", int(np.count_nonzero(want[q])))


# ---- launch_remap_keys -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000])
def test_remap_keys(kp, torch_, n):
    """global row = base + local * stride + offset, up to row 2^32 - 1; 0 stays 0."""
    rng = np.random.default_rng(n)
    stride, offset = 3, 2
    local = rng.permutation(n).astype(U64)
    base = 0xFFFFFFFF - (int(local.max()) * stride + offset)
    hi = rng.integers(1, 1 << 32, size=n, dtype=np.uint64) << U64(32)
    keys = hi | (U64(0xFFFFFFFF) - local)
    if n > 1:
        keys[1::3] = 0  # empty entries in between
    want = np.where(keys == 0, U64(0), hi | (U64(0xFFFFFFFF) - (U64(base) + local * U64(stride) + U64(offset))))
    assert int((U64(base) + local * U64(stride) + U64(offset)).max()) == 0xFFFFFFFF
    assert n == 1 or (np.count_nonzero(want == 0) == np.count_nonzero(keys == 0) > 0)
    d = torch_.full((n + GUARD,), P64, dtype=torch_.int64, device=DEV)
    d[:n] = _i64(torch_, keys)
    kp.check(kp.remap_keys(d.data_ptr(), n, stride, offset, base))
    torch_.cuda.synchronize()
    o = _np64(d)
    assert np.all(o[n:] == P64), "wrote past keys[n]"
    assert np.array_equal(o[:n], want)
