"""(CPU) tests/gemv_ref.py on its own: its key order against the oracle's
(score descending, ties by row ascending) on floats that include +-0,
negatives and +-inf, its list and ownership helpers on hand cases, and each
data builder's stated bound, so an edit to a builder cannot quietly lose what
tests/test_gemv_stages_gpu.py relies on it for."""
import numpy as np
import pytest

import gemv_ref as GR
import q8_gemv_ref as G
import q8_ref
import rsel_ref as R

U64 = np.uint64


def _floats(rng, n):
    s = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38],
                       np.float32)
    s[rng.choice(n, 60, replace=False)] = np.tile(special, 6)  # each special value six times: ties
    return s


@pytest.mark.parametrize("row_base", [0, 12345, 0xFFFFFFFE - 500])
def test_key_order_is_the_oracles(orc, row_base):
    """The oracle searching a one-column collection under q = [1] ranks the
    floats themselves: its order has to be the descending key order."""
    rng = np.random.default_rng(row_base % 1000)
    n = 500
    s = _floats(rng, n)
    _, s64, rows, cnt = orc.search(s.reshape(n, 1), np.ones((1, 1), np.float32), n, row_base)
    assert int(cnt[0]) == n
    keys = GR.topk_keys(s, np.arange(n), row_base, n)
    assert np.array_equal(GR.key_row(keys), rows[0].astype(np.int64))
    got = GR.key_score(keys)
    assert np.array_equal(got.astype(np.float64), s64[0] + 0.0)  # -0.0 comes back as +0.0
    assert not np.any(np.signbit(got[got == 0]))
    assert np.all(keys[:-1] > keys[1:]) and np.all(keys != 0)


def test_make_key_hand_cases():
    k = GR.make_key(np.array([1.0, -1.0, -0.0, 0.0], np.float32), [0, 5, 7, 7])
    assert [hex(int(x)) for x in k] == ["0xbf800000ffffffff", "0x407ffffffffffffa",
                                        "0x80000000fffffff8", "0x80000000fffffff8"]
    # one image function, three names
    s = _floats(np.random.default_rng(1), 200)
    assert np.array_equal(R.score_ord(s), G.image(s))
    assert np.array_equal((GR.make_key(s, np.arange(200)) >> U64(32)).astype(np.uint32), G.image(s))
    assert int(GR.make_key(np.float32(-np.inf), 0xFFFFFFFF)) == 0x007FFFFF << 32  # the smallest key of a number
    out = GR.topk_keys(np.array([2.0, 2.0, 3.0], np.float32), [4, 1, 9], 10, 5)
    assert list(GR.key_row(out[:3])) == [19, 11, 14] and list(out[3:]) == [0, 0]
    assert list(GR.topk_keys(np.zeros(0, np.float32), [], 0, 2)) == [0, 0]


def test_topk_lists_against_a_loop():
    rng = np.random.default_rng(5)
    keys = rng.integers(1, 1 << 63, 300, dtype=np.uint64)
    unit = rng.integers(0, 7, 300)
    unit[unit == 3] = 2  # list 3 stays empty
    for k in (1, 5, 64, 100):
        got = GR.topk_lists(keys, unit, 7, k)
        for u in range(7):
            want = np.sort(keys[unit == u])[::-1][:k]
            assert np.array_equal(got[u, :want.size], want) and not got[u, want.size:].any()
    assert not GR.topk_lists(keys[:0], unit[:0], 3, 4).any()


def test_owner():
    # RB as GemvShape computes it: 64 / gcd(chunks per row, 64)
    assert [GR.rows_per_step(d, 0) for d in GR.TABLE_DIMS] == [2, 1, 2, 1, 1, 1, 1, 1, 1, 1]
    assert [GR.rows_per_step(d, 1) for d in GR.TABLE_DIMS] == [4, 2, 4, 1, 2, 1, 1, 1, 1, 1]
    for d in GR.TABLE_DIMS:
        for bf in (0, 1):
            cpr, rb = d // (8 if bf else 4), GR.rows_per_step(d, bf)
            assert (rb * cpr) % 64 == 0 and all((r * cpr) % 64 for r in range(1, rb))
    # 2 workgroups = 16 waves, 4 rows a step: rows 0..3 wave 0, 4..7 wave 1, ..., 64..67 wave 0
    rows = np.arange(200)
    w = GR.owner_wave(rows, 4, 16)
    assert list(w[:9]) == [0, 0, 0, 0, 1, 1, 1, 1, 2] and w[63] == 15 and w[64] == 0
    assert np.array_equal(GR.owner(rows, 4, 16), w // 8)
    assert GR.owner(35, 4, 16) == 1 and GR.owner(99, 4, 16) == 1 and GR.owner(100, 4, 16) == 1
    # contiguous slices: every row has a wave, the waves fit the workgroups
    for n in (1, 2, 63, 64, 65, 257, 4103, 1_000_000):
        for cus in (8, 256, 304):
            nwg, rpw = GR.slice_grid(n, cus)
            last = int(GR.owner_slice_wave(n - 1, rpw))
            assert nwg * GR.WAVES - GR.WAVES <= last < nwg * GR.WAVES and nwg <= 3 * cus
            assert rpw >= min(GR.MIN_ROWS_PER_WAVE, n) or n < GR.WAVES * GR.MIN_ROWS_PER_WAVE


@pytest.mark.parametrize("n", [1, 63, 64, 65, 16384, 16385, 40000])
def test_compact_and_its_bitmaps(n):
    rng = np.random.default_rng(n)
    maps = GR.compact_bitmaps(n, rng)
    assert ("bits past n set" in maps) == (n % 64 != 0)
    for name, w in maps.items():
        assert w.dtype == np.uint64 and w.size == (n + 63) // 64, name
        rows = GR.compact(w, n)
        bits = [(int(w[r >> 6]) >> (r & 63)) & 1 for r in range(n)] if n <= 16385 else None
        if bits is not None:
            assert list(rows) == [r for r in range(n) if bits[r]], name
        assert rows.size == 0 or (int(rows[-1]) < n and np.all(np.diff(rows.astype(np.int64)) > 0)), name
    assert GR.compact(maps["all ones"], n).size == n and GR.compact(maps["all zeros"], n).size == 0
    assert list(GR.compact(maps["bit n - 1 alone"], n)) == [n - 1]
    assert set(GR.compact(maps["bits 0, 63, 64, n - 1"], n)) == {b for b in (0, 63, 64, n - 1) if b < n}
    if n > 16384:
        r = GR.compact(maps["alternate blocks"], n)
        assert r[0] == 16384 and not np.any((r // 16384) % 2 == 0)
    if n % 64:
        w = maps["bits past n set"]
        assert bin(int(w[-1])).count("1") > bin(int(w[-1]) & ((1 << (n % 64)) - 1)).count("1")


@pytest.mark.parametrize("dim", [8, 100, 772, 128, 4096])
def test_exact_data(dim):
    n = 300
    for negative in (False, True):
        q = GR.exact_query(dim, negative)
        X = GR.exact_rows(n, q)
        s = GR.exact_scores(X, q)  # asserts |dot| <= 9 dim < 2^24 and float32(dot) == dot
        assert np.abs(X).max() <= 3 and np.abs(q).max() <= 3 and q.any()
        assert not X[0].any() and np.array_equal(X[1], q) and np.array_equal(X[2], -q)
        assert s[0] == 0 and s[1] == float(q @ q) == -s[2]
        # exact in bf16: the collection stores these very numbers
        assert np.array_equal(q8_ref._bf16(X), X) and np.array_equal(q8_ref._bf16(q), q)
        # whole-score ties, so the row word decides most ranks
        assert np.unique(s).size <= n // 2 + 4
        if negative:
            assert np.all(q < 0)
            assert np.all(np.signbit(X[0] * q))  # every product of the zero row is -0.0
    assert 9 * 4096 < 1 << 24


@pytest.mark.parametrize("dim", [8, 100, 128, 4096])
def test_onehot_data(dim):
    n = 4103
    X, q, s = GR.onehot_rows(n, dim), GR.onehot_query(dim), GR.onehot_scores(n, dim)
    assert np.array_equal(X.sum(axis=1), np.ones(n)) and np.array_equal(X @ q, s)
    assert all(GR.onehot_column(s[r]) == r % dim for r in (0, 1, dim - 1, dim, n - 1))
    assert np.array_equal(q8_ref._bf16(X), X)


@pytest.mark.parametrize("bf16", [0, 1])
def test_real_data(orc, bf16):
    X, q = GR.real_rows(orc, 50, 256, bf16), GR.real_query(orc, 256)
    assert X.shape == (50, 256) and q.shape == (256,)
    assert np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1.0, atol=1e-2)
    if bf16:
        assert np.array_equal(q8_ref._bf16(X), X)
    assert np.all(GR.bar(np.array([0.0, 2.0])) == [1e-6, 2e-5 + 1e-6])
