"""(CPU) The single-query int8 path's restatement (tests/q8_gemv_ref.py) is
sound on its own, on every row kind x query kind the GPU stage tests use
(tests/test_q8_gemv_stages_gpu.py), at dim 768 and 1024:

  * P, the radix floor of the k-th largest workgroup L image, is at most the
    image of the k-th best score, for the fp64 score and for fp32 sums in
    three orders -- the finish may drop every key under P;
  * the scan's formation of the half-width (one rounding of c + sigma, FMA
    contraction allowed) stays within 4 2^-24 w of the reference's, hence
    U and L within 4 2^-24 w + one ulp -- plus half an ulp of xs = dot sqS
    where the device contracts xs +- w into one FMA and so skips the
    reference's rounding of xs (q8_gemv_ref.edge_tol): the tolerance the GPU
    tests use, derived here and not tuned against the kernel.
"""
import numpy as np
import pytest

import q8_gemv_ref as G
import q8_ref as R

N = 130 * 32 + 5  # 130 workgroups of one 4-row step a wave, and a ragged tail
KS = (1, 10, 64, 128)
GRIDS = (130, 40, 5)  # more than k workgroups with rows; fewer than 64 / 128; fewer than 10

CASES = [pytest.param(k, f, d, id=f"{k}-{'f32' if f else 'bf16'}-{d}")
         for d in (768, 1024) for f in (False, True) for k in R.row_kinds(f)]


@pytest.fixture(scope="module")
def corpus():
    cache = {}

    def get(kind, f32, dim):
        key = (kind, f32, dim)
        if key not in cache:
            X, X0 = R.make_rows(kind, N, dim, f32)
            S = R.scale_of(X0)
            X8, dt, nt = R._quantize_rows(X, S)
            Q, kinds = R.make_queries(X, f32)
            cache.clear()  # one corpus at a time
            cache[key] = (X, S, X8, dt, nt, Q, kinds)
        return cache[key]
    return get


@pytest.mark.parametrize("kind,f32,dim", CASES)
def test_P_is_at_most_the_kth_score(corpus, kind, f32, dim):
    X, S, X8, dt, nt, Q, kinds = corpus(kind, f32, dim)
    assert kinds == R.QUERY_KINDS
    for q, qk in zip(Q, kinds):
        L, U, w, xs, r, d = G.brackets(X8, dt, nt, q, S)
        scores = R._fp32_sums(X, q) + [X.astype(np.float64) @ q.astype(np.float64)]
        for nscan in GRIDS:
            lb = G.lbest_ref(L, nscan)
            assert np.count_nonzero(lb) == nscan  # every workgroup has rows
            for k in KS:
                P = G.radix_floor_P(lb, k)
                if nscan < k:
                    assert P == 0, (kind, qk, nscan, k)
                    continue
                assert P != 0 and P & 0xFFFF == 0
                for s in scores:
                    # (fp64 scores: rounded to float toward -inf, so the image is no larger)
                    s32 = s.astype(np.float32)
                    if s.dtype == np.float64:
                        s32 = np.where(s32 > s, np.nextafter(s32, np.float32(-np.inf)), s32)
                    kth = np.sort(G.image(s32))[::-1][k - 1]
                    assert P <= int(kth), (kind, qk, nscan, k, hex(P), hex(int(kth)))


@pytest.mark.parametrize("kind,f32,dim", CASES)
def test_device_formation_of_the_half_width_stays_within_bound(corpus, kind, f32, dim):
    X, S, X8, dt, nt, Q, kinds = corpus(kind, f32, dim)
    tile = np.arange(N) // 32
    for q, qk in zip(Q, kinds):
        L, U, w, xs, r, d = G.brackets(X8, dt, nt, q, S)
        tol = G.width_tol(w)
        floor = G.U_floor(d, r, dt[tile], nt[tile], dim)
        for v, wd in enumerate(G.width_dev(r["a"], r["c"], r["sigma"], dt[tile], nt[tile])):
            err = np.abs(wd.astype(np.float64) - w.astype(np.float64))
            assert np.all(err <= tol), (kind, qk, "variant", v, float((err / np.maximum(tol, 1e-300)).max()))
            for f, (Ud, Ld) in enumerate(G.edges_dev(d, r["sqS"], wd)):
                eu = np.abs(Ud.astype(np.float64) - U.astype(np.float64))
                el = np.abs(Ld.astype(np.float64) - L.astype(np.float64))
                assert np.all(eu <= G.edge_tol(w, U, xs)), (kind, qk, "U variant", v, f)
                assert np.all(el <= G.edge_tol(w, L, xs)), (kind, qk, "L variant", v, f)
                if f == 0:  # xs rounded as the reference rounds it: the bound without its last term
                    assert np.all(eu <= G.width_tol(w) + G.ulp(U)), (kind, qk, "U variant", v)
                    assert np.all(el <= G.width_tol(w) + G.ulp(L)), (kind, qk, "L variant", v)
                # the floor the GPU test holds U to is under every sound form
                assert np.all(floor <= Ud), (kind, qk, "floor", v, f)
        if qk == "zero":
            assert not w.any() and not U.any() and not L.any()


def test_radix_floor_and_counts_on_small_cases():
    img = G.image(np.array([0.5, -0.25, 0.0, 2.0], np.float32))
    assert list(np.argsort(img)) == [1, 2, 0, 3] and img.min() > 0
    assert np.array_equal(G.unimage(img), np.array([0.5, -0.25, 0.0, 2.0], np.float32))
    lb = np.array([0, 0x81234567, 0x81230000, 0, 0x7F000001], np.uint32)
    assert G.radix_floor_P(lb, 1) == 0x81230000
    assert G.radix_floor_P(lb, 3) == 0x7F000000
    assert G.radix_floor_P(lb, 4) == 0
    # two workgroups: 4-row steps 0..7 -> workgroup 0, 8..15 -> 1, 16..23 -> 0 again
    assert list(G.wg_of_row([0, 3, 4, 31, 32, 63, 64, 95, 96], 2)) == [0, 0, 0, 0, 1, 1, 0, 0, 1]
    # list 0 full with its last entry at P: falls back; list 1 has one entry over P
    key = lambda im, row: (np.uint64(im) << np.uint64(32)) | np.uint64(0xFFFFFFFF - row)
    ul = np.array([[key(9, 0), key(8, 1)], [key(9, 32), key(3, 33)], [key(9, 64), 0]], np.uint64)
    allow = np.ones(96, bool)
    allow[5] = False
    assert G.finish_counts(ul, 8, allow, 96, 3) == (31 + 1 + 1, 1)
    assert G.finish_counts(ul, 0, None, 96, 3) == (32 + 32 + 1, 2)
