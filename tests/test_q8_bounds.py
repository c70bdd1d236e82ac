"""(CPU) The int8 prefilter's bracket, restated in numpy (DESIGN.md §5 "int8
prefilter"; the device side is vs_q8.hip + select_q8_kernel, checked on the
GPU by tools/q8_check.hip and tests/test_q8_gpu.py).

For rows x (bf16 values, or fp32), one collection scale S = max|x| / 127 and
x8 = clamp(rint(x / S), -127, 127); per 32-row tile dt = max |x - S x8| and
nt = max |x| rounded up; per query q, sq = max|q| / 127, q8, a = |sq q8|,
c = |q - sq q8| (rounded up) and sigma = (4 D + 64) 2^-24 |q|. Then for every
row, with m = a dt + c nt and the int32 dot q8 . x8:
    L = sqS dot - m - sigma nt  <=  s  <=  U = sqS dot + m + sigma nt
for any fp32 evaluation s of q . x. This file checks that on random,
clipped and adversarial rows against fp32 sums in several orders.
"""
import numpy as np
import pytest

D = 768


# the restatement itself lives in tests/q8_ref.py, shared with the GPU stage tests
from q8_ref import (QUERY_KINDS, _bf16, _fp32_sums, _quantize_query, _quantize_rows, _up,  # noqa: F401
                    bracket, make_queries, make_rows, row_kinds, scale_of)


@pytest.mark.parametrize("case", ["unit_bf16", "fp32", "clipped", "spiky"])
def test_int8_bracket_holds(case):
    rng = np.random.default_rng(["unit_bf16", "fp32", "clipped", "spiky"].index(case) + 11)
    n = 1024
    X = rng.standard_normal((n, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    if case == "unit_bf16":
        X = _bf16(X)
    S = np.float32(np.float32(np.abs(X).max()) / np.float32(127))
    if case == "clipped":  # rows written after S was chosen, 4x larger: clipped
        X[::7] *= 4
    if case == "spiky":  # one large coordinate per row, the rest tiny
        X[:, 5] = 0.9
        X[:, 6:] *= 0.01
        S = np.float32(np.float32(np.abs(X).max()) / np.float32(127))
    X8, dt, nt = _quantize_rows(X, S)
    for j in range(6):
        q = rng.standard_normal(D).astype(np.float32)
        q = _bf16(q / np.linalg.norm(q)) if case == "unit_bf16" else q / np.linalg.norm(q)
        if j == 5:
            q = q * np.float32(30.0)  # large norm
        q8, sqS, a, c, sigma = _quantize_query(q, S)
        dot = X8 @ q8  # exact in int64
        assert np.abs(dot).max() < 2 ** 24  # exact in fp32 too
        tile = np.arange(n) // 32
        m = a * dt[tile] + c * nt[tile]
        L = np.float32(dot.astype(np.float32) * sqS) - m - sigma * nt[tile]
        U = np.float32(dot.astype(np.float32) * sqS) + m + sigma * nt[tile]
        exact = X.astype(np.float64) @ q.astype(np.float64)
        assert np.all(L <= exact) and np.all(exact <= U), case
        for s in _fp32_sums(X, q):
            assert np.all(L <= s) and np.all(s <= U), case


def test_int8_window_is_narrow():
    """The bracket is worth having: for unit 768-d rows its width 2m is a
    fraction of the score spread (the int8 pass admits ~5x the rows the
    bf16 pass does, not all of them)."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((4096, D)).astype(np.float32)
    X = _bf16(X / np.linalg.norm(X, axis=1, keepdims=True))
    S = np.float32(np.float32(np.abs(X).max()) / np.float32(127))
    X8, dt, nt = _quantize_rows(X, S)
    q = _bf16(rng.standard_normal(D).astype(np.float32))
    q = _bf16(q / np.linalg.norm(q))
    q8, sqS, a, c, sigma = _quantize_query(q, S)
    m = float(a * dt.max() + c * nt.max())
    spread = float(np.std(X.astype(np.float64) @ q.astype(np.float64)))
    assert 0.2 < 2 * m / spread < 1.5, (m, spread)


def _cases():
    for f32 in (False, True):
        for kind in row_kinds(f32):
            for dim in (768, 1024) if not f32 else (768,):
                yield pytest.param(kind, f32, dim, id=f"{kind}-{'f32' if f32 else 'bf16'}-{dim}")
    yield pytest.param("unit", False, 128, id="unit-bf16-128")
    # (the bracket's domain ends at dim 127^2 < 2^24, dim <= 1040: DESIGN.md §5 "Domain")
    yield pytest.param("clipped", True, 1024, id="clipped-f32-1024")
    yield pytest.param("pm_absmax", True, 1024, id="pm_absmax-f32-1024")


@pytest.mark.parametrize("kind,f32,dim", list(_cases()))
def test_reference_bracket_on_every_generator(kind, f32, dim):
    """Every row kind x every query kind the GPU stage tests use: the
    reference bracket L <= s <= U holds against the fp64 score and against
    fp32 sums in three orders, with a stale S where the kind has one and a
    ragged last tile (n = 101)."""
    n = 101
    X, X0 = make_rows(kind, n, dim, f32)
    assert X.shape == (n, dim) and (f32 or np.all(_bf16(X) == X))
    S = scale_of(X0)
    X8, dt, nt = _quantize_rows(X, S)
    assert X8.min() >= -127 and X8.max() <= 127
    if kind == "pm_absmax":
        assert np.all(np.abs(X8) == 127)
    if kind == "halfway":  # rint went to even on every value but the planted absmax
        assert np.all(X8.ravel()[1:] % 2 == 0)
    if kind == "tiny":
        assert np.all(X8[1::2] == 0)
    Q, kinds = make_queries(X, f32)
    assert kinds == QUERY_KINDS
    tile = np.arange(n) // 32
    for q, qk in zip(Q, kinds):
        assert f32 or np.all(_bf16(q) == q)
        q8, sqS, a, c, sigma = _quantize_query(q, S)
        dot = X8 @ q8
        assert np.abs(dot).max() < 2 ** 24, (kind, qk)  # exact in fp32 too
        L, U = bracket(dot, sqS, a, c, sigma, dt[tile], nt[tile])
        exact = X.astype(np.float64) @ q.astype(np.float64)
        assert np.all(L <= exact) and np.all(exact <= U), (kind, qk)
        for s in _fp32_sums(X, q):
            assert np.all(L <= s) and np.all(s <= U), (kind, qk)
        if qk == "zero":
            assert sqS == 0 and a == 0 and c == 0 and sigma == 0 and not q8.any()
    if kind == "pm_absmax" and dim == 1024:  # the largest dot the int8 pass can meet
        q8 = _quantize_query(Q[kinds.index("pm_amax")], S)[0]
        assert abs(int(X8[0] @ q8)) == 127 * 127 * dim
