"""The int8 prefilter's arithmetic restated in numpy (DESIGN.md §5 "int8
prefilter"; device side csrc/vs_q8.hip), and the adversarial rows and queries
that both tests/test_q8_bounds.py (CPU: the reference alone is sound) and the
stage-level GPU tests (tests/test_q8_stages_gpu.py, test_spec_verify_gpu.py)
draw from.

Rows x are fp32 values (bf16-representable ones for a bf16 collection), any
dim % 128 == 0. One scale S = fp32(max|x|) / fp32(127) per collection (1 for
an all-zero one), fixed when the copy is built: rows written later are
quantised with that stale S and clip. x8 = clamp(rint(fp32(x) / S), -127, 127)
in fp32, half to even. Per row the fp64 norms |x - S x8| and |x|; per 32-row
tile their maxima over live rows, times (1 + 2^-30), rounded up to float (dt,
nt). Per query sq = fp32(max|q|) / 127, q8, a = |sq q8|, c = |q - sq q8|
(rounded up the same way), sigma = (4 dim + 64) 2^-24 |q|_up (1 + 2^-20).
Then for every row and any fp32 evaluation s of q . x:
    L = sqS dot - m - sigma nt  <=  s  <=  U = sqS dot + m + sigma nt,
    m = a dt + c nt.
"""
import numpy as np

F32 = np.float32
UP = 1 + 2.0 ** -30  # q8_norm_up's relative margin ahead of the float round-up
# dev <= t (1 + 2^-30) rounded up to float, one ulp <= 2^-23 relative:
# (1 + 2^-30)(1 + 2^-23) < 1 + 2^-22
NORM_SLACK = 1 + 2.0 ** -22


def _up(v):
    """The smallest float32 >= v (v: an fp64 value)."""
    f = np.float32(v)
    return f if np.float64(f) >= np.float64(v) else np.nextafter(f, np.float32(np.inf))


def _bf16(a):
    """fp32 values rounded to bf16 (nearest even), as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.view(np.float32)


def bf16_bits(a):
    """bf16-representable fp32 values -> their uint16 storage."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not np.any(u & 0xFFFF), "not bf16 values"
    return (u >> 16).astype(np.uint16)


def scale_of(X):
    """S of a collection whose rows are X when the copy is built."""
    amax = np.float32(np.abs(X).max()) if X.size else np.float32(0)
    return np.float32(amax / np.float32(127)) if amax > 0 else np.float32(1)


def row_norms(X, S):
    """x8 (int32) and the fp64 norms |x - S x8|, |x| of every row."""
    X = np.ascontiguousarray(X, np.float32)
    X8 = np.clip(np.rint(X / np.float32(S)), -127, 127).astype(np.int32)
    d = X.astype(np.float64) - np.float64(S) * X8
    return X8, np.sqrt((d * d).sum(1)), np.sqrt((X.astype(np.float64) ** 2).sum(1))


def tile_max(v, n_rows=None):
    """fp64 maxima of v over 32-row tiles (live rows only)."""
    v = v[:n_rows] if n_rows is not None else v
    return np.array([v[i:i + 32].max() for i in range(0, len(v), 32)], np.float64)


def _quantize_rows(X, S):
    X8, dn, xn = row_norms(X, S)
    dt = np.array([_up(t * UP) for t in tile_max(dn)], np.float32)
    nt = np.array([_up(t * UP) for t in tile_max(xn)], np.float32)
    return X8, dt, nt


def query_ref(q, S):
    """Everything the query side derives from one query (fp32 values)."""
    q = np.ascontiguousarray(q, np.float32)
    amax = np.float32(np.abs(q).max())
    sq = np.float32(amax / np.float32(127)) if amax > 0 else np.float32(0)
    if sq > 0:
        q8 = np.clip(np.rint(q / sq), -127, 127).astype(np.int32)
    else:
        q8 = np.zeros(q.shape[0], np.int32)
    s = np.float64(sq) * q8
    e = q.astype(np.float64) - s
    an, cn = np.sqrt((s * s).sum()), np.sqrt((e * e).sum())
    qn = np.sqrt((q.astype(np.float64) ** 2).sum())
    qn_up = _up(qn * UP)
    sigma = np.float32((4.0 * q.shape[0] + 64.0) * 2.0 ** -24 * float(qn_up) * (1 + 2.0 ** -20))
    return dict(q8=q8, sq=sq, sqS=np.float32(sq * np.float32(S)), a=_up(an * UP), c=_up(cn * UP),
                sigma=sigma, an=an, cn=cn, qn=qn)


def _quantize_query(q, S):
    r = query_ref(q, S)
    return r["q8"], r["sqS"], r["a"], r["c"], r["sigma"]


def _fp32_sums(X, q):
    """fp32 scores in three orders: sequential, pairwise (numpy), reversed."""
    xf, qf = X.astype(np.float32), q.astype(np.float32)
    D = xf.shape[1]
    seq = np.zeros(len(X), np.float32)
    rev = np.zeros(len(X), np.float32)
    for i in range(D):
        seq = np.float32(seq + xf[:, i] * qf[i])
        rev = np.float32(rev + xf[:, D - 1 - i] * qf[D - 1 - i])
    return [seq, rev, (xf @ qf).astype(np.float32)]


def bracket(dot, sqS, a, c, sigma, dt_row, nt_row):
    """L, U of every row as the select forms them (float32 arithmetic);
    dt_row / nt_row: the row's tile's bounds."""
    f = np.float32
    m = f(a) * dt_row.astype(f) + f(c) * nt_row.astype(f)
    mid = (dot.astype(f) * f(sqS)).astype(f)
    w = (m + f(sigma) * nt_row.astype(f)).astype(f)
    return (mid - w).astype(f), (mid + w).astype(f)


# ---------------------------------------------------------------------------
# adversarial corpora and queries
# ---------------------------------------------------------------------------
ROW_KINDS = ("unit", "clipped", "spiky", "zero_rows", "pm_absmax", "halfway", "tiny", "norm30")
QUERY_KINDS = ("unit", "norm30", "zero", "onehot", "pm_amax", "neg_row", "copy_row")


def row_kinds(f32):
    """The row kinds of a storage dtype (norm-30 rows: fp32 storage only)."""
    return tuple(k for k in ROW_KINDS if f32 or k != "norm30")


def _unit(rng, n, dim):
    X = rng.standard_normal((n, dim)).astype(np.float32)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def make_rows(kind, n, dim, f32, seed=0):
    """-> (X, X0): the collection's n rows (fp32 values, bf16-representable
    unless f32), and the rows S is computed from (X0 is X unless the kind
    writes rows after the scale was fixed)."""
    rng = np.random.default_rng(1000 + 17 * ROW_KINDS.index(kind) + seed)
    rd = (lambda a: np.ascontiguousarray(a, np.float32)) if f32 else _bf16
    X = rd(_unit(rng, n, dim))
    X0 = X
    if kind == "clipped":  # written after S was fixed: every 7th row x4, one x100
        X = X.copy()
        X[::7] = rd(X[::7] * np.float32(4))
        X[min(n - 1, 11)] = rd(X0[min(n - 1, 11)] * np.float32(100))
    elif kind == "spiky":  # one coordinate 0.9, the rest tiny
        X = X.copy()
        X[:, 6:] *= np.float32(0.01)
        X[:, :5] *= np.float32(0.01)
        X[:, 5] = 0.9
        X = rd(X)
        X0 = X
    elif kind == "zero_rows":  # all-zero rows inside live tiles, and one whole zero tile
        X = X.copy()
        X[1::3] = 0
        X[32:64] = 0
        X[n - 1] = 0
        X0 = X
    elif kind == "pm_absmax":  # every value +-A: every x8 is +-127
        A = np.float32(0.0390625)  # 5 * 2^-7: a bf16 value
        X = np.where(rng.integers(0, 2, (n, dim)) == 1, A, -A).astype(np.float32)
        X[0] = A  # the all-plus row (against a +-amax query: |dot| = 127^2 dim)
        if n > 1:
            X[n - 1] = -A
        X0 = X
    elif kind == "halfway":  # every value an exact half-way point (j + 0.5) S
        # absmax = 127 * 2^-10 makes S = 2^-10 exactly; (2 j + 1) 2^-11 has at
        # most 8 significant bits, so it is a bf16 value as well
        S = np.float32(2.0 ** -10)
        j = rng.integers(-127, 127, (n, dim))  # j + 0.5 in [-126.5, 126.5]
        X = ((j + 0.5) * np.float64(S)).astype(np.float32)
        X[0, 0] = np.float32(127) * S
        assert np.all(_bf16(X) == X) and scale_of(X) == S
        X0 = X
    elif kind == "tiny":  # odd rows: every |value| < S / 2, so x8 = 0 and dt = |x|
        X = X.copy()
        X[0, 0] = np.abs(X).max()  # the scale comes from an even row
        S = scale_of(X)
        t = rng.uniform(-0.49, 0.49, (n, dim)) * np.float64(S)
        X[1::2] = rd(t.astype(np.float32))[1::2]
        assert np.all(np.abs(X[1::2]) < S / 2) and scale_of(X) == S
        X0 = X
    elif kind == "norm30":
        assert f32
        X = (X * np.float32(30)).astype(np.float32)
        X0 = X
    elif kind != "unit":
        raise ValueError(kind)
    return np.ascontiguousarray(X, np.float32), np.ascontiguousarray(X0, np.float32)


def make_queries(X, f32, seed=0, kinds=QUERY_KINDS):
    """One query of every kind for the rows X -> (Q [len(kinds), dim], kinds)."""
    rng = np.random.default_rng(77 + seed)
    n, dim = X.shape
    rd = (lambda a: np.ascontiguousarray(a, np.float32)) if f32 else _bf16
    out = []
    for kind in kinds:
        u = _unit(rng, 1, dim)[0]
        if kind == "unit":
            q = rd(u)
        elif kind == "norm30":
            q = rd(u * np.float32(30))
        elif kind == "zero":
            q = np.zeros(dim, np.float32)
        elif kind == "onehot":
            q = np.zeros(dim, np.float32)
            q[dim // 3] = 1
        elif kind == "pm_amax":
            q = np.where(rng.integers(0, 2, dim) == 1, np.float32(0.25), np.float32(-0.25))
            if n > 0:  # the signs of row 0, so a +-absmax row meets it at full scale
                q = np.where(X[0] >= 0, np.float32(0.25), np.float32(-0.25))
        elif kind == "neg_row":
            q = -X[n // 2]
        elif kind == "copy_row":
            q = X[n - 1 if n < 3 else n // 3].copy()
        else:
            raise ValueError(kind)
        out.append(np.ascontiguousarray(q, np.float32))
    return np.stack(out), tuple(kinds)
