"""Grouped search restated in numpy (include/vsearch.h "Grouped search"), for
the tests of vs_search_groups and of the kernels in csrc/vs_group.hip.

The contract in one sentence: walk the query's full ranking (keys descending);
a row without a group is skipped; the first `limit` distinct groups met are the
answer, in that order, and each keeps the first `group_size` of its rows met.
That is "the groups with the largest best key B(g), descending, each with its
largest keys", because a group is first met at its best key.
"""
import numpy as np

GROUP_NONE = 0xFFFFFFFF
MAX_LIMIT = 128
MAX_SIZE = 16


def score_image(scores):
    """The order-preserving 32-bit image of fp32 scores (the key's high word);
    -0.0 ranks as +0.0."""
    s = np.ascontiguousarray(scores, np.float32).copy()
    s[s == 0.0] = 0.0
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def image_score(images):
    o = np.ascontiguousarray(images, np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return u.view(np.float32)


def make_keys(images, rows):
    """Result keys of (image, global row) pairs."""
    return (np.asarray(images, np.uint64) << np.uint64(32)) | (
        np.uint64(0xFFFFFFFF) - np.asarray(rows, np.uint64))


def key_rows(keys):
    return np.uint64(0xFFFFFFFF) - (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF))


def ranking_of_images(sc, row_base=0):
    """Descending keys of the rows whose image is not 0 (0 = masked)."""
    sc = np.asarray(sc, np.uint32)
    r = np.nonzero(sc)[0]
    keys = make_keys(sc[r], r.astype(np.uint64) + np.uint64(row_base))
    return np.sort(keys)[::-1]


def groups_ref(keys_desc, group_of_row, limit, group_size, row_base=0):
    """keys_desc: one query's full ranking (u64 keys, descending; zeros are
    padding). group_of_row[local row] = group or GROUP_NONE. Returns
    [(group, [keys...])], at most `limit` entries of at most `group_size` keys."""
    assert 1 <= limit <= MAX_LIMIT and 1 <= group_size <= MAX_SIZE
    gor = np.asarray(group_of_row, np.uint32)
    keys = np.asarray(keys_desc, np.uint64)
    keys = keys[keys != 0]
    assert np.all(keys[:-1] > keys[1:]), "the ranking must be strictly descending"
    g = gor[(key_rows(keys) - np.uint64(row_base)).astype(np.int64)]
    on = g != GROUP_NONE
    keys, g = keys[on], g[on]
    # groups in the order first met = descending best key
    _, first = np.unique(g, return_index=True)
    order = g[np.sort(first)][:limit]
    out = []
    for grp in order:
        out.append((int(grp), [int(x) for x in keys[g == grp][:group_size]]))
    return out


def as_arrays(ref, limit, group_size):
    """groups_ref's answer in the layout vs_search_groups writes for one query:
    (groups [limit], hits [limit], keys [limit, group_size], count), zero-padded."""
    groups = np.zeros(limit, np.uint32)
    hits = np.zeros(limit, np.uint32)
    keys = np.zeros((limit, group_size), np.uint64)
    for j, (grp, ks) in enumerate(ref):
        groups[j], hits[j] = grp, len(ks)
        keys[j, :len(ks)] = ks
    return groups, hits, keys, len(ref)
