"""The definition of phx_traj_compact (include/phantom_amd_compact.h) restated in numpy, twice: ``compact`` by the header's positions
formula, column by column, and ``by_mask`` as the boolean index of the transposed plane that ``FragmentBatch.to_sample_batches``
applies on the host.  Plus the cases the tests share.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

DENSITIES = ("all", "none", "alternating", "one", "random 0.1", "random 0.5", "random 0.9")
SPECIAL_WORDS = (0x80000000, 0x7fc00001, 0xff800001, 0x7f800000, 0x00000001)      # -0.0, two NaN payloads, +inf, a denormal


def keep_case(rng, T, N, density):
    """u8 [T, N]; a kept element holds any non-zero byte (the definition tests != 0)"""
    if density == "all":
        k = np.ones((T, N), bool)
    elif density == "none":
        k = np.zeros((T, N), bool)
    elif density == "alternating":                       # an FSM chain's shape: the agents act in every other step
        k = np.broadcast_to((np.arange(T) % 2 == 0)[:, None], (T, N)).copy()
    elif density == "one":
        k = np.zeros((T, N), bool)
        k[rng.integers(T), rng.integers(N)] = True
    else:
        k = rng.random((T, N)) < float(density.split()[1])
    return np.where(k, rng.integers(1, 256, (T, N)), 0).astype(np.uint8)


def plane_case(rng, T, N, elem_bytes):
    """a source plane of any bit patterns: u8 [T, N] for elem_bytes 1, else u32 [T, N] (w = 1) or [T, N, w]"""
    if elem_bytes == 1:
        return rng.integers(0, 256, (T, N), dtype=np.uint64).astype(np.uint8)
    w = elem_bytes // 4
    a = rng.integers(0, 2 ** 32, (T, N, w), dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    flat[:len(SPECIAL_WORDS)] = SPECIAL_WORDS[:flat.size]
    return a[..., 0] if w == 1 else a


def starts(keep):
    """i64 [N + 1]: start[n] = the kept elements of the columns before n; start[N] = K"""
    start = np.zeros(keep.shape[1] + 1, dtype=np.int64)
    np.cumsum((keep != 0).sum(axis=0), out=start[1:])
    return start


def compact(keep, planes, capacity=None):
    """(start, out_row, out_col, {name: dense}) by the header's formula: the position of a kept element (t, n) is
    start[n] + #{u < t : keep[u][n] != 0}; what lies at or beyond ``capacity`` is written nowhere.  The three results are
    min(K, capacity) elements long: what the call writes"""
    T, N = keep.shape
    k = keep != 0
    start = starts(keep)
    capacity = T * N if capacity is None else capacity
    n_out = int(min(start[N], capacity))
    out_row, out_col = np.full(n_out, -1, np.int32), np.full(n_out, -1, np.int32)
    dense = {name: np.zeros((n_out,) + src.shape[2:], src.dtype) for name, src in planes.items()}
    pos = start[None, :N] + (np.cumsum(k, axis=0) - k)           # [T, N]: the position of (t, n) if it is kept
    tt, nn = np.nonzero(k)
    p = pos[tt, nn]
    assert len(set(p.tolist())) == len(p) == start[N] and (p.size == 0 or (p.min() == 0 and p.max() == start[N] - 1))
    fits = p < capacity
    tt, nn, p = tt[fits], nn[fits], p[fits]
    out_row[p], out_col[p] = tt, nn
    for name, src in planes.items():
        dense[name][p] = src[tt, nn]
    return start, out_row, out_col, dense


def by_mask(keep, src):
    """the second restatement: the transposed plane under the transposed mask, as the host masks a FragmentBatch's columns"""
    return np.moveaxis(src, 0, 1)[np.moveaxis(keep, 0, 1) != 0]


def assert_same_batches(got, want, what=""):
    """two to_sample_batches() results: policy for policy, key for key, and every array equal in dtype, shape and bytes"""
    assert set(got) == set(want), (what, set(got), set(want))
    for pid in want:
        assert set(got[pid]) == set(want[pid]), (what, pid, set(got[pid]) ^ set(want[pid]))
        for k, w in want[pid].items():
            g = got[pid][k]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, pid, k, g.dtype, w.dtype, g.shape, w.shape)
            assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, pid, k)
