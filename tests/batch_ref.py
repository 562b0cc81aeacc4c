"""The definition of phx_train_batch (include/phantom_amd_batch.h) restated in numpy, twice: ``train_batch`` vectorised, and
``train_batch_loop`` as a plain per-element Python loop for the positions, the walk, the record image and the moments in the fixed
order.  Sources are u8 ``[T, N]`` (a byte plane) or u32 ``[T, N]`` / ``[T, N, w]`` (bit patterns); a plane is ``(src, word_off)``.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
GOLDEN = 0x9E3779B97F4A7C15
MOMENTS_DTYPE = np.dtype([("count", "<i8"), ("sum", "<f8"), ("sumsq", "<f8"), ("mean", "<f4"), ("den", "<f4")])


def round_keys(seed, epoch):
    """six u32 round keys from splitmix64, all arithmetic mod 2^64"""
    s = (seed ^ ((epoch * GOLDEN) & M64)) & M64
    keys = []
    for _ in range(6):
        s = (s + GOLDEN) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        keys.append(z & M32)
    return keys


def half_bits(K):
    """h = w / 2 for the smallest even w >= 2 with 2^w >= K"""
    w = 2
    while (1 << w) < K:
        w += 2
    return w // 2


def _f(R, key, mask):
    x = (R ^ np.uint64(key)) & np.uint64(M32)
    for mul, sh in ((0x9E3779B1, 15), (0x85EBCA77, 13), (0xC2B2AE3D, 16)):
        x = (x * np.uint64(mul)) & np.uint64(M32)
        x ^= x >> np.uint64(sh)
    return x & mask


def perm(K, seed, epoch, shuffle=1, walks=None):
    """i64 [K]: q for every p; ``walks`` (a list) receives the longest walk"""
    p = np.arange(K, dtype=np.uint64)
    if not shuffle or K <= 1:
        return p.astype(np.int64)
    h = np.uint64(half_bits(K))
    mask = np.uint64((1 << int(h)) - 1)
    keys = round_keys(seed, epoch)
    x, todo, trips = p.copy(), np.ones(K, bool), 0
    while todo.any():
        v = x[todo]
        L, R = v >> h, v & mask
        for key in keys:
            L, R = R, L ^ _f(R, key, mask)
        v = (L << h) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(K)
        trips += 1
    if walks is not None:
        walks.append(trips)
    return x.astype(np.int64)


def perm_one(p, K, keys):
    """the walk of one position in Python integers"""
    if K <= 1:
        return p
    h = half_bits(K)
    mask = (1 << h) - 1
    x = p
    while True:
        L, R = x >> h, x & mask
        for key in keys:
            y = (R ^ key) & M32
            y = (y * 0x9E3779B1) & M32; y ^= y >> 15
            y = (y * 0x85EBCA77) & M32; y ^= y >> 13
            y = (y * 0xC2B2AE3D) & M32; y ^= y >> 16
            L, R = R, L ^ (y & mask)
        x = (L << h) | R
        if x < K:
            return x


def kept_mask(T, N, keep=None, col_class=None, class_id=0):
    k = np.ones((T, N), bool) if keep is None else np.asarray(keep).reshape(T, N) != 0
    if col_class is not None:
        cc = np.asarray(col_class)
        k = k & (cc[np.arange(N) % len(cc)] == class_id)[None, :]
    return k


def fixed_order_sum(x):
    """f64: 256 lane values folding j, j + 256, .. from +0.0, then the tree h = 128 .. 1 (a +0.0 pad changes no lane: none is -0.0)"""
    x = np.asarray(x, np.float64)
    pad = np.zeros((-len(x)) % 256 + len(x), np.float64)
    pad[:len(x)] = x
    a = np.zeros(256, np.float64)
    for row in pad.reshape(-1, 256):
        a = a + row
    h = 128
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def moments_of(x, k):
    """the moments record of f32 ``x`` [T, N] under the kept mask ``k``"""
    T, N = k.shape
    s, q = np.zeros(N, np.float64), np.zeros(N, np.float64)
    for t in range(T):
        d = x[t].astype(np.float64)
        with np.errstate(all="ignore"):                       # (what is not kept may hold anything)
            s = np.where(k[t], s + d, s)
            q = np.where(k[t], q + d * d, q)
    return finish_moments(int(k.sum()), fixed_order_sum(s), fixed_order_sum(q))


def finish_moments(K, total, totsq):
    m = np.zeros((), MOMENTS_DTYPE)
    m["count"], m["sum"], m["sumsq"], m["mean"], m["den"] = K, total, totsq, np.float32(0.0), np.float32(1e-4)
    if K > 0:
        mu = np.float64(total) / np.float64(K)
        v = np.float64(totsq) / np.float64(K) - mu * mu
        v = v if v > 0 else np.float64(0.0)
        m["mean"] = np.float32(mu)
        m["den"] = max(np.float32(1e-4), np.float32(np.sqrt(v)))
    return m


def _words(src):
    """u32 [T, N, w] of a source: a byte zero-extended, a word plane as it is"""
    a = np.asarray(src)
    if a.dtype == np.uint8:
        return a.astype(np.uint32)[..., None]
    a = a.view(np.uint32)
    return a[..., None] if a.ndim == 2 else a


def default_layout(elem_bytes):
    """(word_offs, row_words): the planes packed in order, the record rounded up to whole 64-byte units"""
    offs, o = [], 0
    for eb in elem_bytes:
        offs.append(o)
        o += 1 if eb == 1 else eb // 4
    return offs, max(16, -(-o // 16) * 16)


def train_batch(T, N, planes, row_words, keep=None, col_class=None, class_id=0, shuffle=1, seed=0, epoch=0, std_plane=-1, capacity=None):
    """dict(start, K, records u32 [K, row_words], out_row, out_col i32 [K], moments or None); records / out_row / out_col are None
    where K > capacity: the call writes none of them"""
    k = kept_mask(T, N, keep, col_class, class_id)
    start = np.zeros(N + 1, np.int64)
    np.cumsum(k.sum(axis=0), out=start[1:])
    K = int(start[N])
    res = dict(start=start, K=K, records=None, out_row=None, out_col=None, moments=None)
    if std_plane >= 0:
        x = _words(planes[std_plane][0])[..., 0].view(np.float32)
        res["moments"] = moments_of(x, k)
    if capacity is not None and K > capacity:
        return res
    pos = start[None, :N] + (np.cumsum(k, axis=0) - k)
    tt, nn = np.nonzero(k)
    q = perm(K, seed, epoch, shuffle)[pos[tt, nn]]
    rec = np.zeros((K, row_words), np.uint32)
    for i, (src, off) in enumerate(planes):
        w = _words(src)[tt, nn]
        if i == std_plane:
            with np.errstate(all="ignore"):
                w = ((w.view(np.float32) - res["moments"]["mean"]) / res["moments"]["den"]).astype(np.float32).view(np.uint32)
        rec[q, off:off + w.shape[1]] = w
    row, col = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    row[q], col[q] = tt, nn
    res.update(records=rec, out_row=row, out_col=col)
    return res


def train_batch_loop(T, N, planes, row_words, keep=None, col_class=None, class_id=0, shuffle=1, seed=0, epoch=0, std_plane=-1, capacity=None):
    """the same by plain loops over the elements, Python floats for the f64 steps and np.float32 for the f32 ones"""
    kp = None if keep is None else np.asarray(keep).reshape(T, N)
    is_kept = lambda t, n: (kp is None or kp[t, n] != 0) and (col_class is None or col_class[n % len(col_class)] == class_id)
    count = [sum(1 for t in range(T) if is_kept(t, n)) for n in range(N)]
    start = np.zeros(N + 1, np.int64)
    for n in range(N):
        start[n + 1] = start[n] + count[n]
    K = int(start[N])
    res = dict(start=start, K=K, records=None, out_row=None, out_col=None, moments=None)
    words = [_words(src) for src, _ in planes]
    mean = den = None
    if std_plane >= 0:
        x = words[std_plane][..., 0].view(np.float32)
        s, sq = [0.0] * N, [0.0] * N
        for n in range(N):
            for t in range(T):
                if is_kept(t, n):
                    d = float(x[t, n])
                    s[n] += d
                    sq[n] += d * d
        tot = []
        for col in (s, sq):
            a = [0.0] * 256
            for j, v in enumerate(col):
                a[j % 256] = a[j % 256] + v
            h = 128
            while h >= 1:
                for i in range(h):
                    a[i] = a[i] + a[i + h]
                h //= 2
            tot.append(a[0])
        m = np.zeros((), MOMENTS_DTYPE)
        m["count"], m["sum"], m["sumsq"] = K, tot[0], tot[1]
        mean, den = np.float32(0.0), np.float32(1e-4)
        if K > 0:
            mu = tot[0] / float(K)
            v = tot[1] / float(K) - mu * mu
            v = v if v > 0 else 0.0
            mean = np.float32(mu)
            sd = np.float32(math.sqrt(v))
            den = sd if sd > np.float32(1e-4) else np.float32(1e-4)
        m["mean"], m["den"] = mean, den
        res["moments"] = m
    if capacity is not None and K > capacity:
        return res
    keys = round_keys(seed, epoch)
    rec = np.zeros((K, row_words), np.uint32)
    row, col = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    for n in range(N):
        p = int(start[n])
        for t in range(T):
            if not is_kept(t, n):
                continue
            q = perm_one(p, K, keys) if shuffle and K > 1 else p
            p += 1
            assert row[q] == -1
            row[q], col[q] = t, n
            for i, (_, off) in enumerate(planes):
                for j in range(words[i].shape[2]):
                    u = words[i][t, n, j]
                    if i == std_plane:
                        u = np.float32((np.float32(u.view(np.float32) - mean)) / den).view(np.uint32)
                    rec[q, off + j] = u
    res.update(records=rec, out_row=row, out_col=col)
    return res


def same(a, b):
    """two results are equal byte for byte"""
    assert a["K"] == b["K"] and a["start"].tobytes() == b["start"].tobytes()
    for k in ("records", "out_row", "out_col", "moments"):
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or (a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()), k
