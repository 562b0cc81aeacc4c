"""phx_filter_update / phx_filter_apply and ObsFilter.fold restated in numpy, bit for bit (include/phantom_amd_filter.h), twice: a plain
loop form that follows the header a line at a time (``*_loop``) and a vectorised form (the names without the suffix) that the GPU tests
use; tests/test_filter_cpu.py holds the two against each other.  Every f64 operation is numpy's correctly rounded one on scalars or
arrays of float64; nothing here contracts a product and a sum."""
import numpy as np

MAX_DIM, MAX_CLASSES, LANES = 16, 16, 256
STATE_DTYPE = np.dtype([("count", "<i8"), ("updates", "<i8"), ("mean", "<f8", (MAX_DIM,)), ("m2", "<f8", (MAX_DIM,))])
UPDATE_KERNELS = "phx_filter_sum_kernel+phx_filter_mean_kernel+phx_filter_center_kernel+phx_filter_m2_kernel+phx_filter_merge_kernel"
APPLY_KERNEL = "phx_filter_apply_kernel"


def workspace_bytes(N, D):
    return 8 * ((D + 1) * N + 528)


def empty_state(n_classes):
    return np.zeros(n_classes, STATE_DTYPE)


def _planes(obs, keep, col_class):
    x = np.asarray(obs, np.float32)
    T, D = x.shape[0], x.shape[-1]
    x = x.reshape(T, -1, D)
    N = x.shape[1]
    k = np.ones((T, N), bool) if keep is None else np.asarray(keep).reshape(T, N) != 0
    c = np.zeros(N, np.int64) if col_class is None else np.asarray(col_class, np.int64).reshape(N)
    return x, k, c, T, N, D


# ---- the fixed-order fold ----------------------------------------------------------------------------------------------------------
def fold_loop(v):
    """the header's FOLD of f64 values v[n] (columns of other classes already +0.0)"""
    a = [np.float64(0.0)] * LANES
    for i in range(LANES):
        for n in range(i, len(v), LANES):
            a[i] = a[i] + np.float64(v[n])
    h = LANES // 2
    while h >= 1:
        for i in range(h):
            a[i] = a[i] + a[i + h]
        h //= 2
    return a[0]


def fold(v):
    """FOLD along the first axis of f64 ``v`` [N, ..]"""
    v = np.asarray(v, np.float64)
    rows = -(-v.shape[0] // LANES)
    pad = np.zeros((rows * LANES,) + v.shape[1:], np.float64)
    pad[:v.shape[0]] = v
    pad = pad.reshape((rows, LANES) + v.shape[1:])
    a = np.zeros((LANES,) + v.shape[1:], np.float64)
    for r in range(rows):                                # (a missing n adds +0.0: the lane's value is unchanged, also when it is +0.0)
        a = a + pad[r]
    h = LANES // 2
    while h >= 1:
        a = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


# ---- update ------------------------------------------------------------------------------------------------------------------------
def _merge(st, c, D, K, mb, m2b):
    na = int(st["count"][c])
    n = na + K
    for d in range(D):
        mean, m2 = np.float64(st["mean"][c, d]), np.float64(st["m2"][c, d])
        delta = np.float64(mb[d]) - mean
        st["mean"][c, d] = mean + delta * (np.float64(K) / np.float64(n))
        st["m2"][c, d] = (m2 + np.float64(m2b[d])) + (delta * delta) * ((np.float64(na) * np.float64(K)) / np.float64(n))
    st["count"][c] = n
    st["updates"][c] += 1


def update_loop(state, obs, keep=None, col_class=None):
    """the state after phx_filter_update, the header a line at a time; ``state`` [n_classes] of STATE_DTYPE is not modified"""
    x, k, cls, T, N, D = _planes(obs, keep, col_class)
    st = state.copy()
    for c in range(len(st)):
        K = int(sum(int(k[t, n]) for n in range(N) if cls[n] == c for t in range(T)))
        if K == 0:
            continue
        mb, m2b = [], []
        for d in range(D):
            s = [np.float64(0.0)] * N
            for n in range(N):
                if cls[n] == c:
                    for t in range(T):
                        if k[t, n]:
                            s[n] = s[n] + np.float64(x[t, n, d])
            mb.append(fold_loop(s) / np.float64(K))
            q = [np.float64(0.0)] * N
            for n in range(N):
                if cls[n] == c:
                    for t in range(T):
                        if k[t, n]:
                            e = np.float64(x[t, n, d]) - mb[d]
                            q[n] = q[n] + e * e
            m2b.append(fold_loop(q))
        _merge(st, c, D, K, mb, m2b)
    return st


def update(state, obs, keep=None, col_class=None):
    """the vectorised form of ``update_loop``"""
    x, k, cls, T, N, D = _planes(obs, keep, col_class)
    st = state.copy()
    xd = x.astype(np.float64)
    s = np.zeros((N, D), np.float64)
    for t in range(T):
        s = np.where(k[t][:, None], s + xd[t], s)
    cnt = k.sum(axis=0)
    for c in range(len(st)):
        of = cls == c
        K = int(cnt[of].sum())
        if K == 0:
            continue
        mb = fold(np.where(of[:, None], s, 0.0)) / np.float64(K)
        q = np.zeros((N, D), np.float64)
        for t in range(T):
            e = xd[t] - mb[None, :]
            q = np.where(k[t][:, None], q + e * e, q)
        m2b = fold(np.where(of[:, None], q, 0.0))
        _merge(st, c, D, K, mb, m2b)
    return st


# ---- apply -------------------------------------------------------------------------------------------------------------------------
def table(state, D):
    """``(mean_f f32 [n_classes, D], den_f f32 [n_classes, D], seen bool [n_classes])`` as apply forms them"""
    n = len(state)
    mean_f, den_f = np.zeros((n, D), np.float32), np.ones((n, D), np.float32)
    for c in range(n):
        count = int(state["count"][c])
        if count == 0:
            continue
        mean = state["mean"][c, :D].astype(np.float64)
        var = mean * mean if count == 1 else state["m2"][c, :D].astype(np.float64) / np.float64(count - 1)
        mean_f[c] = mean.astype(np.float32)
        den_f[c] = np.sqrt(var).astype(np.float32) + np.float32(1e-8)
    return mean_f, den_f, state["count"] > 0


def apply_loop(state, obs, keep=None, col_class=None, clip=0.0):
    x, k, cls, T, N, D = _planes(obs, keep, col_class)
    mean_f, den_f, seen = table(state, D)
    clip = np.float32(clip)
    out = np.zeros((T, N, D), np.float32)
    for t in range(T):
        for n in range(N):
            c = int(cls[n])
            if not k[t, n] or not 0 <= c < len(state):
                continue
            for d in range(D):
                y = np.float32(np.float32(x[t, n, d] - mean_f[c, d]) / den_f[c, d])
                if clip > 0 and seen[c]:
                    y = min(max(y, -clip), clip)
                out[t, n, d] = y
    return out.reshape(np.asarray(obs).shape)


def apply(state, obs, keep=None, col_class=None, clip=0.0):
    """the vectorised form of ``apply_loop``"""
    x, k, cls, T, N, D = _planes(obs, keep, col_class)
    mean_f, den_f, seen = table(state, D)
    ok = (cls >= 0) & (cls < len(state))
    c = np.where(ok, cls, 0)
    with np.errstate(over="ignore"):
        y = ((x - mean_f[c][None]).astype(np.float32) / den_f[c][None]).astype(np.float32)
    if clip > 0:
        y = np.where(seen[c][None, :, None], np.minimum(np.maximum(y, -np.float32(clip)), np.float32(clip)), y)
    out = np.where((k & ok[None, :])[..., None], y, np.float32(0.0)).astype(np.float32)
    return out.reshape(np.asarray(obs).shape)


# ---- the fold into a first layer ---------------------------------------------------------------------------------------------------------
def fold_layer_loop(W, b, mean_f, den_f):
    """``(W', b')`` f32: W [H, D] and b [H] with the filter of one class folded in"""
    W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
    W2, b2 = np.empty_like(W), np.empty_like(b)
    for j in range(W.shape[0]):
        s = np.float64(0.0)
        for i in range(W.shape[1]):
            W2[j, i] = np.float32(np.float64(W[j, i]) / np.float64(den_f[i]))
            s = s + (np.float64(W[j, i]) * np.float64(mean_f[i])) / np.float64(den_f[i])
        b2[j] = np.float32(np.float64(b[j]) - s)
    return W2, b2


def fold_layer(W, b, mean_f, den_f):
    W, b = np.asarray(W, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    m, den = np.asarray(mean_f, np.float32).astype(np.float64), np.asarray(den_f, np.float32).astype(np.float64)
    terms = (W * m[None, :]) / den[None, :]
    s = np.zeros(W.shape[0], np.float64)
    for i in range(W.shape[1]):
        s = s + terms[:, i]
    return (W / den[None, :]).astype(np.float32), (b - s).astype(np.float32)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def known_obs(u, T=3, N=5, D=2):
    """the header's small case: x[t][n][d] = (float)(((u * 7 + 3 t + 5 n + 11 d) % 13) - 4) / 2"""
    t, n, d = np.meshgrid(np.arange(T), np.arange(N), np.arange(D), indexing="ij")
    return (((u * 7 + 3 * t + 5 * n + 11 * d) % 13 - 4).astype(np.float32) / np.float32(2)).astype(np.float32)


KNOWN_CLASS = np.array([0, 1, 0, 1, 0], np.int32)


def random_case(rng, T, N, D, n_classes, keep="random", offset=0.0):
    """``(obs f32 [T, N, D], keep u8 [T, N] or None, col_class i32 [N])``: class ``n_classes - 1`` stays empty where there are at least
    three classes, and one column (the last, where N > 1) has no class"""
    obs = (offset + rng.uniform(-3.0, 3.0, (T, N, D)) * rng.uniform(0.5, 20.0, (1, 1, D))).astype(np.float32)
    live = max(1, n_classes - 1) if n_classes >= 3 else n_classes
    cls = rng.integers(0, live, N).astype(np.int32)
    if N > 1:
        cls[-1] = n_classes if rng.integers(2) else -1
    k = {"none": None, "zero": np.zeros((T, N), np.uint8), "random": (rng.uniform(size=(T, N)) < 0.6).astype(np.uint8)}[keep]
    return obs, k, cls
