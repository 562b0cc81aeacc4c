"""phx_episode_stats restated in numpy, bit for bit (include/phantom_amd_episodes.h): the header's scan run for all output columns at
once, a row and a group member at a time, every operation the correctly rounded f32 (f64 where the header says so) one; the
per-column records; the reduction in the header's lane / tree order; and a case generator."""
import numpy as np

DTYPE = np.dtype([("count", "<i8"), ("len_sum", "<i8"), ("ret_sum", "<f8"), ("ret_sumsq", "<f8"), ("ret_min", "<f4"), ("ret_max", "<f4"),
                  ("len_min", "<i4"), ("len_max", "<i4")])
INT_FIELDS = ("count", "len_sum", "len_min", "len_max")
SUM_FIELDS = ("ret_sum", "ret_sumsq")
VALUE_FIELDS = ("ret_min", "ret_max")                   # compared by value: +0.0 and -0.0 may tie either way
LANES = 256
INT32_MAX = np.iinfo(np.int32).max


def empty(n):
    """n empty records"""
    s = np.zeros(n, DTYPE)
    s["ret_min"], s["ret_max"], s["len_min"], s["len_max"] = np.inf, -np.inf, INT32_MAX, -1
    return s


def scan(reward, truncated, terminated=None, acted=None, reward_valid=None, G=1, carry=None):
    """the scan: ``(episode_return f32 [T, C], episode_len i32 [T, C], col_stats [C], (carry_return f32 [C], carry_len i32 [C]))``.
    The planes are [T, N] (or [T, ...]: flattened); ``carry``: the (return, length) pair to start from, None: (+0.0, -1); the pair
    returned is the state after row T - 1 (what the call writes back when the carry is given)"""
    r = np.asarray(reward, np.float32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    N = r.shape[1]
    assert N % G == 0
    C = N // G
    flat = lambda x: None if x is None else np.asarray(x).reshape(T, N)
    tr, te, ac, rv = flat(truncated), flat(terminated), flat(acted), flat(reward_valid)
    ret = np.zeros(C, np.float32) if carry is None else np.array(carry[0], np.float32).reshape(C).copy()
    ln = np.full(C, -1, np.int32) if carry is None else np.array(carry[1], np.int32).reshape(C).copy()
    e_ret, e_len = np.zeros((T, C), np.float32), np.full((T, C), -1, np.int32)
    col = empty(C)
    zero = np.float32(0.0)
    for t in range(T):
        any_act, all_flag = np.zeros(C, bool), np.ones(C, bool)
        for g in range(G):
            n = np.arange(C) * G + g
            present = np.ones(C, bool) if rv is None else rv[t, n] == 1
            act = np.ones(C, bool) if ac is None else ac[t, n] != 0
            opens = (present | act) & (ln < 0)
            ret = np.where(opens, zero, ret)
            ln = np.where(opens, np.int32(0), ln)
            with np.errstate(invalid="ignore", over="ignore"):
                ret = np.where(present, (ret + r[t, n]).astype(np.float32), ret)
            any_act |= act
            all_flag &= (tr[t, n] != 0) if te is None else ((te[t, n] != 0) | (tr[t, n] != 0))
        ln = np.where(any_act, ln + np.int32(1), ln).astype(np.int32)
        closes = all_flag & (ln >= 0)
        e_ret[t], e_len[t] = np.where(closes, ret, zero), np.where(closes, ln, np.int32(-1))
        d = ret.astype(np.float64)
        col["count"] += closes
        col["len_sum"] += np.where(closes, ln, 0)
        col["ret_sum"] = np.where(closes, col["ret_sum"] + d, col["ret_sum"])
        col["ret_sumsq"] = np.where(closes, col["ret_sumsq"] + d * d, col["ret_sumsq"])
        col["ret_min"] = np.where(closes & (ret < col["ret_min"]), ret, col["ret_min"])
        col["ret_max"] = np.where(closes & (ret > col["ret_max"]), ret, col["ret_max"])
        col["len_min"] = np.where(closes & (ln < col["len_min"]), ln, col["len_min"])
        col["len_max"] = np.where(closes & (ln > col["len_max"]), ln, col["len_max"])
        ret = np.where(closes, zero, ret)
        ln = np.where(closes, np.int32(-1), ln).astype(np.int32)
    return e_ret, e_len, col, (ret, ln)


def ordered_sum(x):
    """the header's order for one f64 sum over x[0 .. M): 256 lane values a_i = ((+0.0 + x_i) + x_{i+256}) + .., then the tree"""
    x = np.asarray(x, np.float64)
    a = np.zeros(LANES, np.float64)
    for base in range(0, x.size, LANES):
        part = x[base:base + LANES]
        a[:part.size] = a[:part.size] + part
    h = LANES // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def reduce(col, K):
    """summary [K]: class k combines the columns c = j * K + k"""
    C = col.shape[0]
    assert C % K == 0
    out = empty(K)
    for k in range(K):
        m = col[k::K]
        out["count"][k], out["len_sum"][k] = m["count"].sum(), m["len_sum"].sum()
        out["len_min"][k], out["len_max"][k] = m["len_min"].min(), m["len_max"].max()
        out["ret_min"][k], out["ret_max"][k] = m["ret_min"].min(), m["ret_max"].max()
        out["ret_sum"][k], out["ret_sumsq"][k] = ordered_sum(m["ret_sum"]), ordered_sum(m["ret_sumsq"])
    return out


def episode_stats(reward, truncated, terminated=None, acted=None, reward_valid=None, G=1, K=1, carry=None):
    """the call: a dict of episode_return, episode_len, col_stats, summary, carry_return, carry_len"""
    e_ret, e_len, col, (cr, cl) = scan(reward, truncated, terminated, acted, reward_valid, G, carry)
    return dict(episode_return=e_ret, episode_len=e_len, col_stats=col, summary=reduce(col, K), carry_return=cr, carry_len=cl)


def assert_same_stats(got, want, what=""):
    """records: bit equality on every field but ret_min / ret_max, which compare by value"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}{got.shape} records, expected {want.shape}"
    for f in INT_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=what + f)
    for f in SUM_FIELDS:
        np.testing.assert_array_equal(got[f].view(np.uint64), want[f].view(np.uint64), err_msg=what + f)
    for f in VALUE_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=what + f)


def gpu_shapes(ep_k):
    """the (T, C, G) list tests/test_gpu_episode_stats.py walks (ep_k: the scan's chunk depth, read from the kernel's source): every T
    with every C for G = 1, and G in (2, 3) with C in (1, 64, 65)"""
    ts = (1, 2, ep_k - 1, ep_k, ep_k + 1, 2 * ep_k + 1, 40)
    return [(T, C, 1) for T in ts for C in (1, 63, 64, 65, 257)] + [(T, C, G) for T in ts for G in (2, 3) for C in (1, 64, 65)]


def case(T, C, G=1, seed=0):
    """the case both test files use for a shape"""
    return random_case(np.random.default_rng([seed, T, C, G]), T, C * G, G)


def random_case(rng, T, N, G=1, p_flag=0.2, p_act=0.6, p_valid=0.6):
    """planes [T, N] of a fragment with holes: rewards of mixed sign and magnitude (so that f32 sums round), flags that close an
    output column (all G members in one row) with probability about ``p_flag`` per row, some columns' members flagged alone,
    terminated and truncated both in use, reward_valid with the value 2 among the zeros (only 1 counts), rewards that arrive in rows
    without an action.  With T >= 4 output column 0 closes at rows T // 3 and 2 T // 3 and is open after the last row.  Input columns of output column 2 (when there is one) never act, get no reward and carry no flag; output
    column 1's members act, are rewarded and are flagged in no row but are open: it ends with an episode open"""
    C = N // G
    reward = (rng.normal(0, 1, (T, N)) * 10.0 ** rng.integers(-3, 3, (T, N))).astype(np.float32)
    acted = (rng.random((T, N)) < p_act).astype(np.uint8) * rng.integers(1, 4, (T, N)).astype(np.uint8)
    valid = np.where(rng.random((T, N)) < p_valid, 1, rng.integers(0, 2, (T, N)) * 2).astype(np.uint8)
    close = rng.random((T, C)) < p_flag                                         # the output column closes in this row
    which = rng.random((T, C)) < 0.5                                            # .. by termination (else truncation)
    member = lambda x: np.repeat(x, G, axis=1)
    lone = rng.random((T, N)) < 0.1                                             # a member flagged alone (closes only where G == 1)
    terminated = ((member(close & which) | (lone & (rng.random((T, N)) < 0.5)))).astype(np.uint8)
    truncated = ((member(close & ~which) | (lone & (terminated == 0)))).astype(np.uint8) * rng.integers(1, 3, (T, N)).astype(np.uint8)
    both = member(close) & (rng.random((T, N)) < 0.2)
    terminated[both], truncated[both] = 1, 1
    if T >= 4:                                                                  # output column 0: closes twice, ends with an episode open
        a, b = T // 3, (2 * T) // 3
        terminated[a, :G], truncated[b, :G], acted[a, 0], acted[b, 0] = 1, 1, 1, 1
        terminated[T - 1, :G], truncated[T - 1, :G], acted[T - 1, 0] = 0, 0, 1
    if C > 1:
        sl = slice(G, 2 * G)
        terminated[:, sl], truncated[:, sl], acted[:, sl], valid[:, sl] = 0, 0, 1, 1
    if C > 2:
        sl = slice(2 * G, 3 * G)
        terminated[:, sl], truncated[:, sl], acted[:, sl], valid[:, sl] = 0, 0, 0, 0
    return dict(reward=reward, truncated=truncated, terminated=terminated, acted=acted, reward_valid=valid)
