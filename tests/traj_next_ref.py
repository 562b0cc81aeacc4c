"""phx_traj_next restated in numpy (include/phantom_amd_traj.h): the header's reverse scan vectorised over the columns, the same
result built segment by segment on gae_masked_ref.segments, the gather, the elements of obs / new_obs a result depends on, and a
case generator on top of gae_masked_ref.random_case."""
import numpy as np

import gae_masked_ref as gm


def _planes(truncated, terminated, acted, new_obs_valid):
    tr = np.asarray(truncated)
    T = tr.shape[0]
    tr = tr.reshape(T, -1) != 0
    te = np.zeros(tr.shape, bool) if terminated is None else np.asarray(terminated).reshape(T, -1) != 0
    act = np.ones(tr.shape, bool) if acted is None else np.asarray(acted).reshape(T, -1) != 0
    nv = np.ones(tr.shape, bool) if new_obs_valid is None else np.asarray(new_obs_valid).reshape(T, -1) != 0
    return T, tr, te, act, nv


def scan(truncated, terminated=None, acted=None, new_obs_valid=None):
    """(next_row i32, next_terminated u8, next_truncated u8), the shape of `truncated` ([T, ...]): the header's scan, t from T - 1 down to 0"""
    shape = np.asarray(truncated).shape
    T, tr, te, act, nv = _planes(truncated, terminated, acted, new_obs_valid)
    N = tr.shape[1]
    nr, term, trunc = np.full(N, -1, np.int32), np.zeros(N, bool), np.zeros(N, bool)
    out_r, out_te, out_tr = np.empty((T, N), np.int32), np.empty((T, N), np.uint8), np.empty((T, N), np.uint8)
    for t in range(T - 1, -1, -1):
        c = te[t] | tr[t] | (t == T - 1)
        here = np.where(nv[t], np.int32(t), np.int32(-1))
        nr = np.where(c, here, np.where(nr < 0, here, nr))
        term = np.where(c, te[t], term)
        trunc = np.where(c, ~te[t] & tr[t], trunc)
        a = act[t]
        out_r[t] = np.where(a, nr, -1)
        out_te[t] = a & term
        out_tr[t] = a & trunc
        nr = np.where(a, np.int32(-1), nr)
        term, trunc = term & ~a, trunc & ~a
    return out_r.reshape(shape), out_te.reshape(shape), out_tr.reshape(shape)


def by_segments(truncated, terminated=None, acted=None, new_obs_valid=None):
    """the same three planes from the definition in words: per column, per segment of gae_masked_ref.segments ([T, N] planes)"""
    T, tr, te, act, nv = _planes(truncated, terminated, acted, new_obs_valid)
    N = tr.shape[1]
    case = dict(reward=np.zeros((T, N), np.float32), truncated=tr.astype(np.uint8), terminated=te.astype(np.uint8), acted=act.astype(np.uint8))
    out_r, out_te, out_tr = np.full((T, N), -1, np.int32), np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    for n in range(N):
        rows = np.flatnonzero(act[:, n]).tolist()
        for i, (t0, close, _) in enumerate(gm.segments(case, n)):
            t1 = rows[i + 1] if i + 1 < len(rows) else T
            last = close if close is not None else t1 - 1
            held = [u for u in range(t0, last + 1) if nv[u, n]]
            out_r[t0, n] = held[-1] if held else -1
            if close is not None:
                out_te[t0, n] = te[close, n]
                out_tr[t0, n] = (not te[close, n]) and tr[close, n]       # (row T - 1 without a flag: neither)
    return out_r, out_te, out_tr


def gather(next_row, acted, obs, new_obs):
    """next_obs [T, ..., D]: new_obs[next_row] where next_row >= 0, obs of the row itself where it is -1, +0.0 at hole rows -- the words
    are copied as 32-bit integers"""
    o, nob = np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(new_obs, np.float32)
    shape, D = o.shape, o.shape[-1]
    T = shape[0]
    o, nob = o.view(np.uint32).reshape(T, -1, D), nob.view(np.uint32).reshape(T, -1, D)
    nr = np.asarray(next_row).reshape(T, -1)
    act = np.ones(nr.shape, bool) if acted is None else np.asarray(acted).reshape(T, -1) != 0
    cols = np.arange(nr.shape[1])[None, :]
    src = nob[np.maximum(nr, 0), cols]                       # [T, N, D]
    out = np.where((nr >= 0)[..., None], src, o)
    out = np.where(act[..., None], out, np.uint32(0))
    return np.ascontiguousarray(out).view(np.float32).reshape(shape)


def traj_next(truncated, terminated=None, acted=None, new_obs_valid=None, obs=None, new_obs=None):
    """the call: (next_row, next_terminated, next_truncated, next_obs or None)"""
    nr, te, tr = scan(truncated, terminated, acted, new_obs_valid)
    return nr, te, tr, (None if obs is None else gather(nr, acted, obs, new_obs))


def reads(next_row, acted=None):
    """{"obs", "new_obs"}: bool [T, ...], the elements (all D words of each) that a result depends on: new_obs[next_row] of a trajectory
    row with next_row >= 0, obs of a trajectory row with next_row == -1"""
    nr = np.asarray(next_row)
    shape, T = nr.shape, nr.shape[0]
    nr = nr.reshape(T, -1)
    act = np.ones(nr.shape, bool) if acted is None else np.asarray(acted).reshape(T, -1) != 0
    rd_new = np.zeros(nr.shape, bool)
    t, n = np.nonzero(act & (nr >= 0))
    rd_new[nr[t, n], n] = True
    return {"obs": (act & (nr < 0)).reshape(shape), "new_obs": rd_new.reshape(shape)}


def random_case(rng, T, N, density=0.4, D=None):
    """gae_masked_ref.random_case's flag and acted planes plus a validity plane of `density`; with D also obs / new_obs [T, N, D] of
    distinct finite words (so that a wrong source shows)"""
    c = gm.random_case(rng, T, N)
    case = dict(truncated=c["truncated"], terminated=c["terminated"], acted=c["acted"],
                new_obs_valid=(rng.random((T, N)) < density).astype(np.uint8))
    if D is not None:
        case["obs"] = (1.0 + np.arange(T * N * D, dtype=np.float32)).reshape(T, N, D)
        case["new_obs"] = -(1.0 + np.arange(T * N * D, dtype=np.float32)).reshape(T, N, D)
    return case


def features(case):
    """which of the classes of row a case holds (the CPU test asserts them for N >= 63, T >= 15)"""
    T, tr, te, act, nv = _planes(case["truncated"], case.get("terminated"), case.get("acted"), case.get("new_obs_valid"))
    nr, nte, ntr = scan(case["truncated"], case.get("terminated"), case.get("acted"), case.get("new_obs_valid"))
    rows = np.arange(T)[:, None]
    g = dict(reward=np.zeros(tr.shape, np.float32), truncated=tr, terminated=te, acted=act)
    hole_close = False
    for n in range(tr.shape[1]):
        hole_close |= any(close is not None and close != t0 and close != T - 1 for t0, close, _ in gm.segments(g, n))
    return dict(none=bool((act & (nr < 0)).any()), own=bool((act & (nr == rows)).any()), later=bool((act & (nr > rows)).any()),
                terminated=bool(nte.any()), truncated=bool(ntr.any()), closed_on_a_hole_row=bool(hole_close),
                incomplete=bool((act & (nr < 0) & (nte == 0) & (ntr == 0)).any()))
