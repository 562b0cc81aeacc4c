"""phx_gae_masked restated in numpy, bit for bit (include/phantom_amd_gae.h): the definition's row step, every operation the
correctly rounded f32 one, vectorised over the columns like gae_ref.gae; the elements of the inputs the definition reads; the
per-column compaction that reduces it to gae_ref.gae; and a case generator on top of gae_ref.random_case."""
import numpy as np

import gae_ref
from policy_explore_ref import fsub
from policy_ref import fmaf, fmul


def fadd(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) + np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def _flags(T, shape, terminated, truncated, acted, reward_valid):
    te = np.zeros(shape, bool) if terminated is None else np.asarray(terminated).reshape(T, -1) != 0
    crow = te | (np.asarray(truncated).reshape(T, -1) != 0)
    crow[T - 1] = True
    act = np.ones(shape, bool) if acted is None else np.asarray(acted).reshape(T, -1) != 0
    present = np.ones(shape, bool) if reward_valid is None else np.asarray(reward_valid).reshape(T, -1) == 1
    return te, crow, act, present


def gae_masked(reward, truncated, vf_pred=None, vf_next=None, terminated=None, acted=None, reward_valid=None, gamma=0.99, lam=1.0):
    """(advantage, value_target, reward_sum) f32, the shape of `reward` ([T, ...]): the header's row step, t from T - 1 down to 0.
    What the definition does not read may hold anything: it is selected away, never multiplied."""
    shape = np.asarray(reward).shape
    r = np.asarray(reward, np.float32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    f = lambda x: np.zeros_like(r) if x is None else np.asarray(x, np.float32).reshape(T, -1)
    v, vn = f(vf_pred), f(vf_next)
    te, crow, act, present = _flags(T, r.shape, terminated, truncated, acted, reward_valid)
    gamma, lam = np.float32(gamma), np.float32(lam)
    gl = fmul(gamma, lam)
    N = r.shape[1]
    zero = np.zeros(N, np.float32)
    acc, nv, adv_next, v_next = zero.copy(), zero.copy(), zero.copy(), zero.copy()
    empty, cut, term = np.ones(N, bool), np.ones(N, bool), np.zeros(N, bool)
    adv, vt, rs_out = np.empty_like(r), np.empty_like(r), np.empty_like(r)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            c = crow[t]
            empty, cut, term = empty | c, cut | c, np.where(c, te[t], term)
            nv = np.where(c, np.where(te[t], zero, vn[t]), nv)
            acc = np.where(present[t], np.where(empty, r[t], fadd(r[t], acc)), acc)
            empty = empty & ~present[t]
            a = act[t]
            rs = np.where(empty, zero, acc)
            nvv = np.where(term, zero, np.where(cut, nv, v_next))
            cc = np.where(cut, zero, adv_next)
            d = fsub(fmaf(gamma, nvv, rs), v[t])
            ad = fmaf(gl, cc, d)
            adv[t] = np.where(a, ad, zero)
            vt[t] = np.where(a, fadd(ad, v[t]), zero)
            rs_out[t] = np.where(a, rs, zero)
            adv_next, v_next = np.where(a, ad, adv_next), np.where(a, v[t], v_next)
            empty, cut, term = empty | a, cut & ~a, term & ~a
    return adv.reshape(shape), vt.reshape(shape), rs_out.reshape(shape)


def reads(truncated, terminated=None, acted=None, reward_valid=None):
    """{"vf_next", "vf_pred", "reward"}: bool [T, ...], the elements an output depends on.  vf_pred: the trajectory rows; reward: the
    present rewards of a segment up to and including its closing cut row; vf_next: that cut row unless it terminates."""
    shape = np.asarray(truncated).shape
    T = shape[0]
    te, crow, act, present = _flags(T, (T, int(np.prod(shape[1:]))), terminated, truncated, acted, reward_valid)
    rd_r, rd_n = np.zeros_like(te), np.zeros_like(te)
    live = np.zeros(te.shape[1], bool)                      # forwards: inside a segment that no cut row has closed yet
    for t in range(T):
        live = live | act[t]
        rd_r[t] = live & present[t]
        rd_n[t] = live & crow[t] & ~te[t]
        live = live & ~crow[t]
    return {"vf_next": rd_n.reshape(shape), "vf_pred": act.reshape(shape), "reward": rd_r.reshape(shape)}


def segments(case, n):
    """column n: [(t0, closing cut row or None, [rows of the rewards that count, ascending])] for every trajectory row t0"""
    T = case["reward"].shape[0]
    te, crow, act, present = (x[:, n] for x in _flags(T, case["reward"].shape, case.get("terminated"), case["truncated"], case.get("acted"),
                                                      case.get("reward_valid")))
    rows = np.flatnonzero(act).tolist()
    out = []
    for i, t0 in enumerate(rows):
        t1 = rows[i + 1] if i + 1 < len(rows) else T
        cuts = [t for t in range(t0, t1) if crow[t]]
        close = cuts[0] if cuts else None
        last = close if close is not None else t1 - 1
        out.append((t0, close, [t for t in range(t0, last + 1) if present[t]]))
    return out


def compact(case, n):
    """column n compacted to its trajectory rows: (rows, planes [M, 1] for gae_ref.gae, segment sums [M])"""
    segs = segments(case, n)
    M = len(segs)
    f = lambda k: None if case.get(k) is None else np.asarray(case[k])[:, n]
    r, v, vn, te = f("reward"), f("vf_pred"), f("vf_next"), f("terminated")
    out = dict(reward=np.zeros((M, 1), np.float32), vf_pred=None if v is None else np.zeros((M, 1), np.float32),
               vf_next=None if vn is None else np.zeros((M, 1), np.float32), terminated=np.zeros((M, 1), np.uint8),
               truncated=np.zeros((M, 1), np.uint8))
    for i, (t0, close, rew_rows) in enumerate(segs):
        acc = np.float32(0.0)
        for j, t in enumerate(reversed(rew_rows)):          # added from the last one down; the first one assigned
            acc = r[t] if j == 0 else fadd(r[t], acc)
        out["reward"][i, 0] = acc
        if v is not None:
            out["vf_pred"][i, 0] = v[t0]
        if close is not None:
            out["truncated"][i, 0] = 1
            out["terminated"][i, 0] = te is not None and te[close] != 0
            if vn is not None:
                out["vf_next"][i, 0] = vn[close]
    return [s[0] for s in segs], out, out["reward"][:, 0].copy()


DENSITIES = (1.0, 0.5, 0.1)


def random_case(rng, T, N, p_trunc=0.12, p_term=0.06):
    """gae_ref.random_case plus `acted` (column n acts with density DENSITIES[n % 3]) and `reward_valid` (0 / 1 / 2) planes, and, in
    columns 10 .. 15 as far as the shape has them, the shapes of trajectory the scan can get wrong (features() names them)"""
    case = gae_ref.random_case(rng, T, N, p_trunc, p_term)
    dens = np.array([DENSITIES[n % 3] for n in range(N)])
    acted = (rng.random((T, N)) < dens[None, :]).astype(np.uint8)
    rv = rng.choice(np.array([0, 1, 2], np.uint8), size=(T, N), p=[0.25, 0.65, 0.10])
    tr, te = case["truncated"], case["terminated"]
    if N > 15:
        acted[:, 10] = 0                                    # no trajectory row at all
        acted[T - 1, 11] = 0; acted[0, 11] = 1              # row T - 1 is not a trajectory row
        acted[0, 12] = 0; acted[T - 1, 12] = 1              # row 0 is not one
        if T >= 8:
            acted[1, 13] = 1; acted[2:7, 13] = 0            # one segment, rows 1 .. 6, with two cut rows, neither on an acted row:
            tr[1:7, 13] = 0; te[1:7, 13] = 0
            tr[3, 13] = 1; te[5, 13] = 1                    # a truncating one closes it, a terminating one follows
            acted[1, 14] = 1; acted[2:7, 14] = 0
            tr[1:7, 14] = 0; te[1:7, 14] = 0
            te[4, 14] = 1; rv[1:7, 14] = 1                  # a terminating cut on a non-acted row closes this one
            acted[1, 15] = acted[4, 15] = 1; acted[2:4, 15] = 0
            rv[1:4, 15] = [0, 2, 0]                         # a segment with no present reward
    case.update(acted=acted, reward_valid=rv)
    return case


def features(case):
    """which of the hard shapes a case holds (the CPU test asserts them on the generated case for N >= 63, T >= 15)"""
    T, N = case["reward"].shape
    te, crow, act, present = _flags(T, (T, N), case["terminated"], case["truncated"], case["acted"], case["reward_valid"])
    out = dict(no_trajectory_row=bool((~act.any(axis=0)).any()), last_row_not_acted=bool((act.any(axis=0) & ~act[T - 1]).any()),
               first_row_not_acted=bool((act.any(axis=0) & ~act[0]).any()), two_cut_rows=False, trunc_cut_on_hole=False,
               term_cut_on_hole=False, no_present_reward=False, reward_valid_values=sorted(set(np.unique(case["reward_valid"]).tolist())),
               densities=sorted({round(float(act[:, 16 + (n - 16) % 3::3].mean()), 1) for n in range(3)} if N > 18 else []))
    for n in range(N):
        rows = np.flatnonzero(act[:, n]).tolist()
        for i, (t0, close, rew_rows) in enumerate(segments(case, n)):
            t1 = rows[i + 1] if i + 1 < len(rows) else T
            out["two_cut_rows"] |= int(crow[t0:t1, n].sum()) >= 2
            out["no_present_reward"] |= not rew_rows
            if close is not None and close != t0 and close != T - 1:
                out["term_cut_on_hole"] |= bool(te[close, n])
                out["trunc_cut_on_hole"] |= not te[close, n]
    return out
