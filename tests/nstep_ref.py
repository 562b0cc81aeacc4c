"""phx_nstep restated in numpy, bit for bit (include/phantom_amd_nstep.h): the header's loop run for all elements at once, one round
per hop, every operation the correctly rounded f32 one (policy_ref's exact fmaf, one f32 multiply for p); the elements of reward and
next_obs a result depends on; why each chain stopped; and a case generator."""
import numpy as np

from policy_ref import fmaf, fmul

OUTPUTS = ("nstep_reward", "nstep_discount", "nstep_last", "nstep_terminated", "nstep_truncated", "nstep_next_row", "nstep_next_obs")
STOPS = ("m_equals_n", "terminated", "truncated", "no_successor", "incomplete_successor", "incomplete_t0")


def succ_rows(acted, T, N):
    """i32 [T, N]: the column's next trajectory row after t, -1: none (acted None: t + 1, -1 in the last row)"""
    out = np.empty((T, N), np.int32)
    if acted is None:
        out[:] = np.arange(1, T + 1, dtype=np.int32)[:, None]
        out[T - 1] = -1
        return out
    act = np.asarray(acted).reshape(T, N) != 0
    nx = np.full(N, -1, np.int32)
    for t in range(T - 1, -1, -1):
        out[t] = nx
        nx = np.where(act[t], np.int32(t), nx)
    return out


def _fold(reward, truncated, terminated, acted, next_row, n, gamma):
    r = np.asarray(reward, np.float32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    N = r.shape[1]
    tr = np.asarray(truncated).reshape(T, N) != 0
    te = np.zeros((T, N), bool) if terminated is None else np.asarray(terminated).reshape(T, N) != 0
    act = np.ones((T, N), bool) if acted is None else np.asarray(acted).reshape(T, N) != 0
    rows = np.broadcast_to(np.arange(T, dtype=np.int32)[:, None], (T, N))
    nr = rows if next_row is None else np.asarray(next_row, np.int32).reshape(T, N)
    succ = succ_rows(acted, T, N)
    cols = np.broadcast_to(np.arange(N)[None, :], (T, N))
    gamma = np.float32(gamma)
    u, active = rows.copy(), act.copy()
    G, p = np.zeros((T, N), np.float32), np.ones((T, N), np.float32)
    last, lnr = np.full((T, N), -1, np.int32), np.full((T, N), -1, np.int32)
    lte, ltr = np.zeros((T, N), bool), np.zeros((T, N), bool)
    m = np.zeros((T, N), np.int32)
    stop = np.full((T, N), -1, np.int8)                       # index into STOPS, -1 at hole rows
    rd_r = np.zeros((T, N), bool)
    for hop in range(int(n)):                                 # every active element has folded `hop` transitions so far
        if not active.any():
            break
        term, trunc, nru, ru, su = te[u, cols], ~te[u, cols] & tr[u, cols], nr[u, cols], r[u, cols], succ[u, cols]
        cmp = term | trunc | (nru >= 0)
        fold = active & (cmp | (hop == 0))
        stop = np.where(active & ~fold, np.int8(STOPS.index("incomplete_successor")), stop)
        with np.errstate(invalid="ignore", over="ignore"):
            G = np.where(fold, ru if hop == 0 else fmaf(p, ru, G), G)
            p = np.where(fold, fmul(p, gamma), p)
        rd_r[u[fold], cols[fold]] = True
        last, lnr = np.where(fold, u, last), np.where(fold, nru, lnr)
        lte, ltr = np.where(fold, term, lte), np.where(fold, trunc, ltr)
        m = m + fold
        why = np.where(~cmp, STOPS.index("incomplete_t0"), np.where(term, STOPS.index("terminated"), np.where(trunc, STOPS.index("truncated"),
                       np.where(hop + 1 == n, STOPS.index("m_equals_n"), np.where(su < 0, STOPS.index("no_successor"), -1))))).astype(np.int8)
        stop = np.where(fold & (why >= 0), why, stop)
        active = fold & (why < 0)
        u = np.where(active, su, u)
    zero = np.float32(0.0)
    out = dict(nstep_reward=np.where(act, G, zero), nstep_discount=np.where(act, p, zero), nstep_last=last,
               nstep_terminated=lte.astype(np.uint8), nstep_truncated=ltr.astype(np.uint8), nstep_next_row=lnr, succ_row=succ)
    return out, dict(reward=rd_r, m=m, stop=stop, acted=act)


def nstep(reward, truncated, terminated=None, acted=None, next_row=None, next_obs=None, n=3, gamma=0.99):
    """the call: a dict of the seven outputs (nstep_next_obs None without next_obs) plus succ_row, each the shape of `reward` ([T, ...])"""
    shape = np.asarray(reward).shape
    out, _ = _fold(reward, truncated, terminated, acted, next_row, n, gamma)
    last = out["nstep_last"]
    out = {k: v.reshape(shape) for k, v in out.items()}
    out["nstep_next_obs"] = None
    if next_obs is not None:
        o = np.ascontiguousarray(next_obs, np.float32)
        D = o.shape[-1]
        w = o.view(np.uint32).reshape(shape[0], -1, D)
        cols = np.arange(w.shape[1])[None, :]
        got = np.where((last >= 0)[..., None], w[np.maximum(last, 0), cols], np.uint32(0))      # words copied as integers
        out["nstep_next_obs"] = np.ascontiguousarray(got).view(np.float32).reshape(o.shape)
    return out


def reads(reward, truncated, terminated=None, acted=None, next_row=None, n=3, gamma=0.99):
    """{"reward", "next_obs"}: bool [T, ...], the elements a result depends on (next_obs: all D words of the element): the rewards of the
    transitions folded, next_obs at `last` of every trajectory row"""
    shape = np.asarray(reward).shape
    out, info = _fold(reward, truncated, terminated, acted, next_row, n, gamma)
    last = out["nstep_last"]
    rd_o = np.zeros(last.shape, bool)
    t, c = np.nonzero(last >= 0)
    rd_o[last[t, c], c] = True
    return {"reward": info["reward"].reshape(shape), "next_obs": rd_o.reshape(shape)}


def stats(reward, truncated, terminated=None, acted=None, next_row=None, n=3, gamma=0.99):
    """(m i32 [T, N]: transitions folded, 0 at hole rows; stop i8 [T, N]: index into STOPS of why the chain ended, -1 at hole rows)"""
    _, info = _fold(reward, truncated, terminated, acted, next_row, n, gamma)
    return info["m"], info["stop"]


DENSITIES = (1.0, 0.5, 0.15)


def random_case(rng, T, N, D=None, p_trunc=0.08, p_term=0.05, p_incomplete=0.1):
    """planes [T, N] of a phx_nstep call, more general than a rollout produces them: column c acts with density DENSITIES[c % 3];
    flags and an incomplete transition (next_row -1 without a flag) can stand at ANY row, trajectory row or not; next_row is otherwise a
    row in [t, T); rewards are N(0, 1) with a few -0.0.  Columns 10 .. 12, where the shape has them: one that never acts, one that
    acts in every row, and one that acts in every row with neither a flag nor an incomplete row (its chains end at m == n or at the
    fragment's end).  With D also next_obs [T, N, D] of distinct finite words, so that a wrong source row shows."""
    dens = np.array([DENSITIES[c % 3] for c in range(N)])
    acted = (rng.random((T, N)) < dens[None, :]).astype(np.uint8)
    trunc = (rng.random((T, N)) < p_trunc).astype(np.uint8)
    term = (rng.random((T, N)) < p_term).astype(np.uint8)
    both = rng.random((T, N)) < 0.02
    trunc[both] = 1; term[both] = 1
    trunc[trunc != 0] = rng.choice(np.array([1, 2, 255], np.uint8), size=int((trunc != 0).sum()))      # != 0 counts, whatever the value
    rows = np.arange(T)[:, None]
    next_row = (rows + np.floor(rng.random((T, N)) * (T - rows))).astype(np.int32)
    next_row[rng.random((T, N)) < p_incomplete] = -1
    reward = rng.normal(0, 1, (T, N)).astype(np.float32)
    reward[rng.random((T, N)) < 0.02] = np.float32(-0.0)
    if N > 12:
        acted[:, 10] = 0
        acted[:, 11] = 1
        acted[:, 12] = 1; trunc[:, 12] = 0; term[:, 12] = 0; next_row[:, 12] = np.arange(T)
    case = dict(reward=reward, truncated=trunc, terminated=term, acted=acted, next_row=next_row)
    if D is not None:
        case["next_obs"] = (1.0 + np.arange(T * N * D, dtype=np.float32)).reshape(T, N, D)
    return case


def plain_loop(reward, truncated, terminated, acted, next_row, n, gamma):
    """the header's definition as a plain Python double loop over [T, N] planes, written from the header and from nothing else:
    (succ_row or None, nstep_reward, nstep_discount, nstep_last, nstep_terminated, nstep_truncated, nstep_next_row)"""
    T, N = reward.shape
    f32 = np.float32
    succ = None if acted is None else np.full((T, N), -1, np.int32)
    G_o, p_o = np.zeros((T, N), f32), np.zeros((T, N), f32)
    last_o, nr_o = np.full((T, N), -1, np.int32), np.full((T, N), -1, np.int32)
    te_o, tr_o = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    for c in range(N):
        is_row = lambda t: acted is None or acted[t, c] != 0

        def successor(t):
            for t2 in range(t + 1, T):
                if is_row(t2):
                    return t2
            return -1
        term = lambda u: terminated is not None and terminated[u, c] != 0
        trunc = lambda u: (not term(u)) and truncated[u, c] != 0
        complete = lambda u: term(u) or trunc(u) or next_row is None or next_row[u, c] >= 0
        for t0 in range(T):
            if succ is not None:
                succ[t0, c] = successor(t0)
            if not is_row(t0):
                continue
            u, m, p, G, last = t0, 0, f32(1.0), f32(0.0), -1
            while True:
                cmp = complete(u)
                if m > 0 and not cmp:
                    break
                G = reward[u, c] if m == 0 else fmaf(p, reward[u, c], G)[()]
                last, m, p = u, m + 1, fmul(p, f32(gamma))[()]
                if (not cmp) or term(u) or trunc(u) or m == n:
                    break
                u = successor(u)
                if u < 0:
                    break
            G_o[t0, c], p_o[t0, c], last_o[t0, c] = G, p, last
            te_o[t0, c], tr_o[t0, c] = term(last), trunc(last)
            nr_o[t0, c] = last if next_row is None else next_row[last, c]
    return succ, G_o, p_o, last_o, te_o, tr_o, nr_o
