"""phx_gae restated in numpy, bit for bit (include/phantom_amd_gae.h): every operation the correctly rounded f32 one, through
policy_ref's exact fmaf, vectorised over the columns; and RLlib's formula in f64 with its forward error bound."""
import numpy as np

from policy_explore_ref import fsub
from policy_ref import fmaf, fmul


def _planes(reward, vf_pred, vf_next, terminated, truncated):
    r = np.asarray(reward, np.float32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    f = lambda x: np.zeros_like(r) if x is None else np.asarray(x, np.float32).reshape(T, -1)
    term = np.zeros(r.shape, bool) if terminated is None else np.asarray(terminated).reshape(T, -1) != 0
    cut = term | (np.asarray(truncated).reshape(T, -1) != 0)
    cut[T - 1] = True
    return T, r, f(vf_pred), f(vf_next), term, cut


def reads_vf_next(terminated, truncated):
    """bool [T, ...]: the elements of vf_next the definition reads (cut rows that are not terminated)"""
    tr = np.asarray(truncated) != 0
    term = np.zeros(tr.shape, bool) if terminated is None else np.asarray(terminated) != 0
    cut = term | tr
    cut[-1] = True
    return cut & ~term


def gae(reward, truncated, vf_pred=None, vf_next=None, terminated=None, gamma=0.99, lam=1.0):
    """(advantage, value_target) f32, the shape of `reward` ([T, ...]).  Elements of vf_next the definition does not read are
    not touched (they may hold anything, NaN included)."""
    shape = np.asarray(reward).shape
    T, r, v, vn, term, cut = _planes(reward, vf_pred, vf_next, terminated, truncated)
    gamma, lam = np.float32(gamma), np.float32(lam)
    gl = fmul(gamma, lam)
    adv = np.empty_like(r)
    zero = np.zeros(r.shape[1], np.float32)
    for t in range(T - 1, -1, -1):
        nv = np.where(term[t], zero, np.where(cut[t], vn[t], v[t + 1] if t + 1 < T else zero))
        c = np.where(cut[t], zero, adv[t + 1] if t + 1 < T else zero)
        d = fsub(fmaf(gamma, nv, r[t]), v[t])
        adv[t] = fmaf(gl, c, d)
    vt = (adv.astype(np.float64) + v.astype(np.float64)).astype(np.float32)       # one f32 add (the f64 sum of two f32 is exact)
    return adv.reshape(shape), vt.reshape(shape)


def gae_f64(reward, truncated, vf_pred=None, vf_next=None, terminated=None, gamma=0.99, lam=1.0):
    """RLlib's compute_advantages(use_gae=True) in f64 per trajectory segment -- delta = r + gamma v_next - v,
    discount_cumsum(delta, gamma lambda), value_targets = adv + v -- with the f32 gamma and lambda widened, and the forward
    error bounds of the f32 definition against it: (adv, vt, E_adv, E_vt), each [T, N] f64.
    E_t = gl E_{t+1} + 2^-24 (|gamma nv + r| + |d| + |gl c| + |adv_t|), E_T = 0, c = 0 at cuts (one half-ulp per rounded
    operation: the fmaf, the subtraction, the closing fmaf; the gl c term covers the rounding of gl itself, relative 2^-24);
    value_target: one more 2^-24 |vt|."""
    T, r, v, vn, term, cut = _planes(reward, vf_pred, vf_next, terminated, truncated)
    r, v, vn = r.astype(np.float64), v.astype(np.float64), vn.astype(np.float64)
    g = np.float64(np.float32(gamma))
    gl = g * np.float64(np.float32(lam))
    u = 2.0 ** -24
    adv, E = np.empty_like(r), np.empty_like(r)
    for t in range(T - 1, -1, -1):
        nv = np.where(term[t], 0.0, np.where(cut[t], vn[t], v[t + 1] if t + 1 < T else 0.0))
        c = np.where(cut[t], 0.0, adv[t + 1] if t + 1 < T else 0.0)
        e1 = np.where(cut[t], 0.0, E[t + 1] if t + 1 < T else 0.0)
        d = g * nv + r[t] - v[t]                       # delta_t
        adv[t] = gl * c + d                            # discount_cumsum, segment by segment
        E[t] = gl * e1 + u * (np.abs(g * nv + r[t]) + np.abs(d) + np.abs(gl * c) + np.abs(adv[t]))
    vt = adv + v
    return adv, vt, E, E + u * np.abs(vt)


def random_case(rng, T, N, p_trunc=0.12, p_term=0.06):
    """random planes [T, N] with independent per-column cut rows: truncations, terminations, rows with both flags,
    columns without a cut and (in the first six columns, as far as there are) every flag combination at rows 0 and T - 1"""
    f = lambda: rng.normal(0, 1, (T, N)).astype(np.float32)
    trunc = (rng.random((T, N)) < p_trunc).astype(np.uint8)
    term = (rng.random((T, N)) < p_term).astype(np.uint8)
    both = rng.random((T, N)) < 0.03
    trunc[both] = 1; term[both] = 1
    trunc[:, 9::5] = 0; term[:, 9::5] = 0              # some columns run uncut through the whole fragment
    for row in (0, T - 1):                             # every flag combination at the first and the last row
        for k, (a, b) in enumerate(((1, 0), (0, 1), (1, 1))):
            if k < N:
                trunc[row, (k + 3 * (row != 0)) % N], term[row, (k + 3 * (row != 0)) % N] = a, b
    return dict(reward=f(), vf_pred=f(), vf_next=f(), terminated=term, truncated=trunc)
