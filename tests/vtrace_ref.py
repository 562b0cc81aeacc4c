"""phx_vtrace restated in numpy, bit for bit (include/phantom_amd_vtrace.h): every operation the correctly rounded f32 one, through
policy_ref's exact fmaf and policy_explore_ref's exp, vectorised over the columns; RLlib's formula in f64 with its forward error
bound; and the random cases the tests share."""
import numpy as np

import gae_ref
from gae_ref import _planes, reads_vf_next  # noqa: F401  (reads_vf_next: the same elements of vf_next are read as in phx_gae)
from policy_explore_ref import exp_def, fsub
from policy_ref import fmaf, fmul

CLAMP = np.float32(20.0)
EXP_ULP = 0.92                 # the defined exp is within 0.92 ulp of exp over [-20, 20] (include/phantom_amd.h)


def _fadd(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) + np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def log_ratio(behaviour_logp, target_logp):
    """the clamped log importance ratio l, f32, the shape of the planes"""
    lr = fsub(target_logp, behaviour_logp)
    return np.where(lr < -CLAMP, -CLAMP, np.where(lr > CLAMP, CLAMP, lr)).astype(np.float32)


def weights(behaviour_logp, target_logp, gamma, lam, rho_bar, c_bar, pg_rho_bar):
    """(rho, rc, gc, rp) f32: the per-element part of the definition"""
    rho = exp_def(log_ratio(behaviour_logp, target_logp))
    clip = lambda bar: np.where(rho < np.float32(bar), rho, np.float32(bar)).astype(np.float32)
    return rho, clip(rho_bar), fmul(np.float32(gamma), fmul(np.float32(lam), clip(c_bar))), clip(pg_rho_bar)


def vtrace(reward, truncated, vf_pred, behaviour_logp, target_logp, vf_next=None, terminated=None, gamma=0.99, lam=1.0,
           rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0):
    """(vs, pg_advantage) f32, the shape of `reward` ([T, ...]).  Elements of vf_next the definition does not read are not touched
    (they may hold anything, NaN included)."""
    shape = np.asarray(reward).shape
    T, r, v, vn, term, cut = _planes(reward, vf_pred, vf_next, terminated, truncated)
    flat = lambda x: np.asarray(x, np.float32).reshape(T, -1)
    _, rc, gc, rp = weights(flat(behaviour_logp), flat(target_logp), gamma, lam, rho_bar, c_bar, pg_rho_bar)
    gamma = np.float32(gamma)
    acc, vs, pg = np.empty_like(r), np.empty_like(r), np.empty_like(r)
    zero = np.zeros(r.shape[1], np.float32)
    for t in range(T - 1, -1, -1):
        last = t + 1 == T
        nv = np.where(term[t], zero, np.where(cut[t], vn[t], zero if last else v[t + 1]))
        nvs = np.where(term[t], zero, np.where(cut[t], vn[t], zero if last else vs[t + 1]))
        c = np.where(cut[t], zero, zero if last else acc[t + 1])
        td = fsub(fmaf(gamma, nv, r[t]), v[t])
        acc[t] = fmaf(gc[t], c, fmul(rc[t], td))
        vs[t] = _fadd(acc[t], v[t])
        pg[t] = fmul(rp[t], fsub(fmaf(gamma, nvs, r[t]), v[t]))
    return vs.reshape(shape), pg.reshape(shape)


def vtrace_f64(reward, truncated, vf_pred, behaviour_logp, target_logp, vf_next=None, terminated=None, gamma=0.99, lam=1.0,
               rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0):
    """RLlib's vtrace_torch.from_importance_weights in f64 per trajectory segment -- rho = exp(l) with the f32 clamped log-ratio l
    widened and np.exp, delta = min(rho, rho_bar) (r + gamma v_next - v), acc_t = delta_t + gamma lambda min(rho, c_bar) acc_{t+1},
    vs = acc + v, pg = min(rho, pg_rho_bar) (r + gamma vs_next - v) -- with the f32 parameters widened, and the first-order
    forward error bounds of the f32 definition against it: (vs, pg, E_vs, E_pg), each [T, N] f64.  With u = 2^-24 per rounded
    operation and e = 2 * 0.92 u for the defined exp (0.92 ulp, an ulp at most 2^-23 of the value; min(., bar) does not grow it,
    relative to the clipped value):
      gc = gamma (lambda min(rho, c_bar)): two multiplies on top of the exp, relative error (e + 2 u)
      d  = fmaf(gamma, nv, r) - v:         e_d = u (|gamma nv + r| + |d|)                      (nv is an input: exact)
      m  = rc d:                           e_m = rc e_d + (e + u) |m|
      E_t    = gc E_{t+1} + (e + 2 u) |gc c| + e_m + u |acc_t|,   E_T = 0, c = 0 at cuts
      E_vs,t = E_t + u |vs_t|
      q  = fmaf(gamma, nvs, r) - v:        e_q = gamma E_vs,t+1 (not at cuts) + u (|gamma nvs + r| + |q|)
      E_pg,t = rp e_q + (e + u) |pg_t|"""
    T, r, v, vn, term, cut = _planes(reward, vf_pred, vf_next, terminated, truncated)
    r, v, vn = r.astype(np.float64), v.astype(np.float64), vn.astype(np.float64)
    flat = lambda x: np.asarray(x, np.float32).reshape(T, -1)
    rho = np.exp(log_ratio(flat(behaviour_logp), flat(target_logp)).astype(np.float64))
    w = lambda x: np.float64(np.float32(x))
    g, lm = w(gamma), w(lam)
    rc, gc, rp = np.minimum(rho, w(rho_bar)), g * (lm * np.minimum(rho, w(c_bar))), np.minimum(rho, w(pg_rho_bar))
    u = 2.0 ** -24
    e = 2 * EXP_ULP * u
    acc, vs, pg, E, Evs, Epg = (np.empty_like(r) for _ in range(6))
    for t in range(T - 1, -1, -1):
        last = t + 1 == T
        nv = np.where(term[t], 0.0, np.where(cut[t], vn[t], 0.0 if last else v[t + 1]))
        nvs = np.where(term[t], 0.0, np.where(cut[t], vn[t], 0.0 if last else vs[t + 1]))
        c = np.where(cut[t], 0.0, 0.0 if last else acc[t + 1])
        e1 = np.where(cut[t], 0.0, 0.0 if last else E[t + 1])
        evs1 = np.where(cut[t], 0.0, 0.0 if last else Evs[t + 1])
        d = g * nv + r[t] - v[t]
        m = rc[t] * d
        acc[t] = m + gc[t] * c
        e_m = rc[t] * u * (np.abs(g * nv + r[t]) + np.abs(d)) + (e + u) * np.abs(m)
        E[t] = gc[t] * e1 + (e + 2 * u) * np.abs(gc[t] * c) + e_m + u * np.abs(acc[t])
        vs[t] = acc[t] + v[t]
        Evs[t] = E[t] + u * np.abs(vs[t])
        q = g * nvs + r[t] - v[t]
        pg[t] = rp[t] * q
        Epg[t] = rp[t] * (g * evs1 + u * (np.abs(g * nvs + r[t]) + np.abs(q))) + (e + u) * np.abs(pg[t])
    return vs, pg, Evs, Epg


def random_case(rng, T, N, p_trunc=0.12, p_term=0.06):
    """gae_ref.random_case plus the two log-density planes: log-ratios roughly N(0, 0.7); the columns n % 7 == 1 with the two planes
    equal (ratio exactly 0); and, outside those columns, the elements with (t N + n) % 53 == 5 at +25 and == 11 at -25 (beyond the clamp)"""
    case = gae_ref.random_case(rng, T, N, p_trunc, p_term)
    bl = rng.normal(-1.0, 0.5, (T, N)).astype(np.float32)
    tl = (bl + rng.normal(0, 0.7, (T, N)).astype(np.float32)).astype(np.float32)
    idx = np.arange(T)[:, None] * N + np.arange(N)[None, :]
    tl = np.where(idx % 53 == 5, bl + np.float32(25), np.where(idx % 53 == 11, bl - np.float32(25), tl)).astype(np.float32)
    tl[:, 1::7] = bl[:, 1::7]
    case.update(behaviour_logp=bl, target_logp=tl)
    return case


def features(case, thresholds=(1.0, 1.0, 1.0)):
    """which branches of the definition a case takes (tests/test_vtrace_cpu.py asserts them at the shapes the GPU tests use)"""
    bl, tl = case["behaviour_logp"], case["target_logp"]
    T = bl.shape[0]
    lr = fsub(tl, bl)
    rho = exp_def(log_ratio(bl, tl))
    tr, te = case["truncated"] != 0, case["terminated"] != 0
    combos = lambda row: sorted({(int(a), int(b)) for a, b in zip(tr[row], te[row])})
    return dict(below=[bool((rho < np.float32(b)).any()) for b in thresholds], above=[bool((rho > np.float32(b)).any()) for b in thresholds],
                clamp_low=bool((lr < -CLAMP).any()), clamp_high=bool((lr > CLAMP).any()),
                ratio_zero_columns=int((lr == 0).all(axis=0).sum()), rho_one=bool((rho[:, (lr == 0).all(axis=0)] == 1).all()),
                flags_first=combos(0), flags_last=combos(T - 1))
