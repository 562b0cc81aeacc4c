"""phx_policy_mlp restated in numpy, vectorised over rows, bit for bit (include/phantom_amd.h): the f32 fused multiply-add, the
PHX_ACT_TANH approximation step for step, and the network's action -- a second restatement next to the oracle's (oracle/phx_oracle.c), in
numpy, vectorised, and with switches that change the definition.

  fmaf(a, b, c): the product of two f32 is exact in f64 (48 significant bits); TwoSum gives the exact residue of the f64 sum; the sum
  rounded to ODD (the inexact f64 result with its last bit forced to 1) then rounded once to f32 is the correctly rounded f32 result,
  because 53 >= 24 + 2.
  a / b (f32): the f64 quotient rounded to f32 is already the correctly rounded f32 quotient (53 >= 2 * 24 + 2); a * b likewise.

`perturb` (a set of names from PERTURBATIONS) changes the definition the way a kernel could silently differ from it; the edge-value tests
(tests/policy_edges.py) show that they would notice each change.
"""
import numpy as np

ACT_RELU, ACT_HARD_TANH, ACT_TANH = 0, 1, 2
_ACT = {"relu": ACT_RELU, "hard_tanh": ACT_HARD_TANH, "tanh": ACT_TANH}

# the header's PHX_TANH_* literals
TANH_SAT = np.float32(float.fromhex("0x1.f9f09ep+2"))
TANH_SMALL = np.float32(float.fromhex("0x1p-12"))
TANH_A = [np.float32(float.fromhex(h)) for h in ("0x1.40b3b8p-8", "0x1.4e1bdap-11", "0x1.f28694p-17", "0x1.b80082p-25", "-0x1.7a6ffep-34",
                                                  "0x1.c266fcp-43", "-0x1.3e4b80p-52")]      # A1, A3, .., A13
TANH_B = [np.float32(float.fromhex(h)) for h in ("0x1.40b3bap-8", "0x1.29540ap-9", "0x1.f12bacp-14", "0x1.41a7b0p-20")]   # B0, B2, B4, B6


PERTURBATIONS = (
    "flush_subnormal_inputs",    # every product's operands flushed to a zero of their sign when subnormal (an FTZ build / MODE.denorm off)
    "tanh_small_up", "tanh_small_down",   # PHX_TANH_SMALL one ulp higher / lower
    "tanh_sat_up", "tanh_sat_down",       # PHX_TANH_SAT one ulp higher / lower
    "tanh_no_clamp",             # the rational's "t > 1 ? 1 : t" left out
    "k_descending",              # every layer's sum over k in descending order
    "pair_rounded_once",         # c + w[k] h[k] + w[k+1] h[k+1] rounded once per k-pair (an accumulator that rounds two products together)
    "bias_last",                 # the sum starts at 0 and the bias is added after the last k
    "inf_as_max",                # every sum saturating at +-FLT_MAX instead of overflowing to +-inf
    "relu_neg_zero",             # ReLU(-0) = -0 and no closing "+ 0.0f" on the action
    "relu_as_hard_tanh",         # ReLU evaluated with hard-tanh's clip constants (med3(c, -1, 1))
    "hard_tanh_bound_ulp",       # hard-tanh clipping at +-(1 - 2^-24)
)
NONE = frozenset()
_SUBNORMAL_MAX = np.float32(2.0 ** -126)


def _check(perturb):
    perturb = frozenset(perturb or ())
    unknown = perturb - set(PERTURBATIONS)
    if unknown:
        raise ValueError(f"unknown perturbations {sorted(unknown)}")
    return perturb


def _ftz(x):
    x = np.asarray(x, np.float32)
    return np.where(np.abs(x) < _SUBNORMAL_MAX, np.copysign(np.float32(0), x), x).astype(np.float32)


def fmaf(a, b, c):
    """the correctly rounded f32 fused multiply-add, elementwise (broadcasting)"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):             # (an infinite operand: e is NaN, and s stays the infinity)
        p = a * b                                               # exact
        s = p + c
        bv = s - p
        e = (p - (s - bv)) + (c - bv)                            # TwoSum: p + c == s + e exactly
        odd = (s.view(np.uint64) & np.uint64(1)) == 1
        toward = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        s = np.where((e != 0) & ~odd & np.isfinite(s), toward, s)     # round to odd
        return s.astype(np.float32)


def fmul(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def fdiv(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) / np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def tanh_def(c, perturb=NONE):
    """PHX_ACT_TANH exactly as the header defines it"""
    perturb = _check(perturb)
    sat, small = TANH_SAT, TANH_SMALL
    if "tanh_sat_up" in perturb: sat = np.nextafter(sat, np.float32(np.inf))
    if "tanh_sat_down" in perturb: sat = np.nextafter(sat, np.float32(0))
    if "tanh_small_up" in perturb: small = np.nextafter(small, np.float32(np.inf))
    if "tanh_small_down" in perturb: small = np.nextafter(small, np.float32(0))
    c = np.asarray(c, np.float32)
    a = np.abs(c)
    with np.errstate(over="ignore", invalid="ignore"):
        s = fmul(a, a)
        p = np.full_like(a, TANH_A[6])
        for k in (5, 4, 3, 2, 1, 0):
            p = fmaf(p, s, TANH_A[k])
        q = np.full_like(a, TANH_B[3])
        for k in (2, 1, 0):
            q = fmaf(q, s, TANH_B[k])
        t = fdiv(fmul(a, p), q)
    if "tanh_no_clamp" not in perturb:
        t = np.where(t > np.float32(1), np.float32(1), t)
    t = np.where(a < small, a, t)
    t = np.where(a < sat, t, np.float32(1))
    return np.copysign(t, c).astype(np.float32)


def act(c, kind, perturb=NONE):
    perturb = _check(perturb)
    kind = _ACT.get(kind, kind)
    c = np.asarray(c, np.float32)
    if kind == ACT_RELU and "relu_as_hard_tanh" in perturb:
        kind = ACT_HARD_TANH
    if kind == ACT_RELU:
        zero = np.where(c == 0, c, np.float32(0)) if "relu_neg_zero" in perturb else np.float32(0)
        return np.where(c > 0, c, zero).astype(np.float32)
    if kind == ACT_HARD_TANH:
        one = np.float32(1) if "hard_tanh_bound_ulp" not in perturb else np.nextafter(np.float32(1), np.float32(0))
        return np.where(c < -one, -one, np.where(c > one, one, c)).astype(np.float32)
    if kind == ACT_TANH:
        return tanh_def(c, perturb)
    raise ValueError(f"activation {kind}")


def linear(w, b, h, perturb=NONE):
    """c[r, i] = b[i]; for k ascending: c = fmaf(w[i, k], h[r, k], c)"""
    perturb = _check(perturb)
    w = np.asarray(w, np.float32); h = np.asarray(h, np.float32)
    if "flush_subnormal_inputs" in perturb:
        w, h = _ftz(w), _ftz(h)
    b = np.broadcast_to(np.asarray(b, np.float32), (h.shape[0], w.shape[0]))
    c = np.zeros_like(b) if "bias_last" in perturb else b.copy()
    ks = list(range(w.shape[1]))
    if "k_descending" in perturb:
        ks.reverse()
    if "pair_rounded_once" in perturb:
        with np.errstate(over="ignore", invalid="ignore"):
            for j in range(0, len(ks) - 1, 2):
                k0, k1 = ks[j], ks[j + 1]
                s = (c.astype(np.float64) + w[None, :, k0].astype(np.float64) * h[:, k0:k0 + 1]) + w[None, :, k1].astype(np.float64) * h[:, k1:k1 + 1]
                c = s.astype(np.float32)
        if len(ks) % 2:
            c = fmaf(w[None, :, ks[-1]], h[:, ks[-1]:ks[-1] + 1], c)
    else:
        for k in ks:
            c = fmaf(w[None, :, k], h[:, k:k + 1], c)
    if "bias_last" in perturb:
        with np.errstate(over="ignore", invalid="ignore"):
            c = (c + b).astype(np.float32)
    if "inf_as_max" in perturb:
        big = np.finfo(np.float32).max
        c = np.clip(c, -big, big).astype(np.float32)
    return c


def action(pol, x, perturb=NONE):
    """the device's action for observations x [N, D] of an ``MLPPolicy`` (its host weights), f32 [N]; `perturb`: a changed definition"""
    perturb = _check(perturb)
    h = np.asarray(x, np.float32).reshape(-1, pol.weights[0].shape[1])
    n = len(pol.weights)
    for l in range(n - 1):
        h = act(linear(pol.weights[l], pol.biases[l], h, perturb), pol.activation, perturb)
    y = linear(pol.weights[-1], pol.biases[-1], h, perturb)[:, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        a = fmaf(np.float32(pol.out_scale), y, np.float32(pol.out_bias))
    lo, hi = np.float32(pol.out_lo), np.float32(pol.out_hi)
    a = np.where(a < lo, lo, np.where(a > hi, hi, a)).astype(np.float32)
    if "relu_neg_zero" in perturb:
        return a
    return (a + np.float32(0)).astype(np.float32)
