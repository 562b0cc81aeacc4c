"""phx_policy_mlp restated in numpy, vectorised over rows, bit for bit (include/phantom_amd.h): the f32 fused multiply-add, the
PHX_ACT_TANH approximation step for step, and the network's action.  The oracle restates narrow ReLU / hard-tanh networks only; this
module is what the tests use for tanh and for hidden layers wider than 64.

  fmaf(a, b, c): the product of two f32 is exact in f64 (48 significant bits); TwoSum gives the exact residue of the f64 sum; the sum
  rounded to ODD (the inexact f64 result with its last bit forced to 1) then rounded once to f32 is the correctly rounded f32 result,
  because 53 >= 24 + 2.
  a / b (f32): the f64 quotient rounded to f32 is already the correctly rounded f32 quotient (53 >= 2 * 24 + 2); a * b likewise.
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


def fmaf(a, b, c):
    """the correctly rounded f32 fused multiply-add, elementwise (broadcasting)"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b                                                   # exact
    s = p + c
    bv = s - p
    e = (p - (s - bv)) + (c - bv)                                # TwoSum: p + c == s + e exactly
    odd = (s.view(np.uint64) & np.uint64(1)) == 1
    toward = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    s = np.where((e != 0) & ~odd, toward, s)                     # round to odd
    return s.astype(np.float32)


def fmul(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def fdiv(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) / np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def tanh_def(c):
    """PHX_ACT_TANH exactly as the header defines it"""
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
    t = np.where(t > np.float32(1), np.float32(1), t)
    t = np.where(a < TANH_SMALL, a, t)
    t = np.where(a < TANH_SAT, t, np.float32(1))
    return np.copysign(t, c).astype(np.float32)


def act(c, kind):
    kind = _ACT.get(kind, kind)
    c = np.asarray(c, np.float32)
    if kind == ACT_RELU:
        return np.where(c > 0, c, np.float32(0)).astype(np.float32)
    if kind == ACT_HARD_TANH:
        return np.where(c < -1, np.float32(-1), np.where(c > 1, np.float32(1), c)).astype(np.float32)
    if kind == ACT_TANH:
        return tanh_def(c)
    raise ValueError(f"activation {kind}")


def linear(w, b, h):
    """c[r, i] = b[i]; for k ascending: c = fmaf(w[i, k], h[r, k], c)"""
    w = np.asarray(w, np.float32); h = np.asarray(h, np.float32)
    c = np.broadcast_to(np.asarray(b, np.float32), (h.shape[0], w.shape[0])).copy()
    for k in range(w.shape[1]):
        c = fmaf(w[None, :, k], h[:, k:k + 1], c)
    return c


def action(pol, x):
    """the device's action for observations x [N, D] of an ``MLPPolicy`` (its host weights), f32 [N]"""
    h = np.asarray(x, np.float32).reshape(-1, pol.weights[0].shape[1])
    n = len(pol.weights)
    for l in range(n - 1):
        h = act(linear(pol.weights[l], pol.biases[l], h), pol.activation)
    y = linear(pol.weights[-1], pol.biases[-1], h)[:, 0]
    a = fmaf(np.float32(pol.out_scale), y, np.float32(pol.out_bias))
    lo, hi = np.float32(pol.out_lo), np.float32(pol.out_hi)
    a = np.where(a < lo, lo, np.where(a > hi, hi, a)).astype(np.float32)
    return (a + np.float32(0)).astype(np.float32)
