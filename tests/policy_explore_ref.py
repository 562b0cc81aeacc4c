"""phx_policy_explore restated in numpy, vectorised over rows, bit for bit (include/phantom_amd.h, "Gaussian exploration"): the
clamped log-std, PHX_EXP's exp step for step, the draw, the action and the log-density -- every operation the correctly rounded f32 one,
through policy_ref's exact fmaf."""
import numpy as np

from policy_ref import act, fmaf, fmul, linear

LOG_STD_MIN, LOG_STD_MAX = np.float32(-20.0), np.float32(20.0)
EXP_LOG2E = np.float32(float.fromhex("0x1.715476p+0"))
EXP_LN2_HI = np.float32(float.fromhex("0x1.62e430p-1"))
EXP_LN2_LO = np.float32(float.fromhex("-0x1.05c610p-29"))
EXP_C = [np.float32(float.fromhex(h)) for h in ("0x1p+0", "0x1p+0", "0x1p-1", "0x1.555556p-3", "0x1.555556p-5", "0x1.111112p-7",
                                                 "0x1.6c16c2p-10", "0x1.a01a02p-13")]      # C0 .. C7: 1 / k! rounded to f32
HALF_LN_2PI = np.float32(float.fromhex("0x1.d67f1cp-1"))


def fsub(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def clamp_log_std(ls):
    ls = np.asarray(ls, np.float32)
    return np.where(ls < LOG_STD_MIN, LOG_STD_MIN, np.where(ls > LOG_STD_MAX, LOG_STD_MAX, ls)).astype(np.float32)


def exp_def(l):
    """std = exp(l) for a clamped log-std l (|l| <= 20) as the header defines it"""
    l = np.asarray(l, np.float32)
    n = np.rint(fmul(l, EXP_LOG2E)).astype(np.float32)              # (np.rint: half to even)
    r = fmaf(-n, EXP_LN2_HI, l)
    r = fmaf(-n, EXP_LN2_LO, r)
    p = np.full_like(r, EXP_C[7])
    for k in range(6, -1, -1):
        p = fmaf(p, r, EXP_C[k])
    return np.ldexp(p, n.astype(np.int32)).astype(np.float32)        # exact: |n| <= 29, the result is normal


def logp_def(noise, l):
    """log N(z; mean, exp(l)) through the noise: fmaf(-0.5, noise * noise, (-l) - PHX_HALF_LN_2PI)"""
    q = fmul(noise, noise)
    c = fsub(-np.asarray(l, np.float32), HALF_LN_2PI)
    return fmaf(np.float32(-0.5), q, c)


def heads(pol, x):
    """(y, ls): the network's mean output and its log-std output for observations x [N, D], f32 [N] each, unclamped and with the
    sign of an exact zero normalised (+ 0.0f) as the header's exploring definition takes them"""
    h = np.asarray(x, np.float32).reshape(-1, pol.weights[0].shape[1])
    for l in range(len(pol.weights) - 1):
        h = act(linear(pol.weights[l], pol.biases[l], h), pol.activation)
    out = linear(pol.weights[-1], pol.biases[-1], h)
    y = out[:, 0]
    if pol.weights[-1].shape[0] == 2:
        ls = out[:, 1]
    else:
        ls = np.full(y.shape, np.float32(pol.log_std), np.float32)
    return (y + np.float32(0)).astype(np.float32), (ls + np.float32(0)).astype(np.float32)


def explore(pol, x, noise):
    """the exploring policy's planes for observations x [N, D] and standard-normal draws noise [N]:
    (action, raw_action z, logp, dist_inputs [N, 2])"""
    y, ls = heads(pol, x)
    noise = np.asarray(noise, np.float32).reshape(-1)
    l = clamp_log_std(ls)
    std = exp_def(l)
    z = fmaf(std, noise, y)
    with np.errstate(over="ignore", invalid="ignore"):
        a = fmaf(np.float32(pol.out_scale), z, np.float32(pol.out_bias))
    lo, hi = np.float32(pol.out_lo), np.float32(pol.out_hi)
    a = (np.where(a < lo, lo, np.where(a > hi, hi, a)) + np.float32(0)).astype(np.float32)
    return a, z, logp_def(noise, l), np.stack([y, ls], axis=-1)
