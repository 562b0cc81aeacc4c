"""Hand-built phx_policy_mlp networks that drive the definition (include/phantom_amd.h) to the values where a kernel's arithmetic can
differ from it: the tanh thresholds, the ReLU / hard-tanh boundaries (where the kernels use v_med3_f32), signed zeros,
subnormal operands of the products, +inf pre-activations and sums whose value depends on the order of their roundings.

A FAMILY is a list of networks; each is paired with the perturbations of tests/policy_ref.py it targets.  `sensitive()` tells whether a
perturbed definition changes at least one action over a set of observations: a family that cannot tell the definition from its targets is
not a test.

Construction (observations are >= 0 and bounded; a unit whose weights are all 0 has its bias as pre-activation, exactly):
  * a VALUE network puts one pre-activation v on hidden unit j of the last hidden layer -- with one hidden layer as the bias of unit j;
    with two as w1[j][0] * h0[0] where h0[0] = act(ONE) = 1 (the MFMA kernel's A operand is v, its B operand 1) -- and reads it out as
    2^g h with a power of two g (split between the output weight and out_scale, so every product is exact): the action is |act(v)| 2^g
    bit for bit, and a one-ulp change of act(v) is a one-ulp change of the action.
  * NaN pre-activations (inf - inf, 0 * inf) are out of scope: the header defines the action for finite weights whose sums produce no NaN,
    and how the env decodes a NaN action is a separate question.  The overflow family keeps every weight that meets an inf non-zero and of
    one sign.
"""
import numpy as np

import phantom_amd as ph
import policy_ref as pr

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
TINY = F(2.0 ** -149)                                                  # the smallest subnormal: one ulp either side of 0
ONE = {"tanh": 8.0, "relu": 1.0, "hard_tanh": 1.0}                     # act(ONE) == 1 (tanh: ONE > PHX_TANH_SAT)


def _up(x):
    return np.nextafter(F(x), F(np.inf))


def _down(x):
    return np.nextafter(F(x), F(-np.inf))


def _around(x):
    return [F(x), _down(x), _up(x), F(-x), _down(-x), _up(-x)]


def _policy(act, ws, bs, out_scale=1.0, out_bias=-0.0, out_lo=0.0, out_hi=100.0):
    return ph.MLPPolicy([np.asarray(w, F) for w in ws], [np.asarray(b, F) for b in bs], activation=act, out_scale=out_scale,
                        out_bias=out_bias, out_lo=out_lo, out_hi=out_hi)


def _zeros(widths):
    dims = [3] + list(widths) + [1]
    return [np.zeros((dims[l + 1], dims[l]), F) for l in range(len(dims) - 1)], [np.zeros(dims[l + 1], F) for l in range(len(dims) - 1)]


def value_net(act, widths, v, j):
    """act(v) on hidden unit j of the last hidden layer, read out as |act(v)| 2^g (the sign of an exact zero kept up to the closing +0)"""
    v = F(v)
    ws, bs = _zeros(widths)
    neg = bool(np.signbit(v)) and v != 0
    if len(widths) == 1:
        bs[0][j] = v
        if v == 0 and np.signbit(v):
            ws[0][j, :] = F(-0.0)                                        # -0 x (>= 0) = -0: the sum stays -0
    else:
        bs[0][0] = ONE[act]
        ws[1][j, 0] = v
        if v == 0 and np.signbit(v):
            ws[1][j, :] = F(-0.0); bs[1][j] = F(-0.0)
    mag = float(min(abs(float(v)), 1.0)) if v != 0 else 1.0
    g = 5 - int(np.floor(np.log2(mag)))                                # |act(v)| 2^g in [16, 64] for |v| <= 1 (tanh, hard-tanh: |act| <= 1)
    if act == "relu" and abs(float(v)) > 1:
        g = 5
    gw = min(g, 120)
    if v == 0:
        ws[-1][0, :] = v; bs[-1][0] = v                                # (+-0 x +0 = +-0: a -0 reaches y only if every term is -0)
    ws[-1][0, j] = F(2.0 ** gw)
    return _policy(act, ws, bs, out_scale=(-1.0 if neg else 1.0) * 2.0 ** (g - gw))


def subnormal_net(act, widths):
    """two hidden layers: layer 0 units 1.. have subnormal weights and biases (h0 subnormal, row-dependent), unit 0 is 1; layer 1 sums
    subnormal x normal (h0 subnormal) and subnormal x 1 (w1 subnormal) products -- the MFMA's A and B operands -- into subnormal
    pre-activations; the output weight 2^120 and out_scale 2^24 bring them into the action."""
    rng = np.random.default_rng(3)
    W0, W1 = widths
    ws, bs = _zeros(widths)
    bs[0][0] = ONE[act]
    n0 = min(W0 - 1, 8)
    ws[0][1:1 + n0] = (rng.integers(1, 1 << 12, (n0, 3)) * 2.0 ** -149).astype(F)       # 2^-149 .. 2^-137
    bs[0][1:1 + n0] = (rng.integers(1, 1 << 10, n0) * 2.0 ** -149).astype(F)
    n1 = min(W1, 8)
    ws[1][:n1, 0] = (rng.integers(1, 1 << 14, n1) * 2.0 ** -149).astype(F)               # A subnormal, B = 1
    ws[1][:n1, 1:1 + n0] = (2.0 ** rng.integers(0, 6, (n1, n0))).astype(F)              # A normal, B subnormal
    ws[-1][0, :n1] = F(2.0 ** 120)
    return _policy(act, ws, bs, out_scale=2.0 ** 24)


def rounding_order_net(act, widths):
    """sums whose value depends on the order and number of their roundings, 1 + 2^24 - 2^24 (with h = 1 on the units read): 0 from the
    bias in ascending k, 1 descending, with the bias last or with a k-pair rounded once.  Two hidden layers: layer 1 (the MFMA layer of
    the wide kernel), k = 0, 1 (one MFMA k-pair), 1, 2 (across two) and 2, 3; one hidden layer: the output layer"""
    ws, bs = _zeros(widths)
    big = F(2.0 ** 24)
    if len(widths) == 1:
        bs[0][:2] = ONE[act]
        ws[-1][0, :2] = [big, -big]
        bs[-1][0] = F(1.0)
        return _policy(act, ws, bs, out_scale=16.0, out_bias=20.0)
    bs[0][:4] = ONE[act]
    for j, (k0, k1) in enumerate(((0, 1), (1, 2), (2, 3))):
        ws[1][j, k0], ws[1][j, k1] = big, -big
        bs[1][j] = F(1.0)
    ws[-1][0, :3] = F([16.0, 8.0, 4.0])
    return _policy(act, ws, bs, out_bias=20.0)


def overflow_net(act, widths, sign=1.0, out_lo=0.0, out_hi=100.0):
    """all-positive weights FLT_MAX: layer 0 unit 0 (bias 0) is +inf on the rows whose observations sum above 1, unit 1 (bias FLT_MAX) on
    every row with a non-zero observation; ReLU passes inf on, tanh and hard-tanh give 1; every later weight is FLT_MAX (two hidden
    layers) and the output weights are sign x FLT_MAX, so y = sign x inf, clipped to out_hi / out_lo.  No product is 0 x inf and no
    sum meets infinities of both signs.  (out_scale 2^-123: a y that saturated at FLT_MAX instead would land inside the action range.)"""
    ws, bs = _zeros(widths)
    ws[0][:2, :] = FLT_MAX
    bs[0][1] = FLT_MAX
    if len(widths) == 2:
        ws[1][:, :] = FLT_MAX
    ws[-1][0, :] = F(sign) * FLT_MAX
    return _policy(act, ws, bs, out_scale=2.0 ** -123, out_bias=50.0, out_lo=out_lo, out_hi=out_hi)


def exact_zero_net(act, widths, bias_sign, scale_sign, out_lo=0.0, out_hi=100.0):
    """every weight and bias a zero of sign `bias_sign`, out_bias too: the action is a zero whose sign before the closing "+ 0.0f" depends
    on the sign of every zero on the way (out_scale of either sign); it leaves as +0"""
    ws, bs = _zeros(widths)
    z = F(-0.0) if bias_sign < 0 else F(0.0)
    ws = [np.full_like(w, z) for w in ws]
    bs = [np.full_like(b, z) for b in bs]
    return _policy(act, ws, bs, out_scale=scale_sign, out_bias=float(z), out_lo=out_lo, out_hi=out_hi)


def families(act, widths, j):
    """{family name: ([networks], {targeted perturbations})} for activation `act`, hidden `widths` and the edge unit j"""
    two = len(widths) == 2
    fam = {}
    val = lambda vs: [value_net(act, widths, v, j) for v in vs]
    if act == "tanh":
        fam["tanh_small"] = (val(_around(pr.TANH_SMALL)), {"tanh_small_up", "tanh_small_down"})
        fam["tanh_sat"] = (val(_around(pr.TANH_SAT)), {"tanh_sat_up", "tanh_sat_down"})
        fam["signed_zero"] = (val([F(0.0), F(-0.0)]), {"relu_neg_zero"})
    elif act == "relu":
        fam["relu_zero"] = (val([F(0.0), F(-0.0), TINY, -TINY]), {"relu_neg_zero", "relu_as_hard_tanh", "flush_subnormal_inputs"})
        fam["relu_one"] = (val(_around(1.0)), {"relu_as_hard_tanh"})
    else:
        fam["hard_tanh_one"] = (val(_around(1.0)), {"hard_tanh_bound_ulp"})
        fam["signed_zero"] = (val([F(0.0), F(-0.0), TINY, -TINY]), {"relu_neg_zero", "flush_subnormal_inputs"})
    if two:
        fam["subnormal"] = ([subnormal_net(act, widths)], {"flush_subnormal_inputs"})
    fam["rounding_order"] = ([rounding_order_net(act, widths)], {"k_descending", "bias_last", "pair_rounded_once"})
    fam["overflow"] = ([overflow_net(act, widths, s) for s in (1.0, -1.0)] + [overflow_net(act, widths, 1.0, 30.0, 30.0)],
                       {"inf_as_max"})
    fam["exact_zero"] = ([exact_zero_net(act, widths, bsg, ssg) for bsg in (1.0, -1.0) for ssg in (1.0, -1.0)]
                         + [exact_zero_net(act, widths, -1.0, 1.0, 0.0, 0.0)],
                         {"relu_neg_zero"})
    return fam




def sensitive(pol, x, perturb):
    """does the definition changed by `perturb` change at least one action over the observations x?"""
    a, b = pr.action(pol, x), pr.action(pol, x, {perturb})
    return bool((a.view(np.uint32) != b.view(np.uint32)).any())


# (activation, hidden widths, edge unit j, kernel): the wide kernel's MFMA layer (j >= 128: the second weight slot) and VALU layer 0 / output
# layer; the narrow kernel's packed layer 0 and its three second-layer forms (SGPR 8 x 8, SGPR 4-unit, LDS)
MFMA = "phx_sc_rollout_policy_mfma_kernel"
VALU = "phx_sc_rollout_policy_kernel"
CONFIGS = [("tanh", (64, 256), 201, MFMA), ("tanh", (256,), 130, MFMA), ("relu", (64, 256), 201, MFMA), ("relu", (256,), 130, MFMA),
           ("hard_tanh", (64, 256), 201, MFMA), ("hard_tanh", (256,), 130, MFMA),
           ("relu", (24, 16), 13, VALU), ("relu", (16, 12), 5, VALU), ("relu", (5,), 3, VALU), ("hard_tanh", (24, 16), 13, VALU),
           ("hard_tanh", (5, 3), 2, VALU), ("hard_tanh", (5,), 3, VALU)]


def cases():
    """(test id, activation, widths, j, kernel, family name) for every family of every configuration"""
    out = []
    for act, widths, j, kern in CONFIGS:
        for name in families(act, widths, j):
            out.append((f"{act}-{'x'.join(map(str, widths))}-{name}", act, widths, j, kern, name))
    return out


def prev_obs(x0, ro):
    """the policy's input at every row of a rollout: the start observation, then the previous row's (the reset observation, stock 0,
    after an episode's last row), [T B S, 3]"""
    prev = np.concatenate([x0[None], ro["obs"][:-1]]).copy()
    prev[1:][ro["truncated"][:-1].astype(bool), 0] = 0.0
    return prev.reshape(-1, 3)
