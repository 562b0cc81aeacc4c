"""Device policies of RLlib's default size without a GPU: the numpy restatement of phx_policy_mlp (tests/policy_ref.py) against libm's fmaf
and against the oracle's own restatement of narrow ReLU / hard-tanh networks; the PHX_ACT_TANH definition's required properties (odd, bounded,
within 4e-7 of tanh everywhere and 1e-6 relative on [2^-12, 1]); MLPPolicy's width and activation rules and MLPPolicy.from_torch."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phantom_amd as ph
import policy_ref as pr
from helpers import f32_bits, supply_chain_env
from oracle import OracleEnv


def _policy(widths, act, seed, scale=55.0, bias=40.0):
    rng = np.random.default_rng(seed)
    dims = [3] + list(widths) + [1]
    ws = [rng.normal(0, 1.2 / np.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0, 0.3, (dims[l + 1],)).astype(np.float32) for l in range(len(dims) - 1)]
    return ph.MLPPolicy(ws, bs, activation=act, out_scale=scale, out_bias=bias)


def _libm_fmaf():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = m.fmaf
    f.restype, f.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float]
    return f


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- fmaf ----------------------------------------------------------------------------------------------------------------------------------
def _adversarial(rng, n):
    f = lambda x: np.asarray(x, np.float32)
    m = f(1 + rng.integers(0, 1 << 23, n) * 2.0 ** -23)                 # random significands in [1, 2)
    e = rng.integers(-20, 20, n)
    cases = []
    # ties at f32 precision: c + a b exactly half an ulp of c away (and a hair off it, below f64's resolution of a naive double rounding)
    c = f(m * 2.0 ** e)
    half = f(2.0 ** (e - 24))
    cases.append((half, f(np.ones(n)), c))
    cases.append((half, f(1 + 2.0 ** -23 * rng.integers(1, 8, n)), c))
    cases.append((half, f(1 - 2.0 ** -24 * rng.integers(1, 8, n)), c))
    cases.append((f(-half), f(1 + 2.0 ** -23 * rng.integers(1, 8, n)), c))
    # cancellation: c = -fl(a b) (the result is the product's rounding error) and c = -fl(a b) +- one ulp
    a, b = f(rng.normal(0, 1, n)), f(rng.normal(0, 1, n))
    p = f(a.astype(np.float64) * b)
    cases.append((a, b, f(-p)))
    cases.append((a, b, f(np.nextafter(-p, np.float32(np.inf)))))
    cases.append((a, b, f(-p * 2.0)))
    # subnormal results: products and addends around 2^-126 .. 2^-149
    a = f(m * 2.0 ** rng.integers(-75, -60, n)); b = f(rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-75, -60, n))
    cases.append((a, b, f(rng.integers(-(1 << 23), 1 << 23, n).astype(np.int64) * 2.0 ** -149)))
    cases.append((a, b, f(np.zeros(n))))
    # signed zeros
    z = f(np.zeros(n))
    cases.append((z, f(rng.normal(0, 1, n)), f(-z)))
    cases.append((f(-z), f(np.abs(rng.normal(0, 1, n))), z))
    return [tuple(np.asarray(v, np.float32) for v in cs) for cs in cases]


def test_numpy_fmaf_matches_libm_bit_for_bit():
    fmaf = _libm_fmaf()
    rng = np.random.default_rng(12)
    n = 1_000_000
    e = lambda: (2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    a = (rng.normal(0, 1, n) * e()).astype(np.float32)
    b = (rng.normal(0, 1, n) * e()).astype(np.float32)
    c = (rng.normal(0, 1, n) * e()).astype(np.float32)
    trip = [(a, b, c)] + _adversarial(rng, 4000)
    for i, (x, y, z) in enumerate(trip):
        got = pr.fmaf(x, y, z)
        want = np.fromiter((fmaf(float(p), float(q), float(r)) for p, q, r in zip(x.tolist(), y.tolist(), z.tolist())), np.float32, len(x))
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, f"set {i}: {bad.size} mismatches, first {x[bad[0]]!r} {y[bad[0]]!r} {z[bad[0]]!r}: {got[bad[0]]!r} != {want[bad[0]]!r}"


# ---- the restatement against the oracle's policy path (narrow ReLU / hard-tanh: what the oracle knows) --------------------------------------
@pytest.mark.parametrize("widths,act", [((32,), "relu"), ((16, 8), "hard_tanh"), ((64, 64), "relu"), ((17, 33), "hard_tanh")])
def test_restatement_matches_the_oracle(widths, act):
    S, B, ns, T = 4, 24, 9, 25
    env = supply_chain_env(S, [3] * S, ns, B, seed=5)
    o = OracleEnv(env.spec, threads=2)
    first, _ = o.reset()
    pol = _policy(widths, act, 7)
    ro = o.rollout(T, policy=pol)
    prev = np.concatenate([first[None], ro["obs"][:-1]])
    for t in np.flatnonzero(ro["truncated"][:-1, 0, 0]):              # after an episode's end the policy sees the reset observation
        prev[t + 1, ..., 0] = 0.0
    want = pr.action(pol, prev.reshape(-1, 3)).reshape(ro["actions"].shape)
    np.testing.assert_array_equal(f32_bits(ro["actions"]), f32_bits(want))
    assert np.unique(ro["actions"]).size > 20


# ---- PHX_ACT_TANH ---------------------------------------------------------------------------------------------------------------------------
def _check_tanh(c):
    c = np.asarray(c, np.float32)
    t = pr.tanh_def(c)
    tn = pr.tanh_def(-c)
    np.testing.assert_array_equal(_bits(tn), _bits(-t), err_msg="odd")
    assert np.all(np.abs(t) <= 1.0)
    ref = np.tanh(c.astype(np.float64))
    err = np.abs(t.astype(np.float64) - ref)
    assert err.max() <= 4e-7, (err.max(), c[np.argmax(err)])
    m = (np.abs(c) >= 2.0 ** -12) & (np.abs(c) <= 1.0)
    if m.any():
        rel = err[m] / np.abs(ref[m])
        assert rel.max() <= 1e-6, (rel.max(), c[m][np.argmax(rel)])


def test_tanh_definition_dense_grid():
    lo, hi = int(_bits(np.float32(2.0 ** -13))), int(_bits(np.float32(10.0)))
    for start in range(lo, hi + 1, 1 << 22):                           # every 64th bit pattern, in chunks
        bits = np.arange(start, min(start + (1 << 22), hi + 1), 64, dtype=np.uint32)
        _check_tanh(bits.view(np.float32))


def test_tanh_definition_at_its_thresholds_and_everywhere():
    for th in (pr.TANH_SAT, pr.TANH_SMALL, np.float32(1.0), np.float32(2.0 ** -13)):
        b = int(_bits(th))
        _check_tanh(np.arange(b - 4096, b + 4097, dtype=np.uint32).view(np.float32))
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 0x7f800000, 1 << 20, dtype=np.uint32)      # every finite magnitude, subnormals and zero included
    _check_tanh(np.concatenate([bits, np.array([0, 1, 0x7f7fffff], np.uint32)]).view(np.float32))
    assert pr.tanh_def(np.float32(np.inf)) == 1.0 and pr.tanh_def(np.float32(-np.inf)) == -1.0
    z = pr.tanh_def(np.array([0.0, -0.0], np.float32))
    assert _bits(z).tolist() == [0, 0x80000000]                       # act(0) = +0: padded units contribute nothing


# ---- MLPPolicy ------------------------------------------------------------------------------------------------------------------------------
def _zeros(widths):
    dims = [3] + list(widths) + [1]
    return [np.zeros((dims[l + 1], dims[l]), np.float32) for l in range(len(dims) - 1)], [np.zeros(d, np.float32) for d in dims[1:]]


@pytest.mark.parametrize("widths", [(256, 256), (96,), (1,), (64, 64), (128, 32), (224, 96), (256,)])
def test_mlp_policy_accepts_the_width_rule(widths):
    for act in ("relu", "hard_tanh", "tanh"):
        p = ph.MLPPolicy(*_zeros(widths), activation=act)
        s = p.host_struct()
        assert [s.width[0], s.width[1]][:len(widths)] == list(widths) and s.n_hidden == len(widths)
        assert s.activation == {"relu": 0, "hard_tanh": 1, "tanh": 2}[act]


@pytest.mark.parametrize("widths", [(65,), (257,), (200,), (100, 64), (64, 288), (512,), (0,)])
def test_mlp_policy_refuses_other_widths(widths):
    with pytest.raises(ValueError):
        ph.MLPPolicy(*_zeros(widths))


def test_mlp_policy_activation_names_and_constants():
    from phantom_amd import _abi
    assert (_abi.ACT_TANH, _abi.POLICY_WIDE_MAX, _abi.POLICY_WIDE_STEP, _abi.VR_POLICY_MFMA, _abi.POLICY_MAX_WIDTH) == (2, 256, 32, 6, 64)
    from phantom_amd.spec import VARIANT_ROLLOUT
    assert VARIANT_ROLLOUT["policy_mfma"] == 6
    with pytest.raises(ValueError):
        ph.MLPPolicy(*_zeros((8,)), activation="sigmoid")


def test_mlp_policy_call_is_the_same_function():
    import torch
    pol = _policy((256, 256), "tanh", 4)
    x = np.random.default_rng(0).uniform(0, 1.5, (512, 3)).astype(np.float32)
    got = pol(torch.from_numpy(x)).numpy()
    np.testing.assert_allclose(got, pr.action(pol, x), rtol=1e-4, atol=1e-3)


# ---- from_torch ------------------------------------------------------------------------------------------------------------------------------
def test_from_torch_maps_the_activations():
    import torch
    nn = torch.nn
    torch.manual_seed(0)
    cases = [(nn.Sequential(nn.Linear(3, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, 1)), "tanh"),
             (nn.Sequential(nn.Linear(3, 32), nn.ReLU(), nn.Linear(32, 1)), "relu"),
             (nn.Sequential(nn.Linear(3, 16), nn.Hardtanh(), nn.Linear(16, 8), nn.Hardtanh(-1.0, 1.0), nn.Linear(8, 1)), "hard_tanh")]
    x = np.random.default_rng(1).uniform(0, 1, (64, 3)).astype(np.float32)
    for net, act in cases:
        p = ph.MLPPolicy.from_torch(net, out_scale=50.0, out_bias=50.0)
        assert p.activation == act and len(p.weights) == len(net) // 2 + 1
        with torch.no_grad():
            y = net(torch.from_numpy(x)).squeeze(-1)
        want = torch.clamp(y * 50.0 + 50.0, 0.0, 100.0).numpy()
        np.testing.assert_allclose(pr.action(p, x), want, rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(p(torch.from_numpy(x)).numpy(), want, rtol=1e-5, atol=1e-4)


def test_from_torch_takes_the_mean_row_of_an_action_head():
    import torch
    nn = torch.nn
    head = nn.Linear(256, 2)                                            # RLlib's Box head: (mean, log_std)
    mean = nn.Linear(256, 1)
    with torch.no_grad():
        mean.weight.copy_(head.weight[:1]); mean.bias.copy_(head.bias[:1])
    p = ph.MLPPolicy.from_torch(nn.Sequential(nn.Linear(3, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), mean))
    np.testing.assert_array_equal(p.weights[-1], head.weight[:1].detach().numpy())


@pytest.mark.parametrize("build", [
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.Sigmoid(), nn.Linear(8, 1)),                      # another layer
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.ReLU(), nn.Linear(8, 8), nn.Tanh(), nn.Linear(8, 1)),   # mixed activations
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.Linear(8, 1)),                                    # no activation between Linears
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.Hardtanh(0.0, 1.0), nn.Linear(8, 1)),              # Hardtanh with other bounds
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.Tanh(), nn.Linear(8, 1), nn.Tanh()),               # ends in an activation
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.ReLU(), nn.ReLU(), nn.Linear(8, 1)),               # two activations in a row
    lambda nn: nn.Sequential(nn.Linear(3, 8), nn.Tanh(), nn.Dropout(), nn.Linear(8, 1)),            # another layer
    lambda nn: nn.Linear(3, 1),                                                                     # no hidden layer
    lambda nn: nn.Sequential(nn.Linear(3, 65), nn.Tanh(), nn.Linear(65, 1)),                       # width rule
])
def test_from_torch_refuses(build):
    import torch
    with pytest.raises(ValueError):
        ph.MLPPolicy.from_torch(build(torch.nn))
