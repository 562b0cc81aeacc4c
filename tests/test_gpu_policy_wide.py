"""Device policies of RLlib's default size on the GPU (phx_sc_rollout_policy_mfma_kernel: tanh, hidden layers up to 256 units, f32 MFMA).

Every case goes through the oracle end to end (its own on-policy rollout: the rows, last_obs and the state bit for bit).  The decomposed
test also checks two halves, which localise a failure: (a) the oracle, replaying the device's action plane through io.actions from the
same start state, reproduces every other plane and the state bit for bit -- the env semantics; (b) every action (or a seeded sample at the
bench shape, which is not run end to end: the oracle evaluates 256 x 256 with libm's fmaf) equals tests/policy_ref.py's restatement of
phx_policy_mlp on the previous observation bit for bit -- the network.  Narrow shapes also run on the new kernel (variant_rollout =
"policy_mfma") against the default kernel; the shape tests reach the kernel's 128-row workgroups, its second weight slot, its 4-byte weight
loads and both ends of a workgroup's env count."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phantom_amd as ph
import policy_ref as pr
from device_runner import DeviceRunner
from helpers import f32_bits, market_env, supply_chain_env
from oracle import OracleEnv

pytestmark = pytest.mark.gpu
NCPU = min(os.cpu_count() or 1, 128)
STATE = ("shop.stock", "shop.sales", "shop.missed_sales", "shop.delivered_stock", "env.step", "env.tick")
MFMA = "phx_sc_rollout_policy_mfma_kernel"
VALU = "phx_sc_rollout_policy_kernel"


def _policy(widths, act, seed, scale=60.0):
    """a random network whose action at the zero observation is 50 (so that actions neither stick at 0 nor at 100)"""
    rng = np.random.default_rng(seed)
    dims = [3] + list(widths) + [1]
    ws = [rng.normal(0, 1.5 / np.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0, 0.3, (dims[l + 1],)).astype(np.float32) for l in range(len(dims) - 1)]
    f = {"relu": lambda c: np.maximum(c, 0), "hard_tanh": lambda c: np.clip(c, -1, 1), "tanh": np.tanh}[act]
    h = np.zeros(3)
    for l in range(len(ws) - 1):
        h = f(ws[l].astype(np.float64) @ h + bs[l])
    y0 = float((ws[-1].astype(np.float64) @ h + bs[-1])[0])
    return ph.MLPPolicy(ws, bs, activation=act, out_scale=scale, out_bias=50.0 - scale * y0, out_lo=0.0, out_hi=100.0)


def _cmp(rd, ro, what, actions=True):
    for k in ("obs", "rewards") + (("actions",) if actions else ()):
        np.testing.assert_array_equal(f32_bits(rd[k]), f32_bits(ro[k]), err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(rd["truncated"], ro["truncated"], err_msg=what)
    np.testing.assert_array_equal(rd["terminated"], ro["terminated"], err_msg=what)
    np.testing.assert_array_equal(f32_bits(rd["last_obs"]), f32_bits(ro["last_obs"]), err_msg=what)


def _cmp_state(d, o, what):
    for f in STATE:
        np.testing.assert_array_equal(d.get_i32(f), o.get_i32(f), err_msg=f"{f}: {what}")


def _prev_obs(x0, rd):
    """the policy's input at every step: the fragment's start observation, then the previous row's -- the reset observation (stock 0,
    the sales and missed sales of the last step) after an episode's last row"""
    prev = np.concatenate([x0[None], rd["obs"][:-1]]).copy()
    ends = rd["truncated"][:-1].astype(bool)
    prev[1:][ends, 0] = 0.0
    return prev


def _check_actions(pol, prev, acts, idx=None):
    """(b): the device's actions == the restatement on the previous observation, bit for bit (at flat indices idx, or everywhere);
    the restatement runs once per distinct observation"""
    x = prev.reshape(-1, 3); a = acts.reshape(-1)
    if idx is not None:
        x, a = x[idx], a[idx]
    u, inv = np.unique(x, axis=0, return_inverse=True)
    want = pr.action(pol, u)[inv.reshape(-1)]
    bad = np.flatnonzero(f32_bits(want) != f32_bits(a))
    assert bad.size == 0, f"{bad.size} actions differ; first: obs {x[bad[0]]} device {a[bad[0]]!r} restatement {want[bad[0]]!r}"


def _fragment(d, o, pol, T, x0, what, exo=None, idx=None, oe=None):
    rd = d.rollout(T, None, exo, policy=pol)
    assert d.dev.last_kernel() == MFMA, d.dev.last_kernel()
    assert (d.err == 0).all()
    ro = o.rollout(T, rd["actions"], exo)                              # (a) the env semantics, replaying the device's actions
    _cmp(rd, ro, what)
    _cmp_state(d, o, what)
    _check_actions(pol, _prev_obs(x0, rd), rd["actions"], idx)         # (b) the network
    if oe is not None:                                                 # (c) end to end: the oracle's own on-policy rollout
        _cmp(rd, oe.rollout(T, None, exo, policy=pol), f"{what}, end to end")
        _cmp_state(d, oe, f"{what}, end to end")
    return rd


@pytest.mark.parametrize("widths,act", [((256, 256), "tanh"), ((256,), "tanh"), ((96, 224), "relu"), ((128,), "hard_tanh"), ((64, 64), "tanh")])
@pytest.mark.parametrize("S,ks,B,ns", [(5, [3, 1, 6, 2, 4], 29, 7), (9, [6] * 9, 17, 11)])
def test_wide_and_tanh_policies_decomposed(widths, act, S, ks, B, ns):
    """(a) + (b) on every row, and (c) the oracle's own on-policy rollout end to end: S = 5 / 9 (workgroups of 12 / 7 envs, the last
    one partial), episodes ending inside the launch, two fragments in a row, then replayed order sizes"""
    env = supply_chain_env(S, ks, ns, B, seed=11 + S, env_offset=5)
    o, oe, d = OracleEnv(env.spec, threads=8), OracleEnv(env.spec, threads=8), DeviceRunner(env.spec)
    x0, _ = o.reset(); oe.reset(); d.reset()
    np.testing.assert_array_equal(f32_bits(d.dev.obs.cpu().numpy()), f32_bits(x0))
    pol = _policy(widths, act, seed=S + len(widths) + widths[0])
    rd = _fragment(d, o, pol, 2 * ns + 3, x0, "fragment 1", oe=oe)
    assert rd["truncated"].any() and np.unique(rd["actions"]).size > 10
    rd = _fragment(d, o, pol, 13, rd["last_obs"], "fragment 2", oe=oe)
    exo = np.random.default_rng(2).integers(0, 5, (12, B, d.n_exo)).astype(np.uint8)
    _fragment(d, o, pol, 12, rd["last_obs"], "replayed order sizes", exo=exo, oe=oe)


@pytest.mark.parametrize("widths,act", [((32,), "relu"), ((64, 64), "relu"), ((5,), "hard_tanh"), ((8, 3), "hard_tanh"), ((17, 33), "relu"),
                                        ((24, 8), "hard_tanh")])
@pytest.mark.parametrize("S,ks,B,ns", [(9, [6] * 9, 61, 23), (3, [2, 7, 1], 100, 11), (100, [2] * 100, 5, 9)])
def test_mfma_kernel_on_shapes_the_oracle_knows(widths, act, S, ks, B, ns):
    """variant_rollout = "policy_mfma": the oracle's rows end to end and the default kernel's rows, bit for bit (S = 100: 128-row
    workgroups)"""
    spec_v = supply_chain_env(S, ks, ns, B, seed=31 + S, env_offset=7, variants={"rollout": "policy_mfma"}).spec
    spec_d = supply_chain_env(S, ks, ns, B, seed=31 + S, env_offset=7).spec
    o, d, dd = OracleEnv(spec_v, threads=8), DeviceRunner(spec_v), DeviceRunner(spec_d)
    o.reset(); d.reset(); dd.reset()
    pol = _policy(widths, act, seed=S + len(widths))
    for rep, T in enumerate((2 * ns + 3, 17)):
        ro, rd = o.rollout(T, policy=pol), d.rollout(T, policy=pol)
        assert d.dev.last_kernel() == MFMA, d.dev.last_kernel()           # (phx_last_kernel: the process's last launch)
        r0 = dd.rollout(T, policy=pol)
        assert dd.dev.last_kernel() == VALU, dd.dev.last_kernel()
        _cmp(rd, ro, f"oracle rep {rep}")
        _cmp(rd, r0, f"default kernel rep {rep}")
        _cmp_state(d, o, f"rep {rep}")
    exo = np.random.default_rng(1).integers(0, 5, (12, B, d.n_exo)).astype(np.uint8)
    _cmp(d.rollout(12, None, exo, policy=pol), o.rollout(12, None, exo, policy=pol), "replayed order sizes")
    assert (d.err == 0).all()


def test_bench_shape_256_256_tanh():
    """SC64 (9 shops of 6 customers), B = 4096, T = 100, 3-256-256-1 tanh: (a) on every row; (b) on a seeded sample of 8192 (t, env, shop)
    triples (t = 0, the reset steps and t = T - 1 included) bit for bit and on every row against MLPPolicy.__call__ (torch) within 1e-4
    relative (of the action range near zero); then again after MLPPolicy.update()"""
    import torch
    S, K, B, T, ns = 9, 6, 4096, 100, 40
    env = supply_chain_env(S, [K] * S, ns, B, seed=42)
    o, d = OracleEnv(env.spec, threads=NCPU), DeviceRunner(env.spec)
    x0, _ = o.reset(); d.reset()
    pol = _policy((256, 256), "tanh", seed=0)
    rng = np.random.default_rng(9)
    n = T * B * S
    for rep in range(2):
        steps = np.concatenate([[0, ns, 2 * ns, T - 1], rng.integers(0, T, 8188)])
        idx = (steps * B * S + rng.integers(0, B * S, steps.size)).astype(np.int64)
        assert idx.max() < n
        rd = _fragment(d, o, pol, T, x0, f"bench shape, rep {rep}", idx=idx)
        prev = torch.from_numpy(_prev_obs(x0, rd)).to(d.dev.device)
        want = pol(prev).cpu().numpy()
        np.testing.assert_allclose(rd["actions"], want, rtol=1e-4, atol=1e-4 * 100.0)      # (1e-4 of the action range near 0)
        assert np.unique(rd["actions"]).size > 1000
        x0 = rd["last_obs"]
        g = np.random.default_rng(20 + rep)                            # a learner's update (a small step): the next fragment runs it
        pol.update([w + g.normal(0, 0.01, w.shape).astype(np.float32) for w in pol.weights],
                   [b + g.normal(0, 0.01, b.shape).astype(np.float32) for b in pol.biases])


def test_argument_errors_at_the_c_abi():
    from phantom_amd.device import DeviceError
    S, B = 9, 32
    d = DeviceRunner(supply_chain_env(S, [6] * S, 20, B, seed=3).spec); d.reset()
    pol = _policy((256, 256), "tanh", seed=5)
    d.dev.rollout(4, policy=pol)
    assert d.dev.last_kernel() == MFMA
    _, _, st = pol.on(d.dev.device)                                    # the argument block the library reads: broken on purpose below

    def refused(code):
        with pytest.raises(DeviceError, match=rf"\({code}\)"):
            d.dev.rollout(4, policy=pol)

    for w in (65, 200, 257, 0, 288):
        st.width[0] = w
        refused(-1)
    st.width[0] = 256
    st.activation = 3
    refused(-1)
    st.activation = ph.policy.ACTIVATIONS["tanh"]
    keep = st.w[1]
    st.w[1] = None
    refused(-1)
    st.w[1] = keep
    d.dev.rollout(4, policy=pol)                                       # (restored: served again)
    assert d.dev.last_kernel() == MFMA
    fsm = DeviceRunner(supply_chain_env(3, [2] * 3, 10, 8, fsm=True).spec); fsm.reset()
    with pytest.raises(DeviceError, match=r"\(-2\)"):
        fsm.dev.rollout(4, policy=_policy((256, 256), "tanh", 1))
    mk = DeviceRunner(market_env(4, 8, 2, 6, 4).spec); mk.reset()
    with pytest.raises((DeviceError, ValueError)):
        mk.dev.rollout(4, policy=_policy((128,), "tanh", 1))


def _end_to_end(S, ks, B, ns, pol, what, d=None, pol_dev=None):
    """two fragments in a row (episode ends inside) and one with replayed order sizes on the wide kernel == the oracle's on-policy rows,
    last_obs and state; `pol_dev`: what the device gets instead of `pol` (the same weights) -- returns the device's rows"""
    env = supply_chain_env(S, ks, ns, B, seed=7 + S, env_offset=3)
    o, d = OracleEnv(env.spec, threads=8), d or DeviceRunner(env.spec)
    o.reset(); d.reset()
    out = []
    for rep, T in enumerate((2 * ns + 3, ns + 2)):
        rd, ro = d.rollout(T, policy=pol_dev or pol), o.rollout(T, policy=pol)
        assert d.dev.last_kernel() == MFMA, d.dev.last_kernel()
        _cmp(rd, ro, f"{what}: fragment {rep}")
        _cmp_state(d, o, f"{what}: fragment {rep}")
        assert rd["truncated"].any() or rep == 1
        out.append(rd)
    exo = np.random.default_rng(4).integers(0, 5, (6, B, d.n_exo)).astype(np.uint8)
    rd = d.rollout(6, None, exo, policy=pol_dev or pol)
    assert d.dev.last_kernel() == MFMA
    _cmp(rd, o.rollout(6, None, exo, policy=pol), f"{what}: replayed order sizes")
    _cmp_state(d, o, f"{what}: replayed order sizes")
    assert (d.err == 0).all()
    return out + [rd]


@pytest.mark.parametrize("widths,act", [((256, 256), "tanh"), ((256,), "tanh"), ((224, 96), "relu"), ((96, 256), "hard_tanh")])
@pytest.mark.parametrize("S", [65, 100, 128])
def test_128_row_workgroups_end_to_end(S, widths, act):
    """S > 64: NR = 128 rows per workgroup (four 32-row tiles), one env per workgroup; with 256 units both weight slots of every wave"""
    _end_to_end(S, [1 + s % 6 for s in range(S)], 4, 5, _policy(widths, act, seed=S + widths[0]), f"S {S} {widths} {act}")


@pytest.mark.parametrize("S,B", [(1, 70), (33, 5), (64, 4), (9, 1), (9, 15)])
def test_workgroup_env_counts_end_to_end(S, B):
    """S = 1: 64 envs per workgroup (B = 70: the last holds 6); S = 33, 64: one env per workgroup; B = 1; S = 9, B = 15: the last workgroup
    of 7-env groups holds one env"""
    _end_to_end(S, [1 + s % 6 for s in range(S)], B, 6, _policy((256, 256), "tanh", seed=S + B), f"S {S} B {B}")


@pytest.mark.parametrize("widths,act", [((17, 256), "tanh"), ((63, 224), "relu"), ((256, 5), "tanh"), ((256, 1), "hard_tanh"),
                                        ((1, 256), "tanh"), ((96,), "relu")])
def test_odd_shapes_end_to_end(widths, act):
    """W0 % 4 != 0: the guarded 4-byte weight loads; (256, 5) / (256, 1): a wide first layer with one active weight slot and a zero-padded
    output row; (1, 256): Q = 8, the smallest the pipelined k loop takes; (96,): one wide hidden layer"""
    _end_to_end(9, [6] * 9, 15, 7, _policy(widths, act, seed=widths[0] + widths[-1]), f"{widths} {act}")


def test_misaligned_second_layer_end_to_end():
    """w[1] 4 bytes into a larger device tensor (4-byte but not 16-byte aligned: the guarded loads with a 256 x 256 layer): the same rows
    as the aligned tensor of the same weights and as the oracle"""
    import torch
    pol = _policy((256, 256), "tanh", seed=77)
    S, B = 9, 15
    env = supply_chain_env(S, [6] * S, 7, B, seed=7 + S, env_offset=3)
    d = DeviceRunner(env.spec)
    twin = ph.MLPPolicy(pol.weights, pol.biases, activation=pol.activation, out_scale=pol.out_scale, out_bias=pol.out_bias,
                        out_lo=pol.out_lo, out_hi=pol.out_hi)
    _, _, st = twin.on(d.dev.device)
    w1 = torch.from_numpy(pol.weights[1]).reshape(-1)
    big = torch.zeros(w1.numel() + 8, dtype=torch.float32, device=d.dev.device)
    big[1:1 + w1.numel()] = w1.to(d.dev.device)
    st.w[1] = big.data_ptr() + 4
    assert st.w[1] % 16 == 4
    mis = _end_to_end(S, [6] * S, B, 7, pol, "w[1] misaligned", d=d, pol_dev=twin)
    ali = _end_to_end(S, [6] * S, B, 7, pol, "aligned")
    for a, b in zip(mis, ali):
        _cmp(a, b, "misaligned against aligned")
    del big
