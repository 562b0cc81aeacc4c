"""Gaussian exploration of a device policy (phx_policy_explore, ABI 10 additive) on the GPU: both policy kernels against the oracle (which
replays the device's actions) and against the numpy restatement of the header's definition (tests/policy_explore_ref.py), bit for bit; zero
noise against the deterministic rollout; the clamp, the missing log-std row, actions past the bounds and torch's log-density; every refusal;
and PhantomEnv.sample / BatchedBaseEnv.sample with RLlib's columns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phantom_amd as ph
import policy_explore_ref as per
from device_runner import DeviceRunner
from helpers import f32_bits, supply_chain_env
from oracle import OracleEnv
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
STATE = ("shop.stock", "shop.sales", "shop.missed_sales", "shop.delivered_stock", "env.step", "env.tick")
VALU, MFMA = "phx_sc_rollout_policy_explore_kernel", "phx_sc_rollout_policy_mfma_explore_kernel"


def _policy(widths, act, seed, head=2, ls_bias=-0.5, log_std=None, scale=50.0, bias=50.0):
    """a random network with a (mean, log_std) head (head=2) or one row (+ log_std=)"""
    rng = np.random.default_rng(seed)
    dims = [3] + list(widths) + [head]
    ws = [rng.normal(0, 1.2 / np.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0, 0.3, (dims[l + 1],)).astype(np.float32) for l in range(len(dims) - 1)]
    if head == 2:
        ws[-1][1] *= 0.5
        bs[-1][1] = ls_bias
    return ph.MLPPolicy(ws, bs, activation=act, out_scale=scale, out_bias=bias, out_lo=0.0, out_hi=100.0, log_std=log_std)


def _explore(d, T, pol, noise, exo=None):
    """one exploring rollout of DeviceRunner d: (the planes as numpy, the trajectory)"""
    nz = torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to(d.dev.device)
    x = None if exo is None else torch.from_numpy(exo).to(d.dev.device)
    out = d.dev.alloc_trajectory(T, explore=True)
    d.dev.rollout(T, None, x, out=out, policy=pol, noise=nz)
    return {k: getattr(out, f).cpu().numpy() for k, f in (("obs", "observations"), ("actions", "actions"), ("rewards", "rewards"),
                                                            ("truncated", "truncations"), ("last_obs", "last_obs"), ("raw", "raw_actions"),
                                                            ("logp", "action_logp"), ("dist", "dist_inputs"))}


def _prev_obs(first, r):
    """the policy's input of every row: the previous row's observation, the reset observation after an episode's end"""
    prev = np.concatenate([first[None], r["obs"][:-1]])
    for t in np.flatnonzero(r["truncated"][:-1].reshape(r["truncated"].shape[0] - 1, -1)[:, 0]):
        prev[t + 1, ..., 0] = 0.0
    return prev


def _check_against_restatement(pol, first, r, noise):
    prev = _prev_obs(first, r)
    a, z, lp, di = per.explore(pol, prev.reshape(-1, 3), noise.reshape(-1))
    shp = r["actions"].shape
    np.testing.assert_array_equal(f32_bits(r["dist"]), f32_bits(di.reshape(shp + (2,))), err_msg="dist_inputs")
    np.testing.assert_array_equal(f32_bits(r["raw"]), f32_bits(z.reshape(shp)), err_msg="raw_action")
    np.testing.assert_array_equal(f32_bits(r["logp"]), f32_bits(lp.reshape(shp)), err_msg="logp")
    np.testing.assert_array_equal(f32_bits(r["actions"]), f32_bits(a.reshape(shp)), err_msg="action_out")


def _check_oracle_replay(o, d, r, exo):
    ro = o.rollout(r["actions"].shape[0], r["actions"], exo)
    for k, kd in (("obs", "obs"), ("rewards", "rewards"), ("last_obs", "last_obs")):
        np.testing.assert_array_equal(f32_bits(ro[k]), f32_bits(r[kd]), err_msg=k)
    np.testing.assert_array_equal(ro["truncated"], r["truncated"])
    for f in STATE:
        np.testing.assert_array_equal(d.get_i32(f), o.get_i32(f), err_msg=f)


# (widths, activation, variant, kernel): the VALU kernel's one- and two-layer (SGPR-weight) forms, the MFMA kernel's tanh / wide forms,
# and a narrow network on the MFMA kernel
NETS = [((8,), "relu", "auto", VALU), ((32,), "hard_tanh", "auto", VALU), ((64, 64), "relu", "auto", VALU),
        ((24, 16), "hard_tanh", "auto", VALU), ((256, 256), "tanh", "auto", MFMA), ((96,), "relu", "auto", MFMA),
        ((32, 32), "relu", "policy_mfma", MFMA)]
SHAPES = [(9, 61), (64, 5), (65, 3), (128, 2)]          # (S, B): every one leaves a partial last workgroup or one env per workgroup


@pytest.mark.parametrize("replayed", [False, True], ids=["device_orders", "replayed_orders"])
@pytest.mark.parametrize("S,B", SHAPES)
@pytest.mark.parametrize("widths,act,variant,kernel", NETS)
def test_exploring_rollout_is_the_definition(widths, act, variant, kernel, S, B, replayed):
    """(a) the oracle replaying the device's action plane reproduces every plane and the state; (b) dist_inputs, raw_action, logp and
    the actions are the restatement's on the previous observations and the noise, bit for bit -- across an episode end"""
    wide = max(widths) > 64
    if wide and S != 9:
        B = 1                                                        # (the restatement of a 256 x 256 layer is numpy work per row)
    ns, T = 5, 12
    env = supply_chain_env(S, [1 + s % 6 for s in range(S)], ns, B, seed=3 + S, env_offset=5, variants={"rollout": variant})
    o, d = OracleEnv(env.spec, threads=4), DeviceRunner(env.spec)
    o.reset(); d.reset()
    first = d.dev.obs.cpu().numpy()
    pol = _policy(widths, act, seed=S + len(widths))
    noise = np.random.default_rng(S).standard_normal((T, B, S)).astype(np.float32)
    exo = np.random.default_rng(S + 1).integers(0, 5, (T, B, d.n_exo)).astype(np.uint8) if replayed else None
    r = _explore(d, T, pol, noise, exo)
    assert d.dev.last_kernel() == kernel, d.dev.last_kernel()
    assert (d.err == 0).all() and r["truncated"].any()
    _check_oracle_replay(o, d, r, exo)
    _check_against_restatement(pol, first, r, noise)
    assert len(np.unique(r["raw"])) > r["raw"].size // 2


@pytest.mark.parametrize("widths,act,variant", [((32,), "relu", "auto"), ((64, 64), "hard_tanh", "auto"), ((256, 256), "tanh", "auto"),
                                                ((16,), "relu", "policy_mfma")])
def test_zero_noise_is_the_deterministic_rollout(widths, act, variant):
    """noise == 0: z = y, every plane and the state are the deterministic rollout's (the mean row), bit for bit"""
    S, B, ns, T = 9, 40, 6, 15
    spec = supply_chain_env(S, [6] * S, ns, B, seed=8, variants={"rollout": variant}).spec
    d0, d1 = DeviceRunner(spec), DeviceRunner(spec)
    d0.reset(); d1.reset()
    pol = _policy(widths, act, seed=1)
    rd = d0.rollout(T, policy=pol)
    r = _explore(d1, T, pol, np.zeros((T, B, S), np.float32))
    for k in ("obs", "actions", "rewards", "last_obs"):
        np.testing.assert_array_equal(f32_bits(r[k]), f32_bits(rd[k]), err_msg=k)
    np.testing.assert_array_equal(r["truncated"], rd["truncated"])
    for f in STATE:
        np.testing.assert_array_equal(d0.get_i32(f), d1.get_i32(f), err_msg=f)
    np.testing.assert_array_equal(f32_bits(r["raw"]), f32_bits(r["dist"][..., 0] + np.float32(0)))


@pytest.mark.parametrize("variant", ["auto", "policy_mfma"])
def test_edges(variant):
    """the log-std clamped at +-20 (b = +-30), no log-std row (free log_std), noise that drives the action past out_lo / out_hi, and
    logp against torch.distributions.Normal"""
    S, B, ns, T = 9, 16, 6, 10
    spec = supply_chain_env(S, [6] * S, ns, B, seed=2, variants={"rollout": variant}).spec
    rng = np.random.default_rng(4)
    cases = [("clamp_hi", _policy((16,), "relu", 2, ls_bias=30.0), rng.standard_normal((T, B, S)) * 1e-8),
             ("clamp_lo", _policy((16,), "relu", 2, ls_bias=-30.0), rng.standard_normal((T, B, S))),
             ("free_log_std", _policy((16, 8), "relu", 3, head=1, log_std=-1.25), rng.standard_normal((T, B, S))),
             ("free_clamped", _policy((16,), "hard_tanh", 3, head=1, log_std=25.0), rng.standard_normal((T, B, S)) * 1e-9),
             ("past_bounds", _policy((16,), "relu", 5, ls_bias=1.0), rng.standard_normal((T, B, S)) * 40.0)]
    for name, pol, noise in cases:
        noise = noise.astype(np.float32)
        d = DeviceRunner(spec); d.reset()
        first = d.dev.obs.cpu().numpy()
        r = _explore(d, T, pol, noise)
        assert d.dev.last_kernel() == (VALU if variant == "auto" else MFMA)
        _check_against_restatement(pol, first, r, noise)
        l = np.clip(r["dist"][..., 1], -20, 20)
        if name.startswith("clamp") or name == "free_clamped":
            assert (np.abs(r["dist"][..., 1]) > 20).all() and (np.abs(l) == 20).all(), name
        if name.startswith("free"):
            assert (r["dist"][..., 1] == np.float32(pol.log_std)).all()
        if name == "past_bounds":
            assert (r["actions"] == 0).any() and (r["actions"] == 100).any()
        if name in ("free_log_std", "past_bounds"):          # torch's density of z (where std is not far below the ulp of z)
            mean, ls = torch.from_numpy(r["dist"][..., 0]).double(), torch.from_numpy(l).double()
            want = torch.distributions.Normal(mean, ls.exp()).log_prob(torch.from_numpy(r["raw"]).double()).numpy()
            np.testing.assert_allclose(r["logp"], want, rtol=2e-6, atol=2e-6)


def _io(d, T, pol_keep, out, explore=None):
    io = _abi.PhxRolloutIO()
    io.T = T
    io.obs, io.action_out, io.reward = out.observations.data_ptr(), out.actions.data_ptr(), out.rewards.data_ptr()
    io.terminated, io.truncated, io.last_obs = out.terminations.data_ptr(), out.truncations.data_ptr(), out.last_obs.data_ptr()
    io.err = d.dev.err.data_ptr()
    io.policy = None if pol_keep is None else C.addressof(pol_keep[2])
    io.reserved_ptr = None if explore is None else C.addressof(explore)
    return io


def test_refusals_leave_state_and_err_untouched():
    S, B, T = 9, 8, 4
    spec = supply_chain_env(S, [6] * S, 10, B, seed=2).spec
    d = DeviceRunner(spec); d.reset()
    pol = _policy((8,), "relu", 1)
    keep = pol.on(d.dev.device)
    out = d.dev.alloc_trajectory(T, explore=True)
    nz = torch.zeros((T, B, S), dtype=torch.float32, device=d.dev.device)
    good = lambda: pol.explore_struct(d.dev.device, nz, out.raw_actions, out.action_logp, out.dist_inputs)
    lib, h = d.dev.lib, d.dev.handle
    d.dev.err.fill_(7)
    state0 = {f: d.get_i32(f) for f in STATE}
    bad = []
    bad.append(("explore without policy", _io(d, T, None, out, good())))
    for field in ("noise", "b_log_std", "raw_action", "logp", "dist_inputs"):
        x = good(); setattr(x, field, None); bad.append((f"{field} NULL", _io(d, T, keep, out, x)))
        x = good(); setattr(x, field, getattr(x, field) + 2); bad.append((f"{field} misaligned", _io(d, T, keep, out, x)))
    x = good(); x.w_log_std = x.w_log_std + 1; bad.append(("w_log_std misaligned", _io(d, T, keep, out, x)))
    io = _io(d, T, keep, out, good()); io.actions = out.actions.data_ptr(); bad.append(("with replayed actions", io))
    for what, io in bad:
        assert lib.phx_rollout(h, C.byref(io), None) == -1, what                  # PHX_EINVAL
    fsm = DeviceRunner(supply_chain_env(3, [2] * 3, 10, 4, fsm=True).spec); fsm.reset()
    fo = fsm.dev.alloc_trajectory(T, explore=True)
    fz = torch.zeros((T, 4, 3), dtype=torch.float32, device=d.dev.device)
    fk = pol.on(fsm.dev.device)
    io = _io(fsm, T, fk, fo, pol.explore_struct(fsm.dev.device, fz, fo.raw_actions, fo.action_logp, fo.dist_inputs))
    io.obs_valid, io.reward_valid = fo.obs_valid.data_ptr(), fo.reward_valid.data_ptr()
    assert lib.phx_rollout(fsm.dev.handle, C.byref(io), None) == -2                 # PHX_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (d.dev.err.cpu().numpy() == 7).all()
    for f in STATE:
        np.testing.assert_array_equal(d.get_i32(f), state0[f], err_msg=f)
    with pytest.raises(ValueError):
        d.dev.rollout(T, out=out, policy=_policy((8,), "relu", 1, head=1), noise=nz)   # noise with a deterministic policy
    x = good()
    assert lib.phx_rollout(h, C.byref(_io(d, T, keep, out, x)), None) == 0
    assert d.dev.last_kernel() == VALU


def test_sample_gives_rllibs_columns():
    """PhantomEnv.sample(explore=True) across an episode boundary: RLlib's columns, consistent with pol.distribution(obs); the same
    generator seed reproduces the batch; BatchedBaseEnv.sample passes everything through"""
    S, B, ns, T = 9, 12, 7, 16
    pol = _policy((32,), "relu", 9)

    def make():
        env = supply_chain_env(S, [6] * S, ns, B, seed=11, exogenous="device")
        env.reset()
        return env

    env = make()
    g = torch.Generator(device="cuda").manual_seed(123)
    fb = env.sample(T, policy=pol, explore=True, generator=g)
    assert env._device().last_kernel() == VALU
    sb = fb.to_sample_batches()["default_policy"]
    for c in ("actions", "action_logp", "action_prob", "action_dist_inputs", "obs"):
        assert c in sb, c
    n = B * S * T
    assert sb["actions"].shape == (n, 1) and sb["action_dist_inputs"].shape == (n, 2) and (sb["t"] == 0).any()
    np.testing.assert_allclose(sb["action_prob"], np.exp(sb["action_logp"]), rtol=1e-6)
    mean, ls = pol.distribution(torch.from_numpy(sb["obs"]).cuda())
    np.testing.assert_allclose(sb["action_dist_inputs"][:, 0], mean.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sb["action_dist_inputs"][:, 1], ls.cpu().numpy(), rtol=1e-5, atol=1e-5)
    want = torch.distributions.Normal(mean.double(), ls.double().clamp(-20, 20).exp()).log_prob(
        torch.from_numpy(sb["actions"][:, 0]).cuda().double())
    np.testing.assert_allclose(sb["action_logp"], want.cpu().numpy(), rtol=2e-5, atol=1e-5)
    env_act = np.clip(np.float32(pol.out_scale) * fb.raw_actions + np.float32(pol.out_bias), 0, 100)
    np.testing.assert_allclose(fb.actions, env_act, rtol=1e-6, atol=1e-4)              # rollouts() / step() show the env's actions
    st = fb.step(0, 0)
    assert st.actions[fb.agent_ids[0]][0] == fb.actions[0, 0, 0]
    g2 = torch.Generator(device="cuda").manual_seed(123)
    fb2 = make().sample(T, policy=pol, explore=True, generator=g2)
    for k in ("actions", "raw_actions", "action_logp", "dist_inputs", "obs"):
        np.testing.assert_array_equal(f32_bits(getattr(fb, k)), f32_bits(getattr(fb2, k)), err_msg=k)
    fb3 = make().sample(T, policy=pol, explore=True)                                  # the env's own generator: reproducible too
    fb4 = make().sample(T, policy=pol, explore=True)
    np.testing.assert_array_equal(f32_bits(fb3.raw_actions), f32_bits(fb4.raw_actions))
    fd = make().sample(T, policy=pol)                                                  # deterministic on-policy sampling
    assert fd.raw_actions is None and "action_logp" not in fd.to_sample_batches()["default_policy"]
    be = ph.rllib.BatchedBaseEnv(make())
    g3 = torch.Generator(device="cuda").manual_seed(123)
    sb2 = be.sample(T, policy=pol, explore=True, generator=g3)["default_policy"]
    for c in ("actions", "action_logp", "action_prob", "action_dist_inputs"):
        np.testing.assert_array_equal(sb2[c], sb[c], err_msg=c)
