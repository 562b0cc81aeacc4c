"""Gaussian exploration of a device policy without a GPU: the header's exp and log-density restated (tests/policy_explore_ref.py) against
float64, MLPPolicy's stochastic heads and refusals, FragmentBatch's RLlib columns, and the CPU library's refusal of an exploring io."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import phantom_amd as ph
import policy_explore_ref as per
import policy_ref as pr
from helpers import f32_bits, supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import FragmentBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp_err(got, x):
    want = np.exp(np.asarray(x, np.float64))
    return np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)


def test_exp_is_within_one_ulp_over_the_clamp_range():
    """pol_exp's restatement (exact fmaf) within 1 ulp of exp on a dense grid over [-20, 20] and its neighbours"""
    x = np.linspace(-20, 20, 2_000_001).astype(np.float32)
    x = np.unique(np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.float32([0.0, -0.0, 20.0, -20.0])]))
    err = _ulp_err(per.exp_def(x), x)
    assert err.max() < 1.0, (err.max(), x[err.argmax()])
    assert per.exp_def(np.float32([0.0]))[0] == 1.0
    # the reduction: |n| <= 29, so ldexp is exact and the result normal
    n = np.rint(pr.fmul(np.float32([-20, 20]), per.EXP_LOG2E))
    assert np.abs(n).max() <= 29


def test_every_f32_near_the_reduction_boundaries():
    """every f32 within 64 ulp of the half-integer multiples of ln 2 (where rint switches n) stays within 1 ulp"""
    pts = (np.arange(-29, 30) + 0.5) * np.log(2.0)
    pts = pts[np.abs(pts) <= 20].astype(np.float32)
    bits = pts.view(np.int32)[:, None] + np.arange(-64, 65, dtype=np.int32)[None, :]
    x = bits.reshape(-1).view(np.float32)
    assert _ulp_err(per.exp_def(x), x).max() < 1.0


def test_clamp_holds_beyond_the_range():
    ls = np.float32([-1e30, -30, -20.000002, -20, 0, 20, 20.000002, 30, 1e30, np.inf, -np.inf])
    l = per.clamp_log_std(ls)
    assert (l >= -20).all() and (l <= 20).all()
    np.testing.assert_array_equal(l[[3, 4, 5]], ls[[3, 4, 5]])
    assert np.isfinite(per.exp_def(l)).all()
    np.testing.assert_array_equal(per.exp_def(l[:2]), per.exp_def(np.float32([-20, -20])))


def test_logp_is_the_gaussian_density():
    """logp through the noise against the float64 log-density of z = mean + std noise (z exact in float64)"""
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(200_000).astype(np.float32)
    l = rng.uniform(-20, 20, noise.size).astype(np.float32)
    got = per.logp_def(noise, l).astype(np.float64)
    n64, l64 = noise.astype(np.float64), l.astype(np.float64)
    want = -0.5 * n64 * n64 - l64 - 0.5 * np.log(2 * np.pi)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=4e-6)
    # the same through the draw itself, where std is not small against ulp(z)
    mean = rng.normal(0, 1, noise.size)
    std = np.exp(np.clip(l64, -2, 2))
    z = mean + std * n64
    dens = -0.5 * ((z - mean) / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)
    np.testing.assert_allclose(per.logp_def(noise, np.clip(l, -2, 2)), dens, rtol=2e-6, atol=4e-6)


def _net(head=2, log_std=None, widths=(8,), seed=0):
    rng = np.random.default_rng(seed)
    dims = [3] + list(widths) + [head]
    ws = [rng.normal(0, 0.7, (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0, 0.3, (dims[l + 1],)).astype(np.float32) for l in range(len(dims) - 1)]
    return ws, bs, ph.MLPPolicy(ws, bs, out_scale=50.0, out_bias=50.0, log_std=log_std)


def test_mlp_policy_heads_and_refusals():
    ws, bs, p2 = _net(head=2)
    assert p2.stochastic
    _, _, p1 = _net(head=1)
    assert not p1.stochastic
    _, _, pf = _net(head=1, log_std=-0.7)
    assert pf.stochastic and pf.log_std == np.float32(-0.7)
    with pytest.raises(ValueError):                       # a two-row head has its own log-std
        ph.MLPPolicy(ws, bs, log_std=0.0)
    with pytest.raises(ValueError):
        ph.MLPPolicy(ws[:1] + [np.zeros((3, 8), np.float32)], bs[:1] + [np.zeros(3, np.float32)])
    with pytest.raises(ValueError):
        _net(head=1, log_std=float("nan"))
    with pytest.raises(ValueError):                       # the existing refusals stay
        ph.MLPPolicy([np.zeros((65, 3)), np.zeros((2, 65))], [np.zeros(65), np.zeros(2)])
    with pytest.raises(ValueError):
        ph.MLPPolicy([np.zeros((4, 3)), np.zeros((2, 4))], [np.zeros(4), np.zeros(2)], out_lo=-1.0)
    # deterministic use of a two-row head is its mean row (RLlib's deterministic_sample)
    x = np.random.default_rng(1).random((50, 3)).astype(np.float32)
    mean_only = ph.MLPPolicy(ws[:1] + [ws[1][:1]], bs[:1] + [bs[1][:1]], out_scale=50.0, out_bias=50.0)
    np.testing.assert_array_equal(f32_bits(pr.action(p2, x)), f32_bits(pr.action(mean_only, x)))
    np.testing.assert_allclose(p2(torch.from_numpy(x)).numpy(), mean_only(torch.from_numpy(x)).numpy(), rtol=1e-5, atol=1e-4)
    mean, ls = p2.distribution(torch.from_numpy(x))
    y, l = per.heads(p2, x)
    np.testing.assert_allclose(mean.numpy(), y, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ls.numpy(), l, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        p1.distribution(torch.from_numpy(x))


def test_from_torch_takes_a_diag_gaussian_head():
    net = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 2))
    p = ph.MLPPolicy.from_torch(net, out_scale=50.0, out_bias=50.0)
    assert p.stochastic and p.activation == "tanh"
    x = torch.rand(20, 3)
    mean, ls = p.distribution(x)
    with torch.no_grad():
        out = net(x)
    np.testing.assert_allclose(mean.numpy(), out[:, 0].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ls.numpy(), out[:, 1].numpy(), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):                       # the refusals of from_torch stay
        ph.MLPPolicy.from_torch(torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Sigmoid(), torch.nn.Linear(16, 2)))
    with pytest.raises(ValueError):
        ph.MLPPolicy.from_torch(torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, 3)))


def test_explore_struct_and_update():
    """the log-std row is the head's second row (device copies), a free log-std a one-float tensor; noise with a deterministic policy
    raises; update() refreshes both"""
    ws, bs, p2 = _net(head=2)
    T, B, S = 3, 2, 4
    planes = [torch.zeros(T, B, S), torch.zeros(T, B, S), torch.zeros(T, B, S), torch.zeros(T, B, S, 2)]
    x = p2.explore_struct("cpu", *planes)
    dw, db, _ = p2.on("cpu")
    assert x.w_log_std == dw[-1].data_ptr() + 8 * 4 and x.b_log_std == db[-1].data_ptr() + 4
    assert x.noise == planes[0].data_ptr() and x.dist_inputs == planes[3].data_ptr()
    ws2 = [w * 2 for w in ws]
    p2.update(ws2, bs)
    np.testing.assert_array_equal(dw[-1][1].numpy(), ws2[-1][1])
    _, _, pf = _net(head=1, log_std=-1.5)
    xf = pf.explore_struct("cpu", *planes)
    assert xf.w_log_std is None
    assert C.c_float.from_address(xf.b_log_std).value == -1.5
    pf.update(pf.weights, pf.biases, log_std=0.25)
    assert C.c_float.from_address(xf.b_log_std).value == 0.25
    _, _, p1 = _net(head=1)
    with pytest.raises(ValueError):
        p1.explore_struct("cpu", *planes)
    with pytest.raises(ValueError):
        p1.update(p1.weights, p1.biases, log_std=0.0)


def test_sample_batches_carry_rllibs_columns():
    B, S, T, D = 2, 3, 4, 3
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    raw, logp, dist = f(B, S, T), f(B, S, T) - 2, f(B, S, T, 2)
    act = np.clip(50 * raw + 50, 0, 100).astype(np.float32)
    t = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    eps = np.broadcast_to(np.arange(B, dtype=np.int64)[:, None], (B, T)).copy()
    z = np.zeros((B, S, T), bool)
    fb = FragmentBatch(["a", "b", "c"], f(B, S, T, D), f(B, S, T, D), act, f(B, S, T), z, z, t, eps, raw_actions=raw,
                       action_logp=logp, dist_inputs=dist)
    sb = fb.to_sample_batches()["default_policy"]
    np.testing.assert_array_equal(sb["actions"], raw.reshape(-1, 1))
    np.testing.assert_array_equal(sb["action_logp"], logp.reshape(-1))
    np.testing.assert_allclose(sb["action_prob"], np.exp(logp.reshape(-1)))
    np.testing.assert_array_equal(sb["action_dist_inputs"], dist.reshape(-1, 2))
    # two policies over non-contiguous agents: the columns follow the rows
    sb2 = fb.to_sample_batches(lambda aid: "odd" if aid == "b" else "even")
    np.testing.assert_array_equal(sb2["odd"]["action_logp"], logp[:, 1].reshape(-1))
    np.testing.assert_array_equal(sb2["even"]["action_dist_inputs"], dist[:, [0, 2]].reshape(-1, 2))
    # the reference's containers keep showing the env's actions
    assert fb.step(0, 1).actions["b"][0] == act[0, 1, 1]
    plain = FragmentBatch(["a", "b", "c"], f(B, S, T, D), f(B, S, T, D), act, f(B, S, T), z, z, t, eps)
    cols = plain.to_sample_batches()["default_policy"]
    assert "action_logp" not in cols and (cols["actions"] == act.reshape(-1, 1)).all()


def test_cpu_library_refuses_an_exploring_io():
    """the restatement behind the product's symbols (oracle/libphantom_cpu.so) refuses a non-NULL reserved_ptr / explore with PHX_EINVAL,
    as a library older than exploration does"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "libphantom_cpu.so"])
    lib = _abi.bind_signatures(C.CDLL(os.path.join(ROOT, "oracle", "libphantom_cpu.so")))
    B, S, T = 4, 3, 5
    env = supply_chain_env(S, [2] * S, 10, B, seed=5)
    cs, keep = env.spec.to_ctypes()
    n = lib.phx_state_nbytes(C.byref(cs))
    blob = np.zeros(n, np.uint8)
    h = C.c_void_p()
    assert lib.phx_create(C.byref(cs), 0, blob.ctypes.data, n, C.byref(h)) == 0
    try:
        obs0 = np.zeros((B, S, 3), np.float32); ov = np.zeros((B, S), np.uint8)
        assert lib.phx_reset(h, None, None, None, obs0.ctypes.data, ov.ctypes.data, None) == 0
        _, _, pol = _net(head=2)
        pstruct = pol.host_struct()
        bufs = [np.zeros((T, B, S, 3), np.float32)] + [np.zeros((T, B, S), np.float32) for _ in range(2)] + \
               [np.zeros((T, B, S), np.uint8) for _ in range(2)] + [np.zeros((B, S, 3), np.float32)]
        err = np.full(B, 7, np.int32)
        planes = [torch.zeros(T, B, S), torch.zeros(T, B, S), torch.zeros(T, B, S), torch.zeros(T, B, S, 2)]
        ex = pol.explore_struct("cpu", *planes)
        io = _abi.PhxRolloutIO()
        io.T = T
        io.obs, io.action_out, io.reward, io.terminated, io.truncated, io.last_obs = (b.ctypes.data for b in bufs)
        io.err = err.ctypes.data
        io.policy = C.addressof(pstruct)
        io.reserved_ptr = C.addressof(ex)
        assert lib.phx_rollout(h, C.byref(io), None) == -1                   # PHX_EINVAL
        io.policy = None
        assert lib.phx_rollout(h, C.byref(io), None) == -1
        assert (err == 7).all() and not bufs[0].any()
    finally:
        lib.phx_destroy(h)
    assert C.sizeof(_abi.PhxRolloutIO) == 144 and _abi.PhxRolloutIO.reserved_ptr.offset == 112    # the layout did not change
