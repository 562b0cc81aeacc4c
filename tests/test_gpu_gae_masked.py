"""phx_gae_masked (include/phantom_amd_gae.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the
numpy restatement (tests/gae_masked_ref.py) over column counts around the workgroup's and row counts around the kernel's chunk
depth, every optional plane, misaligned inputs, the reduction to phx_gae, every refusal; then DeviceEnv.gae_masked on a real FSM
rollout, the reference's FSM rollout through PhantomEnv.sample(), and sample(value_fn=...) on FSM and Stackelberg envs against
a twin env's rollout() planes."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gae_masked_ref as gm
import gae_ref
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import f32_bits, market_env, supply_chain_env
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_gae_masked.hip")).read()
K = int(re.search(r"constexpr int GMK_K = (\d+);", SRC).group(1))                 # the kernel's chunk depth (rows)
WG = int(re.search(r"constexpr int GMK_LANES = (\d+);", SRC).group(1))            # the workgroup's columns
NS = (1, 63, 64, 65, 549, 4 * 64 + 2)
TS = (1, 2, K - 1, K, K + 1, 2 * K + 1, 100)
F32_INPUTS = ("reward", "vf_pred", "vf_next")
INPUTS = F32_INPUTS + ("terminated", "truncated", "acted", "reward_valid")
OUTPUTS = ("advantage", "value_target", "reward_sum")
NAN = np.float32(np.nan)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _offset(host, nbytes):
    """`host` on the device, starting `nbytes` bytes past a 16-byte boundary (0: on one)"""
    a = np.ascontiguousarray(host)
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device=_dev())
    assert raw.data_ptr() % 16 == 0
    x = raw[nbytes:nbytes + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    x.copy_(torch.from_numpy(a))
    assert x.data_ptr() % 16 == nbytes
    return x


class Call:
    """one phx_gae_masked call: device inputs (NaN wherever the definition does not read vf_next, vf_pred or reward), fenced outputs"""

    def __init__(self, case, gamma, lam, nulls=(), offset=0, poison=True):
        self.case, self.gamma, self.lam, self.nulls = case, gamma, lam, set(nulls)
        T, N = case["reward"].shape
        self.T, self.N = T, N
        given = lambda k: None if k in self.nulls else case[k]
        rd = gm.reads(case["truncated"], given("terminated"), given("acted"), given("reward_valid"))
        self.dev = {}
        for k in INPUTS:
            if k in self.nulls:
                continue
            host = case[k]
            if k in F32_INPUTS and poison:
                host = np.where(rd[k], host, NAN)
            self.dev[k] = _offset(host, offset if k in F32_INPUTS else 0)
        self.before = {k: v.cpu().numpy().copy() for k, v in self.dev.items()}
        self.out, self.whole = {}, {}
        for k in OUTPUTS:
            self.out[k], self.whole[k] = fenced((T, N), torch.float32, _dev())
        p = lambda k: self.dev[k].data_ptr() if k in self.dev else None
        o = lambda k: None if k in self.nulls else self.out[k].data_ptr()
        self.io = _abi.PhxGaeMaskedIO(T=T, N=N, gamma=gamma, lambda_=lam, reward=p("reward"), vf_pred=p("vf_pred"), vf_next=p("vf_next"),
                                      terminated=p("terminated"), truncated=p("truncated"), acted=p("acted"), reward_valid=p("reward_valid"),
                                      advantage=o("advantage"), value_target=o("value_target"), reward_sum=o("reward_sum"))

    def launch(self):
        return _abi.load_library().phx_gae_masked(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def reference(self):
        ref = {k: (None if k in self.nulls else self.case[k]) for k in INPUTS}
        return dict(zip(OUTPUTS, gm.gae_masked(ref["reward"], ref["truncated"], ref["vf_pred"], ref["vf_next"], ref["terminated"], ref["acted"],
                                               ref["reward_valid"], self.gamma, self.lam)))

    def check(self, what=""):
        want = self.reference()
        for k in OUTPUTS:
            assert_fences(self.whole[k], self.T, what + k)
            if k in self.nulls:
                assert_poison(self.out[k], what + k + " (NULL: not written)")
                continue
            assert_written(self.out[k], what + k)
            np.testing.assert_array_equal(f32_bits(self.out[k].cpu().numpy()), f32_bits(want[k]), err_msg=what + k)
        for k, v in self.dev.items():                   # the inputs are byte-identical after the call
            np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), self.before[k].view(np.uint8), err_msg=what + k)

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k in OUTPUTS:
            assert_poison(self.whole[k], f"{what}: {k}")


def _case(T, N, seed=0):
    return gm.random_case(np.random.default_rng([seed, T, N]), T, N)


def _run(T, N, gamma=0.99, lam=0.95, seed=0, **kw):
    call = Call(_case(T, N, seed), gamma, lam, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    for T in TS:
        call = _run(T, N)
        if 63 <= N <= 65 and T >= 15:                   # (the generator's hard columns are there: tests/test_gae_masked_cpu.py)
            f = gm.features(call.case)
            assert f["no_trajectory_row"] and f["two_cut_rows"] and f["term_cut_on_hole"] and f["trunc_cut_on_hole"] and f["no_present_reward"]


def test_large_fragment_many_workgroups_and_chunks():
    _run(4 * K + 3, 61 * 9 * 5 + 1)                     # 43 workgroups, the last one with one live lane; 5 chunks


@pytest.mark.parametrize("null", ["vf_pred", "vf_next", "terminated", "acted", "reward_valid", "value_target", "reward_sum"])
def test_each_optional_plane_left_out(null):
    for T, N in ((K + 1, 65), (3, 549)):
        _run(T, N, nulls=(null,))


def test_all_optional_planes_left_out():
    _run(2 * K + 1, 67, nulls=("vf_pred", "vf_next", "terminated", "acted", "reward_valid", "value_target", "reward_sum"))


def test_inputs_four_bytes_past_a_16_byte_boundary():
    for T, N in ((2 * K + 1, 65), (K, 549), (5, 3)):    # (a slice [t0:t1] of a longer recording: sample()'s pieces)
        _run(T, N, offset=4)


@pytest.mark.parametrize("gamma,lam", [(1.0, 1.0), (0.0, 0.5)])
def test_gamma_lambda_corners(gamma, lam):
    _run(2 * K + 1, 130, gamma=gamma, lam=lam)


@pytest.mark.parametrize("ones", [False, True])
def test_reduction_to_phx_gae_on_the_same_buffers(ones):
    """acted and reward_valid NULL (or all one): phx_gae's advantages and value targets bit for bit, reward_sum == reward; with -0.0 inside"""
    lib = _abi.load_library()
    T, N = 2 * K + 1, 549
    rng = np.random.default_rng(21)
    case = gae_ref.random_case(rng, T, N)
    for k in F32_INPUTS:
        case[k][rng.random((T, N)) < 0.1] = np.float32(-0.0)
    case["acted"] = case["reward_valid"] = np.ones((T, N), np.uint8)
    call = Call(case, 0.99, 0.95, nulls=() if ones else ("acted", "reward_valid"), poison=False)
    assert call.launch() == 0, lib.phx_last_error()
    adv, adv_whole = fenced((T, N), torch.float32, _dev())
    vt, vt_whole = fenced((T, N), torch.float32, _dev())
    d = call.dev
    io = _abi.PhxGaeIO(T=T, N=N, gamma=0.99, lambda_=0.95, reward=d["reward"].data_ptr(), vf_pred=d["vf_pred"].data_ptr(),
                       vf_next=d["vf_next"].data_ptr(), terminated=d["terminated"].data_ptr(), truncated=d["truncated"].data_ptr(),
                       advantage=adv.data_ptr(), value_target=vt.data_ptr())
    assert lib.phx_gae(C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib.phx_last_error()
    assert lib.phx_last_kernel() == b"phx_gae_kernel"
    call.check()
    np.testing.assert_array_equal(f32_bits(call.out["advantage"].cpu().numpy()), f32_bits(adv.cpu().numpy()))
    np.testing.assert_array_equal(f32_bits(call.out["value_target"].cpu().numpy()), f32_bits(vt.cpu().numpy()))
    np.testing.assert_array_equal(f32_bits(call.out["reward_sum"].cpu().numpy()), f32_bits(case["reward"]))
    assert (f32_bits(case["reward"]) == 0x80000000).any()


def test_every_refusal_leaves_the_outputs_untouched():
    lib = _abi.load_library()
    case = _case(K + 1, 65, seed=1)

    def refused(what, **patch):
        call = Call(case, 0.99, 0.95)
        for k, v in patch.items():
            setattr(call.io, k, v(getattr(call.io, k)) if callable(v) else v)
        assert call.launch() == -1, what                # PHX_EINVAL
        assert b"phx_gae_masked" in lib.phx_last_error(), what
        call.check_untouched(what)

    for k in ("reward", "truncated", "advantage"):
        refused(f"{k} NULL", **{k: None})
    for k in ("reward", "vf_pred", "vf_next"):
        refused(f"{k} misaligned", **{k: lambda p: p + 2})
    for k in OUTPUTS:
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 4})
    refused("T = 0", T=0)
    refused("T < 0", T=-3)
    refused("N = 0", N=0)
    refused("N < 0", N=-1)
    refused("N beyond the grid", N=64 * 0x7fffffff + 1)
    for k in ("gamma", "lambda_"):
        for bad in (-0.01, 1.5, float("nan")):
            refused(f"{k} = {bad}", **{k: bad})
    refused("reserved0", reserved0=1)
    assert lib.phx_gae_masked(None, None) == -1 and b"phx_gae_masked" in lib.phx_last_error()


def test_last_kernel_names_the_kernel():
    _run(3, 7)
    assert _abi.load_library().phx_last_kernel() == b"phx_gae_masked_kernel" == _abi.GAE_MASKED_KERNEL.encode()


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(_case(2 * K + 1, 549, seed=11), 0.99, 0.95)
    b = Call(_case(K - 1, 130, seed=12), 0.9, 1.0, nulls=("vf_next", "acted"))
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
S, B, STEPS, T = 5, 13, 7, 20


def _fsm_env(seed=5):
    env = supply_chain_env(S, [3] * S, STEPS, B, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


def _stk_env(seed=5):
    env = market_env(2, 3, 2, 6, 7, seed=seed, exogenous="device")
    env.reset()
    return env


class Twin:
    """an env with the same seed, driven through reset() and rollout() only: the planes sample() must have put together"""

    def __init__(self, make):
        self.env = make()
        dev = self.env._device()
        self.cur_obs, self.cur_valid, self.cur = dev.obs.clone(), dev.obs_valid.clone(), 0
        self.reset_valid = dev.obs_valid.clone()        # the validity reset() returns for the initial stage

    def planes(self, T):
        N = self.env.num_steps
        rows = {k: [] for k in ("obs", "new_obs", "acted", "nvalid", "rvalid", "rewards", "truncations", "terminations", "actions")}
        done, ends = 0, []
        while done < T:
            n = min(T - done, N - self.cur)
            tr = self.env.rollout(n)
            rows["obs"] += [self.cur_obs[None].clone(), tr.observations[:n - 1].clone()]
            rows["acted"] += [self.cur_valid[None].clone(), tr.obs_valid[:n - 1].clone()]
            for k, x in (("new_obs", tr.observations), ("nvalid", tr.obs_valid), ("rvalid", tr.reward_valid), ("rewards", tr.rewards),
                         ("truncations", tr.truncations), ("terminations", tr.terminations), ("actions", tr.actions)):
                rows[k].append(x.clone())
            self.cur_obs = tr.last_obs.clone()
            self.cur += n
            self.cur_valid = self.reset_valid if self.cur == N else tr.obs_valid[n - 1].clone()
            self.cur %= N
            done += n
            ends.append(done - 1)
        return {k: torch.cat(v).cpu().numpy() for k, v in rows.items()}, ends


def _critic(x):
    """element-wise operations on the observation's columns only: a row's value does not depend on the other rows of the call"""
    return 0.5 * x[:, 0] - 0.25 * torch.tanh(x[:, 1]) + 0.125 * x[:, -1] * x[:, -1] + 0.75


def _expected(p, ends, gamma, lam, with_critic=True):
    """the value planes from the twin's planes, then the restatement"""
    if not with_critic:
        return None, gm.gae_masked(p["rewards"], p["truncations"], None, None, p["terminations"], p["acted"], p["rvalid"], gamma, 1.0)
    Tn, Bn, Sn, D = p["obs"].shape
    v = lambda a: _critic(torch.from_numpy(np.ascontiguousarray(a)).to(_dev()).reshape(-1, D)).reshape(a.shape[:-1]).cpu().numpy()
    vf = v(np.where((p["acted"] != 0)[..., None], p["obs"], np.float32(0)))
    vfn = np.full((Tn, Bn, Sn), NAN, np.float32)                       # (unread elements may hold anything)
    first = 0
    for last in ends:
        held = p["obs"][first].copy()                                  # what the agent holds at the piece's last row
        for t in range(first, last + 1):
            held = np.where((p["nvalid"][t] != 0)[..., None], p["new_obs"][t], held)
        vfn[last] = v(held)
        first = last + 1
    return vf, gm.gae_masked(p["rewards"], p["truncations"], vf, vfn, p["terminations"], p["acted"], p["rvalid"], gamma, lam)


def _check_batch(batch, p, ends, gamma, lam, with_critic=True):
    tm = lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0))          # [B, S, T, ..] -> [T, B, S, ..]
    np.testing.assert_array_equal(tm(batch.obs_valid), p["acted"])
    np.testing.assert_array_equal(tm(batch.new_obs_valid), p["nvalid"])
    np.testing.assert_array_equal(tm(batch.reward_valid), p["rvalid"])
    np.testing.assert_array_equal(f32_bits(tm(batch.new_obs)), f32_bits(p["new_obs"]))
    np.testing.assert_array_equal(f32_bits(tm(batch.rewards)), f32_bits(p["rewards"]))
    acted = p["acted"] != 0
    np.testing.assert_array_equal(f32_bits(tm(batch.obs)[acted]), f32_bits(p["obs"][acted]))
    vf, (adv, vt, rs) = _expected(p, ends, gamma, lam, with_critic)
    np.testing.assert_array_equal(f32_bits(tm(batch.trajectory_rewards)), f32_bits(rs))
    cols = batch.to_sample_batches()["default_policy"]
    am = lambda a: np.moveaxis(a, 0, 2)[np.moveaxis(acted, 0, 2)]      # the masked plane in (env, agent, step) order
    np.testing.assert_array_equal(f32_bits(cols["rewards"]), f32_bits(am(rs)))
    assert len(cols["obs"]) == int(acted.sum())
    if with_critic:
        np.testing.assert_array_equal(f32_bits(tm(batch.vf_preds)[acted]), f32_bits(vf[acted]))
        np.testing.assert_array_equal(f32_bits(tm(batch.advantages)), f32_bits(adv))
        np.testing.assert_array_equal(f32_bits(tm(batch.value_targets)), f32_bits(vt))
        for name, want in (("vf_preds", vf), ("advantages", adv), ("value_targets", vt)):
            np.testing.assert_array_equal(f32_bits(cols[name]), f32_bits(am(want)), err_msg=name)
    else:
        assert batch.vf_preds is None and batch.advantages is None and "advantages" not in cols
    return cols


def test_device_env_gae_masked_on_a_real_fsm_rollout():
    twin = Twin(_fsm_env)
    p, ends = twin.planes(T)
    assert ends == [STEPS - 1, 2 * STEPS - 1, T - 1] and p["truncations"][STEPS - 1].all()
    acted = p["acted"] != 0
    assert 0.2 < acted.mean() < 0.8 and set(np.unique(p["rvalid"]).tolist()) >= {0, 1}       # the shops observe every second step
    dev = twin.env._device()
    to = lambda a: torch.from_numpy(a).to(dev.device)
    g = torch.Generator(device=dev.device).manual_seed(3)
    vf = torch.randn((T, B, S), generator=g, device=dev.device)
    vfn = torch.randn((T, B, S), generator=g, device=dev.device)
    args = (to(p["rewards"]), to(p["truncations"]), vf, vfn, to(p["terminations"]), to(p["acted"]), to(p["rvalid"]))
    got = dev.gae_masked(*args, gamma=0.99, lambda_=0.95)
    assert dev.last_kernel() == "phx_gae_masked_kernel" and all(x.shape == (T, B, S) for x in got)
    want = gm.gae_masked(p["rewards"], p["truncations"], vf.cpu().numpy(), vfn.cpu().numpy(), p["terminations"], p["acted"], p["rvalid"], 0.99, 0.95)
    for x, w, name in zip(got, want, OUTPUTS):
        np.testing.assert_array_equal(f32_bits(x.cpu().numpy()), f32_bits(w), err_msg=name)
    # every reward that counts is credited exactly once: per column, the trajectory rewards are the rewards reads() names
    rd = gm.reads(p["truncations"], p["terminations"], p["acted"], p["rvalid"])["reward"]
    counted = np.where(rd, p["rewards"], 0).astype(np.float64)
    err = np.abs(got[2].cpu().numpy().astype(np.float64).sum(axis=0) - counted.sum(axis=0))
    assert (err <= T * 2.0 ** -24 * np.abs(counted).sum(axis=0)).all()      # (at most T f32 additions per column, half an ulp each)
    # refusals at this level leave caller-owned outputs untouched
    outs = [fenced((T, B, S), torch.float32, dev.device) for _ in range(3)]
    out = tuple(o[0] for o in outs)
    for name, i, bad in (("acted", 5, args[5].to(torch.float32)), ("acted", 5, args[5][:-1]), ("reward_valid", 6, args[6].to(torch.int32)),
                         ("reward_valid", 6, args[6][:, :-1].contiguous())):
        a = list(args); a[i] = bad
        with pytest.raises(ValueError, match=name):
            dev.gae_masked(*a, out=out)
    with pytest.raises(ValueError, match="gamma"):
        dev.gae_masked(*args, gamma=1.5, out=out)
    torch.cuda.synchronize()
    for _, whole in outs:
        assert_poison(whole, "a refused DeviceEnv.gae_masked call")
    res = dev.gae_masked(*args, gamma=0.99, lambda_=0.95, out=out)                            # and a good call fills them
    assert res[0].data_ptr() == out[0].data_ptr()
    for (plane, whole), w, name in zip(outs, want, OUTPUTS):
        assert_fences(whole, T, name)
        np.testing.assert_array_equal(f32_bits(plane.cpu().numpy()), f32_bits(w), err_msg=name)


def test_the_references_fsm_rollout_through_sample():
    from test_rollout_containers import _check_rollouts, _env, _load
    g, Tg, Bg, Sg, n_exo, fsm, exo = _load("sc_fsm")
    assert fsm
    env = _env("sc_fsm", Bg, Tg)
    ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
    env.reset()
    dev = env._device().device
    frag = env.sample(Tg, torch.from_numpy(g["actions"].copy()).to(dev), torch.from_numpy(exo).to(dev))
    assert env._device().last_kernel() == "phx_gae_masked_kernel"
    _check_rollouts(frag, g, ids, Tg, Bg, True)
    cols = frag.to_sample_batches()["default_policy"]
    assert len(cols["rewards"]) == int(g["obs_key"].sum())
    assert frag.trajectory_rewards is not None and frag.vf_preds is None


@pytest.mark.parametrize("make,Tn", [(_fsm_env, 20), (_fsm_env, 19), (_stk_env, 20)])
def test_sample_with_a_critic_against_a_twin_envs_rollouts(make, Tn):
    gamma, lam = 0.99, 0.95
    env, twin = make(), Twin(make)
    batch = env.sample(Tn, value_fn=_critic, gamma=gamma, lambda_=lam)
    assert env._device().last_kernel() == "phx_gae_masked_kernel"
    p, ends = twin.planes(Tn)
    acted = p["acted"] != 0
    assert 0.2 < acted.mean() < 0.8 and len(ends) >= 3
    if Tn == 19:                                                        # the last row is an acting row with no answer yet
        assert acted[Tn - 1].any() and not p["truncations"][Tn - 1].any()
    cols = _check_batch(batch, p, ends, gamma, lam)
    if make is _fsm_env:
        assert batch.stage_ids == ["RESTOCK", "SELL"] and batch.stage.shape == (B, Tn)
        assert (batch.stage == batch.t % 2).all()                       # RESTOCK -> SELL -> RESTOCK from every reset on
        assert (batch.obs_valid.any(axis=1) == (batch.stage == 0)).all()   # the shops act in RESTOCK steps
    else:
        assert batch.stage is None
    # the same columns through the RLlib adapter (same seed, fresh env)
    sb = ph.rllib.BatchedBaseEnv(make()).sample(Tn, value_fn=_critic, gamma=gamma, lambda_=lam)["default_policy"]
    for name in ("rewards", "advantages", "value_targets", "vf_preds", "obs"):
        np.testing.assert_array_equal(f32_bits(sb[name]), f32_bits(cols[name]), err_msg=name)
    # a second call continues: its first row's validity is what the first call left
    again = env.sample(5, value_fn=_critic, gamma=gamma, lambda_=lam)
    p2, ends2 = twin.planes(5)
    _check_batch(again, p2, ends2, gamma, lam)
    if Tn == 19:
        np.testing.assert_array_equal(again.obs_valid[:, :, 0], p["nvalid"][Tn - 1])
    # and without a critic: the same launch for trajectory_rewards alone
    env3, twin3 = make(), Twin(make)
    p3, ends3 = twin3.planes(Tn)
    _check_batch(env3.sample(Tn), p3, ends3, gamma, lam, with_critic=False)
    assert env3._device().last_kernel() == "phx_gae_masked_kernel"


def test_fsm_sample_refuses_a_device_policy():
    rng = np.random.default_rng(2)
    pol = ph.MLPPolicy([rng.normal(0, 0.7, (16, 3)).astype(np.float32), rng.normal(0, 0.3, (1, 16)).astype(np.float32)],
                       [np.zeros(16, np.float32), np.zeros(1, np.float32)], activation="relu", out_scale=50.0, out_bias=50.0, out_lo=0.0, out_hi=100.0)
    with pytest.raises(ValueError, match="plain envs only"):
        _fsm_env().sample(T, policy=pol)


def test_a_plain_envs_sample_is_what_it_was():
    env = supply_chain_env(9, [6] * 9, 7, 11, seed=5, exogenous="device")
    env.reset()
    batch = env.sample(T, value_fn=_critic, gamma=0.99, lambda_=0.95)
    assert env._device().last_kernel() == "phx_gae_kernel"
    assert batch.trajectory_rewards is None and batch.obs_valid is None and batch.reward_valid is None and batch.stage is None
    cols = batch.to_sample_batches()["default_policy"]
    np.testing.assert_array_equal(f32_bits(cols["rewards"]), f32_bits(batch.rewards.reshape(-1)))
    assert batch.advantages.shape == (11, 9, T)
