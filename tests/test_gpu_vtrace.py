"""phx_vtrace (include/phantom_amd_vtrace.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the
numpy restatement (tests/vtrace_ref.py) over column counts around the workgroup's and row counts around the kernel's chunk depth, the
optional planes, misaligned inputs, the parameter corners, the reduction to phx_gae on the same buffers, every refusal; then
DeviceEnv.vtrace on a real rollout and PhantomEnv.sample(target_logp_fn=...)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vtrace_ref as vr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import f32_bits, supply_chain_env
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_vtrace.hip")).read()
K = int(re.search(r"constexpr int VT_K = (\d+);", SRC).group(1))                  # the kernel's chunk depth (rows)
WG = int(re.search(r"constexpr int VT_LANES = (\d+);", SRC).group(1))             # the workgroup's columns
NS = (1, 3, 63, 64, 65, 549, WG - 2, WG + 2, 4 * WG + 2)                          # (549 = 61 * 9; 4 k + 2 around the workgroup's columns)
TS = (1, 2, K - 1, K, K + 1, 2 * K + 1, 100)
INPUTS = ("reward", "vf_pred", "vf_next", "behaviour_logp", "target_logp", "terminated", "truncated")
DEFAULT = dict(gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0)


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
    """one phx_vtrace call: device inputs (vf_next poisoned wherever the definition does not read it), fenced outputs"""

    def __init__(self, case, nulls=(), offset=0, same_logp=False, **params):
        self.case, self.nulls, self.params = dict(case), set(nulls), {**DEFAULT, **params}
        if same_logp:
            self.case["target_logp"] = self.case["behaviour_logp"]
        T, N = case["reward"].shape
        self.T, self.N = T, N
        self.dev = {}
        reads = vr.reads_vf_next(None if "terminated" in self.nulls else case["terminated"], case["truncated"])
        for k in INPUTS:
            if k in self.nulls:
                continue
            if k == "target_logp" and same_logp:
                self.dev[k] = self.dev["behaviour_logp"]            # the same pointer
            elif k == "vf_next" and not offset:
                plane, whole = fenced((T, N), torch.float32, _dev())
                self.vf_next_whole = whole
                on = torch.from_numpy(reads).to(_dev())
                plane[on] = torch.from_numpy(case["vf_next"]).to(_dev())[on]
                self.dev[k] = plane
            else:                                       # (a misaligned vf_next: poisoned the same way, inside a plain buffer)
                host = self.case[k]
                if k == "vf_next":
                    host = np.where(reads, host, np.frombuffer(b"\xa5" * 4, np.float32)[0])
                self.dev[k] = _offset(host, offset)
        self.before = {k: v.cpu().numpy().copy() for k, v in self.dev.items()}
        self.vs, self.vs_whole = fenced((T, N), torch.float32, _dev())
        self.pg, self.pg_whole = fenced((T, N), torch.float32, _dev())
        p = lambda k: self.dev[k].data_ptr() if k in self.dev else None
        q = self.params
        self.io = _abi.PhxVtraceIO(T=T, N=N, gamma=q["gamma"], lambda_=q["lam"], rho_bar=q["rho_bar"], c_bar=q["c_bar"], pg_rho_bar=q["pg_rho_bar"],
                                   reward=p("reward"), vf_pred=p("vf_pred"), vf_next=p("vf_next"), behaviour_logp=p("behaviour_logp"),
                                   target_logp=p("target_logp"), terminated=p("terminated"), truncated=p("truncated"), vs=self.vs.data_ptr(),
                                   pg_advantage=None if "pg_advantage" in self.nulls else self.pg.data_ptr())

    def launch(self):
        lib = _abi.load_library()
        return lib.phx_vtrace(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def reference(self):
        ref = {k: (None if k in self.nulls else self.case[k]) for k in INPUTS}
        return vr.vtrace(**ref, **self.params)

    def check(self, what=""):
        vs, pg = self.reference()
        assert_fences(self.vs_whole, self.T, what + "vs")
        assert_fences(self.pg_whole, self.T, what + "pg_advantage")
        assert_written(self.vs, what + "vs")
        np.testing.assert_array_equal(f32_bits(self.vs.cpu().numpy()), f32_bits(vs), err_msg=what + "vs")
        if "pg_advantage" in self.nulls:
            assert_poison(self.pg, what + "pg_advantage (NULL: not written)")
        else:
            assert_written(self.pg, what + "pg_advantage")
            np.testing.assert_array_equal(f32_bits(self.pg.cpu().numpy()), f32_bits(pg), err_msg=what + "pg_advantage")
        for k, v in self.dev.items():                   # the inputs are byte-identical after the call
            np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), self.before[k].view(np.uint8), err_msg=what + k)
        if hasattr(self, "vf_next_whole"):
            assert_fences(self.vf_next_whole, self.T, what + "vf_next")

    def check_untouched(self, what):
        torch.cuda.synchronize()
        assert_poison(self.vs_whole, what + ": vs")
        assert_poison(self.pg_whole, what + ": pg_advantage")


def _case(T, N, seed=0):
    return vr.random_case(np.random.default_rng([seed, T, N]), T, N)


def _run(T, N, seed=0, **kw):
    call = Call(_case(T, N, seed), **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    for T in TS:
        _run(T, N)                                      # (what the cases hold at these shapes: tests/test_vtrace_cpu.py)


def test_large_fragment_many_workgroups_and_chunks():
    _run(4 * K + 3, 61 * 9 * 5 + 1)                     # 43 workgroups, the last one with one live lane; 5 chunks and 3 rows


@pytest.mark.parametrize("null", ["vf_next", "terminated", "pg_advantage"])
def test_each_optional_plane_left_out(null):
    for T, N in ((K + 1, 65), (3, 549)):
        _run(T, N, nulls=(null,))
    _run(2 * K + 1, 67, nulls=("vf_next", "terminated", "pg_advantage"))


def test_inputs_four_bytes_past_a_16_byte_boundary():
    for T, N in ((2 * K + 1, 65), (K, 549), (5, 3)):    # (a slice [t0:t1] of a longer recording: sample()'s pieces)
        _run(T, N, offset=4)


@pytest.mark.parametrize("params", [dict(gamma=0.0, lam=0.5), dict(gamma=1.0, lam=0.0), dict(gamma=1.0, lam=1.0),
                                    dict(rho_bar=0.5, c_bar=2.0, pg_rho_bar=2.0), dict(rho_bar=2.0, c_bar=0.5, pg_rho_bar=0.5),
                                    dict(lam=1.0, rho_bar=1e9, c_bar=1.0, pg_rho_bar=1e9)], ids=str)
def test_parameter_corners(params):
    """gamma = 0, lambda in {0, 1}, thresholds 0.5 / 1 / 2 and one above e^20 (rc and rp are then rho itself, up to e^20)"""
    assert 1e9 > math.exp(20.0)
    call = _run(2 * K + 1, 130, **params)
    if params.get("gamma") == 0.0:                      # vs = rc (r - v) + v exactly: nothing is carried
        c = call.case
        rc = vr.weights(c["behaviour_logp"], c["target_logp"], 0.0, 0.5, 1.0, 1.0, 1.0)[1]
        want = vr._fadd(vr.fmul(rc, vr.fsub(c["reward"], c["vf_pred"])), c["vf_pred"])
        np.testing.assert_array_equal(f32_bits(call.vs.cpu().numpy() + np.float32(0)), f32_bits(want + np.float32(0)))


@pytest.mark.parametrize("thresholds", [(1.0, 1.0, 1.0), (1.5, 2.0, 1.0)])
def test_the_same_logp_pointer_gives_phx_gaes_value_target(thresholds):
    """target_logp and behaviour_logp the SAME pointer, thresholds >= 1: vs equals the value_target of a phx_gae call on the same
    device buffers bit for bit"""
    lib = _abi.load_library()
    for (T, N), (gamma, lam) in zip(((2 * K + 1, 549), (K + 1, 65)), ((0.99, 0.95), (0.99, 1.0))):
        call = Call(_case(T, N, seed=3), same_logp=True, gamma=gamma, lam=lam, rho_bar=thresholds[0], c_bar=thresholds[1], pg_rho_bar=thresholds[2])
        assert call.io.target_logp == call.io.behaviour_logp
        assert call.launch() == 0, lib.phx_last_error()
        call.check("same pointer: ")
        adv, adv_whole = fenced((T, N), torch.float32, _dev())
        vt, vt_whole = fenced((T, N), torch.float32, _dev())
        io = _abi.PhxGaeIO(T=T, N=N, gamma=gamma, lambda_=lam, reward=call.io.reward, vf_pred=call.io.vf_pred, vf_next=call.io.vf_next,
                           terminated=call.io.terminated, truncated=call.io.truncated, advantage=adv.data_ptr(), value_target=vt.data_ptr())
        assert lib.phx_gae(C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib.phx_last_error()
        assert lib.phx_last_kernel() == b"phx_gae_kernel"
        assert_fences(vt_whole, T, "value_target")
        np.testing.assert_array_equal(f32_bits(call.vs.cpu().numpy()), f32_bits(vt.cpu().numpy()))


def test_every_refusal_leaves_the_outputs_untouched():
    lib = _abi.load_library()
    case = _case(K + 1, 65, seed=1)

    def refused(what, **patch):
        call = Call(case)
        for k, v in patch.items():
            setattr(call.io, k, v(getattr(call.io, k)) if callable(v) else v)
        assert call.launch() == -1, what                # PHX_EINVAL
        assert b"phx_vtrace" in lib.phx_last_error(), what
        call.check_untouched(what)

    for k in ("reward", "vf_pred", "behaviour_logp", "target_logp", "truncated", "vs"):
        refused(f"{k} NULL", **{k: None})
    for k in ("reward", "vf_pred", "vf_next", "behaviour_logp", "target_logp"):
        refused(f"{k} misaligned", **{k: lambda p: p + 2})
    for k in ("vs", "pg_advantage"):
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 4})
    refused("T = 0", T=0)
    refused("T < 0", T=-3)
    refused("N = 0", N=0)
    refused("N < 0", N=-1)
    refused("N beyond one launch's grid", N=WG * 0x7fffffff + 1)
    for k in ("gamma", "lambda_"):
        for bad in (-0.01, 1.5, float("nan")):
            refused(f"{k} = {bad}", **{k: bad})
    for k in ("rho_bar", "c_bar", "pg_rho_bar"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(f"{k} = {bad}", **{k: bad})
    refused("reserved0", reserved0=1)
    refused("reserved1", reserved1=1.0)
    assert lib.phx_vtrace(None, None) == -1 and b"phx_vtrace" in lib.phx_last_error()


def test_last_kernel_names_the_kernel():
    _run(3, 7)
    assert _abi.load_library().phx_last_kernel() == b"phx_vtrace_kernel" == _abi.VTRACE_KERNEL.encode()


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(_case(2 * K + 1, 549, seed=11))
    b = Call(_case(K - 1, 130, seed=12), nulls=("vf_next",), gamma=0.9, lam=1.0, rho_bar=2.0)
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface: S = 9, B = 61, 7-step episodes, T = 20 (episode ends inside the fragment) --------------------------------------
S, B, STEPS, T = 9, 61, 7, 20


def _env(seed=5):
    env = supply_chain_env(S, [6] * S, STEPS, B, seed=seed, exogenous="device")
    env.reset()
    return env


def test_device_env_vtrace_on_a_real_rollout():
    env = _env()
    dev = env._device()
    tr = env.rollout(T)
    trunc = tr.truncations.cpu().numpy()
    assert trunc[STEPS - 1].all() and trunc[2 * STEPS - 1].all() and trunc.sum() == 2 * B * S      # rows 6 and 13 end episodes
    g = torch.Generator(device=dev.device).manual_seed(3)
    rnd = lambda: torch.randn((T, B, S), generator=g, device=dev.device)
    vf, vfn, bl = rnd(), rnd(), rnd() - 1.0
    tl = bl + 0.7 * rnd()
    np_ = lambda x: x.cpu().numpy()
    vs, pg = dev.vtrace(tr.rewards, tr.truncations, vf, bl, tl, vfn, tr.terminations, gamma=0.99, lambda_=0.95, clip_rho_threshold=2.0,
                        clip_pg_rho_threshold=0.5)
    assert dev.last_kernel() == "phx_vtrace_kernel" and vs.shape == pg.shape == (T, B, S)
    want = vr.vtrace(np_(tr.rewards), trunc, np_(vf), np_(bl), np_(tl), np_(vfn), np_(tr.terminations), 0.99, 0.95, 2.0, 1.0, 0.5)
    np.testing.assert_array_equal(f32_bits(np_(vs)), f32_bits(want[0]))
    np.testing.assert_array_equal(f32_bits(np_(pg)), f32_bits(want[1]))
    out = (torch.empty_like(vs), torch.empty_like(pg))                     # caller-owned outputs, [T, N] planes, no optional plane
    flat = lambda x: x.reshape(T, B * S)
    got = dev.vtrace(flat(tr.rewards), flat(tr.truncations), flat(vf), flat(bl), flat(tl), gamma=0.9, out=(flat(out[0]), flat(out[1])))
    want = vr.vtrace(np_(flat(tr.rewards)), np_(flat(tr.truncations)), np_(flat(vf)), np_(flat(bl)), np_(flat(tl)), gamma=0.9)
    np.testing.assert_array_equal(f32_bits(np_(got[0])), f32_bits(want[0]))
    np.testing.assert_array_equal(f32_bits(np_(got[1])), f32_bits(want[1]))
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    with pytest.raises(ValueError, match="vf_pred"):
        dev.vtrace(tr.rewards, tr.truncations, vf[:-1], bl, tl)
    with pytest.raises(ValueError, match="vf_pred"):
        dev.vtrace(tr.rewards, tr.truncations, None, bl, tl)
    with pytest.raises(ValueError, match="target_logp"):
        dev.vtrace(tr.rewards, tr.truncations, vf, bl, tl.double())
    with pytest.raises(ValueError, match="truncations"):
        dev.vtrace(tr.rewards, None, vf, bl, tl)
    with pytest.raises(ValueError, match="gamma"):
        dev.vtrace(tr.rewards, tr.truncations, vf, bl, tl, gamma=1.5)
    with pytest.raises(ValueError, match="clip_c_threshold"):
        dev.vtrace(tr.rewards, tr.truncations, vf, bl, tl, clip_c_threshold=0.0)
    with pytest.raises(ValueError, match="clip_rho_threshold"):
        dev.vtrace(tr.rewards, tr.truncations, vf, bl, tl, clip_rho_threshold=float("inf"))
    with pytest.raises(ValueError, match=r"out\[1\]"):
        dev.vtrace(tr.rewards, tr.truncations, vf, bl, tl, out=(out[0], out[1][:-1]))


def _policy():
    rng = np.random.default_rng(2)
    ws = [rng.normal(0, 0.7, (16, 3)).astype(np.float32), rng.normal(0, 0.3, (2, 16)).astype(np.float32)]
    bs = [rng.normal(0, 0.3, (16,)).astype(np.float32), np.array([0.1, -0.5], np.float32)]
    return ph.MLPPolicy(ws, bs, activation="relu", out_scale=50.0, out_bias=50.0, out_lo=0.0, out_hi=100.0)


class _Learner(torch.nn.Module):
    """the learner's current Gaussian head: another network than the behaviour policy's"""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.Tanh(), torch.nn.Linear(8, 2))

    def forward(self, obs, raw):
        mean, log_std = self.body(obs).unbind(-1)
        return -0.5 * ((raw - mean) * torch.exp(-log_std)) ** 2 - log_std - 0.5 * math.log(2 * math.pi)


def test_sample_with_a_target_policy():
    env = _env()
    device = env._device().device
    torch.manual_seed(0)
    critic = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)).to(device)
    fn = _Learner().to(device)
    pol = _policy()
    clip = (2.0, 1.0, 0.5)
    batch = env.sample(T, policy=pol, explore=True, value_fn=critic, gamma=0.99, lambda_=0.95, target_logp_fn=fn, vtrace_clip=clip)
    assert env._device().last_kernel() == "phx_vtrace_kernel"
    names = ("vf_preds", "target_logp", "vtrace_vs", "vtrace_pg_advantages")
    for name in names:
        x = getattr(batch, name)
        assert x.shape == (B, S, T) and x.dtype == np.float32
    assert batch.advantages is None and batch.value_targets is None
    keep = {k: np.array(getattr(batch, k)) for k in ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "raw_actions",
                                                     "action_logp", "dist_inputs", "t", "eps_id") + names}
    tm = lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0))            # [B, S, T, ..] -> [T, B, S, ..]
    with torch.no_grad():                                               # critic and learner on the same rows in the same order
        v = lambda a: critic(torch.from_numpy(a).to(device).reshape(-1, 3)).reshape(a.shape[:-1]).cpu().numpy()
        vf = v(tm(keep["obs"]))
        tl = fn(torch.from_numpy(tm(keep["obs"])).to(device).reshape(-1, 3),
                torch.from_numpy(tm(keep["raw_actions"])).to(device).reshape(-1)).reshape(T, B, S).cpu().numpy()
        cut = tm(keep["truncateds"]) | tm(keep["terminateds"])
        ends = sorted(set(np.flatnonzero(cut.reshape(T, -1).any(axis=1)).tolist()) | {T - 1})
        assert ends == [STEPS - 1, 2 * STEPS - 1, T - 1]
        vfn = np.full((T, B, S), np.nan, np.float32)                    # (unread elements may hold anything)
        vfn[ends] = v(tm(keep["new_obs"])[ends])
    np.testing.assert_array_equal(f32_bits(tm(keep["vf_preds"])), f32_bits(vf))
    np.testing.assert_array_equal(f32_bits(tm(keep["target_logp"])), f32_bits(tl))
    assert (tl != tm(keep["action_logp"])).mean() > 0.99                # (another policy: the ratios are not 1)
    vs, pg = vr.vtrace(tm(keep["rewards"]), tm(keep["truncateds"]), vf, tm(keep["action_logp"]), tl, vfn, tm(keep["terminateds"]), 0.99, 0.95, *clip)
    np.testing.assert_array_equal(f32_bits(tm(keep["vtrace_vs"])), f32_bits(vs))
    np.testing.assert_array_equal(f32_bits(tm(keep["vtrace_pg_advantages"])), f32_bits(pg))
    cols = batch.to_sample_batches()["default_policy"]
    for name in names:
        np.testing.assert_array_equal(cols[name], keep[name].reshape(-1))
        assert cols[name].shape == cols["rewards"].shape == (B * S * T,)
    assert "advantages" not in cols and "value_targets" not in cols
    # without target_logp_fn: today's batch, bit for bit, from the phx_gae launch (same seed, fresh env)
    env2 = _env()
    ppo = env2.sample(T, policy=pol, explore=True, value_fn=critic, gamma=0.99, lambda_=0.95)
    assert env2._device().last_kernel() == "phx_gae_kernel"
    assert ppo.target_logp is None and ppo.vtrace_vs is None and ppo.vtrace_pg_advantages is None
    assert not set(names[1:]) & set(ppo.to_sample_batches()["default_policy"])
    for k in ("obs", "new_obs", "actions", "rewards", "raw_actions", "action_logp", "dist_inputs", "vf_preds"):
        np.testing.assert_array_equal(f32_bits(getattr(ppo, k)), f32_bits(keep[k]), err_msg=k)
    for k in ("terminateds", "truncateds", "t", "eps_id"):
        np.testing.assert_array_equal(getattr(ppo, k), keep[k], err_msg=k)
    import gae_ref
    adv, vt = gae_ref.gae(tm(keep["rewards"]), tm(keep["truncateds"]), vf, vfn, tm(keep["terminateds"]), 0.99, 0.95)
    np.testing.assert_array_equal(f32_bits(tm(ppo.advantages)), f32_bits(adv))
    np.testing.assert_array_equal(f32_bits(tm(ppo.value_targets)), f32_bits(vt))
    sb = ph.rllib.BatchedBaseEnv(_env()).sample(T, policy=pol, explore=True, value_fn=critic, gamma=0.99, lambda_=0.95, target_logp_fn=fn,
                                                vtrace_clip=clip)["default_policy"]
    np.testing.assert_array_equal(f32_bits(sb["vtrace_vs"]), f32_bits(keep["vtrace_vs"].reshape(-1)))
    np.testing.assert_array_equal(f32_bits(sb["vtrace_pg_advantages"]), f32_bits(keep["vtrace_pg_advantages"].reshape(-1)))
    with pytest.raises(ValueError, match="target_logp_fn"):
        _env().sample(T, policy=pol, explore=True, target_logp_fn=fn)                  # no critic
    with pytest.raises(ValueError, match="target_logp_fn"):
        _env().sample(T, policy=pol, value_fn=critic, target_logp_fn=fn)               # not exploring
    with pytest.raises(ValueError, match="target_logp_fn"):
        _env().sample(T, value_fn=critic, target_logp_fn=fn)                           # no device policy
    fsm = supply_chain_env(S, [6] * S, STEPS, B, seed=5, exogenous="device", fsm=True)
    fsm.reset()
    with pytest.raises(ValueError, match="target_logp_fn"):
        fsm.sample(T, value_fn=critic, target_logp_fn=fn)
