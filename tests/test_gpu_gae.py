"""phx_gae (include/phantom_amd_gae.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the numpy
restatement (tests/gae_ref.py) over column counts around the workgroup's and row counts around the kernel's chunk depth, the
optional planes, misaligned inputs, every refusal; then DeviceEnv.gae on a real rollout and PhantomEnv.sample(value_fn=...)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gae_ref
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import f32_bits, supply_chain_env
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_gae.hip")).read()
K = int(re.search(r"constexpr int GAE_K = (\d+);", SRC).group(1))                 # the kernel's chunk depth (rows)
WG = int(re.search(r"constexpr int GAE_LANES = (\d+);", SRC).group(1))            # the workgroup's columns
NS = (1, 3, 63, 64, 65, 549, WG - 2, WG + 2, 4 * WG + 2)                          # (549 = 61 * 9; 4 k + 2 around the workgroup's columns)
TS = (1, 2, K - 1, K, K + 1, 2 * K + 1, 100)
INPUTS = ("reward", "vf_pred", "vf_next", "terminated", "truncated")


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
    """one phx_gae call: device inputs (vf_next poisoned wherever the definition does not read it), fenced outputs"""

    def __init__(self, case, gamma, lam, nulls=(), offset=0):
        self.case, self.gamma, self.lam, self.nulls = case, gamma, lam, set(nulls)
        T, N = case["reward"].shape
        self.T, self.N = T, N
        self.dev = {}
        for k in INPUTS:
            if k in self.nulls:
                continue
            if k == "vf_next" and not offset:
                plane, whole = fenced((T, N), torch.float32, _dev())
                self.vf_next_whole = whole
                reads = torch.from_numpy(gae_ref.reads_vf_next(None if "terminated" in self.nulls else case["terminated"], case["truncated"])).to(_dev())
                plane[reads] = torch.from_numpy(case["vf_next"]).to(_dev())[reads]
                self.dev[k] = plane
            else:                                       # (a misaligned vf_next: poisoned the same way, inside a plain buffer)
                host = case[k]
                if k == "vf_next":
                    reads = gae_ref.reads_vf_next(None if "terminated" in self.nulls else case["terminated"], case["truncated"])
                    host = np.where(reads, host, np.frombuffer(b"\xa5" * 4, np.float32)[0])
                self.dev[k] = _offset(host, offset)
        self.before = {k: v.cpu().numpy().copy() for k, v in self.dev.items()}
        self.adv, self.adv_whole = fenced((T, N), torch.float32, _dev())
        self.vt, self.vt_whole = fenced((T, N), torch.float32, _dev())
        p = lambda k: self.dev[k].data_ptr() if k in self.dev else None
        self.io = _abi.PhxGaeIO(T=T, N=N, gamma=gamma, lambda_=lam, reward=p("reward"), vf_pred=p("vf_pred"), vf_next=p("vf_next"),
                                terminated=p("terminated"), truncated=p("truncated"), advantage=self.adv.data_ptr(),
                                value_target=None if "value_target" in self.nulls else self.vt.data_ptr())

    def launch(self):
        lib = _abi.load_library()
        return lib.phx_gae(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        ref = {k: (None if k in self.nulls else v) for k, v in self.case.items()}
        adv, vt = gae_ref.gae(ref["reward"], ref["truncated"], ref["vf_pred"], ref["vf_next"], ref["terminated"], self.gamma, self.lam)
        assert_fences(self.adv_whole, self.T, what + "advantage")
        assert_fences(self.vt_whole, self.T, what + "value_target")
        assert_written(self.adv, what + "advantage")
        np.testing.assert_array_equal(f32_bits(self.adv.cpu().numpy()), f32_bits(adv), err_msg=what + "advantage")
        if "value_target" in self.nulls:
            assert_poison(self.vt, what + "value_target (NULL: not written)")
        else:
            assert_written(self.vt, what + "value_target")
            np.testing.assert_array_equal(f32_bits(self.vt.cpu().numpy()), f32_bits(vt), err_msg=what + "value_target")
        for k, v in self.dev.items():                   # the inputs are byte-identical after the call
            np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), self.before[k].view(np.uint8), err_msg=what + k)
        if hasattr(self, "vf_next_whole"):
            assert_fences(self.vf_next_whole, self.T, what + "vf_next")

    def check_untouched(self, what):
        torch.cuda.synchronize()
        assert_poison(self.adv_whole, what + ": advantage")
        assert_poison(self.vt_whole, what + ": value_target")


def _run(T, N, gamma=0.99, lam=0.95, seed=0, **kw):
    call = Call(gae_ref.random_case(np.random.default_rng([seed, T, N]), T, N), gamma, lam, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    for T in TS:
        call = _run(T, N)
        tr, te = call.case["truncated"], call.case["terminated"]
        assert tr[0].any() and tr[T - 1].any() and (N < 3 or (te[T - 1].any() and (tr & te).any()))


def test_large_fragment_many_workgroups_and_chunks():
    _run(4 * K + 3, 61 * 9 * 5 + 1)                     # 43 workgroups, the last one with one live lane; 5 chunks


@pytest.mark.parametrize("null", ["vf_pred", "vf_next", "terminated", "value_target"])
def test_each_optional_plane_left_out(null):
    for T, N in ((K + 1, 65), (3, 549)):
        _run(T, N, nulls=(null,))
    _run(2 * K + 1, 67, nulls=("vf_pred", "vf_next", "terminated", "value_target"))


def test_inputs_four_bytes_past_a_16_byte_boundary():
    for T, N in ((2 * K + 1, 65), (K, 549), (5, 3)):    # (a slice [t0:t1] of a longer recording: sample()'s pieces)
        _run(T, N, offset=4)


@pytest.mark.parametrize("gamma,lam", [(1.0, 1.0), (0.99, 0.95), (0.0, 0.5)])
def test_gamma_lambda_corners(gamma, lam):
    call = _run(2 * K + 1, 130, gamma=gamma, lam=lam)
    if gamma == 0.0:
        want = (call.case["reward"].astype(np.float64) - call.case["vf_pred"].astype(np.float64)).astype(np.float32)
        np.testing.assert_array_equal(call.adv.cpu().numpy(), want)


def test_every_refusal_leaves_the_outputs_untouched():
    lib = _abi.load_library()
    case = gae_ref.random_case(np.random.default_rng(1), K + 1, 65)

    def refused(what, **patch):
        call = Call(case, 0.99, 0.95)
        for k, v in patch.items():
            setattr(call.io, k, v(getattr(call.io, k)) if callable(v) else v)
        assert call.launch() == -1, what                # PHX_EINVAL
        assert b"phx_gae" in lib.phx_last_error(), what
        call.check_untouched(what)

    for k in ("reward", "truncated", "advantage"):
        refused(f"{k} NULL", **{k: None})
    for k in ("reward", "vf_pred", "vf_next"):
        refused(f"{k} misaligned", **{k: lambda p: p + 2})
    for k in ("advantage", "value_target"):
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 4})
    refused("T = 0", T=0)
    refused("T < 0", T=-3)
    refused("N = 0", N=0)
    refused("N < 0", N=-1)
    for k in ("gamma", "lambda_"):
        for bad in (-0.01, 1.5, float("nan")):
            refused(f"{k} = {bad}", **{k: bad})
    refused("reserved0", reserved0=1)
    assert lib.phx_gae(None, None) == -1 and b"phx_gae" in lib.phx_last_error()


def test_last_kernel_names_the_kernel():
    _run(3, 7)
    assert _abi.load_library().phx_last_kernel() == b"phx_gae_kernel" == _abi.GAE_KERNEL.encode()


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(gae_ref.random_case(np.random.default_rng(11), 2 * K + 1, 549), 0.99, 0.95)
    b = Call(gae_ref.random_case(np.random.default_rng(12), K - 1, 130), 0.9, 1.0, nulls=("vf_next",))
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface: S = 9, B = 61, 7-step episodes, T = 20 (episode ends inside the fragment) --------------------------------------
S, B, STEPS, T = 9, 61, 7, 20


def _env(seed=5):
    env = supply_chain_env(S, [6] * S, STEPS, B, seed=seed, exogenous="device")
    env.reset()
    return env


def test_device_env_gae_on_a_real_rollout():
    env = _env()
    dev = env._device()
    tr = env.rollout(T)
    trunc = tr.truncations.cpu().numpy()
    assert trunc[STEPS - 1].all() and trunc[2 * STEPS - 1].all() and trunc.sum() == 2 * B * S      # rows 6 and 13 end episodes
    g = torch.Generator(device=dev.device).manual_seed(3)
    vf = torch.randn((T, B, S), generator=g, device=dev.device)
    vfn = torch.randn((T, B, S), generator=g, device=dev.device)
    adv, vt = dev.gae(tr.rewards, tr.truncations, vf, vfn, tr.terminations, gamma=0.99, lambda_=0.95)
    assert dev.last_kernel() == "phx_gae_kernel" and adv.shape == vt.shape == (T, B, S)
    want = gae_ref.gae(tr.rewards.cpu().numpy(), trunc, vf.cpu().numpy(), vfn.cpu().numpy(), tr.terminations.cpu().numpy(), 0.99, 0.95)
    np.testing.assert_array_equal(f32_bits(adv.cpu().numpy()), f32_bits(want[0]))
    np.testing.assert_array_equal(f32_bits(vt.cpu().numpy()), f32_bits(want[1]))
    out = (torch.empty_like(adv), torch.empty_like(vt))                    # caller-owned outputs, [T, N] planes, no critic
    flat = lambda x: x.reshape(T, B * S)
    got = dev.gae(flat(tr.rewards), flat(tr.truncations), gamma=0.9, out=(flat(out[0]), flat(out[1])))
    want = gae_ref.gae(flat(tr.rewards).cpu().numpy(), flat(tr.truncations).cpu().numpy(), gamma=0.9)
    np.testing.assert_array_equal(f32_bits(got[0].cpu().numpy()), f32_bits(want[0]))
    np.testing.assert_array_equal(f32_bits(got[1].cpu().numpy()), f32_bits(want[1]))
    assert got[0].data_ptr() == out[0].data_ptr()
    with pytest.raises(ValueError, match="vf_pred"):
        dev.gae(tr.rewards, tr.truncations, vf[:-1])
    with pytest.raises(ValueError, match="truncations"):
        dev.gae(tr.rewards, None)
    with pytest.raises(ValueError, match="gamma"):
        dev.gae(tr.rewards, tr.truncations, gamma=1.5)


def _policy():
    rng = np.random.default_rng(2)
    ws = [rng.normal(0, 0.7, (16, 3)).astype(np.float32), rng.normal(0, 0.3, (2, 16)).astype(np.float32)]
    bs = [rng.normal(0, 0.3, (16,)).astype(np.float32), np.array([0.1, -0.5], np.float32)]
    return ph.MLPPolicy(ws, bs, activation="relu", out_scale=50.0, out_bias=50.0, out_lo=0.0, out_hi=100.0)


def test_sample_with_a_critic():
    env = _env()
    device = env._device().device
    torch.manual_seed(0)
    critic = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)).to(device)
    pol = _policy()
    batch = env.sample(T, policy=pol, explore=True, value_fn=critic, gamma=0.99, lambda_=0.95)
    assert env._device().last_kernel() == "phx_gae_kernel"
    for name in ("vf_preds", "advantages", "value_targets"):
        x = getattr(batch, name)
        assert x.shape == (B, S, T) and x.dtype == np.float32
    keep = {k: np.array(getattr(batch, k)) for k in ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "raw_actions",
                                                     "action_logp", "dist_inputs", "t", "eps_id", "vf_preds", "advantages", "value_targets")}
    tm = lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0))            # [B, S, T, ..] -> [T, B, S, ..]
    with torch.no_grad():                                               # the critic on the same rows in the same order
        v = lambda a: critic(torch.from_numpy(a).to(device).reshape(-1, 3)).reshape(a.shape[:-1]).cpu().numpy()
        vf = v(tm(keep["obs"]))
        cut = tm(keep["truncateds"]) | tm(keep["terminateds"])
        ends = sorted(set(np.flatnonzero(cut.reshape(T, -1).any(axis=1)).tolist()) | {T - 1})
        assert ends == [STEPS - 1, 2 * STEPS - 1, T - 1]
        vfn = np.full((T, B, S), np.nan, np.float32)                    # (unread elements may hold anything)
        vfn[ends] = v(tm(keep["new_obs"])[ends])
    np.testing.assert_array_equal(f32_bits(tm(keep["vf_preds"])), f32_bits(vf))
    adv, vt = gae_ref.gae(tm(keep["rewards"]), tm(keep["truncateds"]), vf, vfn, tm(keep["terminateds"]), 0.99, 0.95)
    np.testing.assert_array_equal(f32_bits(tm(keep["advantages"])), f32_bits(adv))
    np.testing.assert_array_equal(f32_bits(tm(keep["value_targets"])), f32_bits(vt))
    cols = batch.to_sample_batches()["default_policy"]
    for name in ("vf_preds", "advantages", "value_targets"):
        np.testing.assert_array_equal(cols[name], keep[name].reshape(-1))
        assert cols[name].shape == cols["rewards"].shape == (B * S * T,)
    # without value_fn: the same batch, bit for bit, and no critic columns (same seed, fresh env)
    env2 = _env()
    plain = env2.sample(T, policy=pol, explore=True)
    assert plain.vf_preds is None and plain.advantages is None and plain.value_targets is None
    assert "advantages" not in plain.to_sample_batches()["default_policy"]
    for k in ("obs", "new_obs", "actions", "rewards", "raw_actions", "action_logp", "dist_inputs"):
        np.testing.assert_array_equal(f32_bits(getattr(plain, k)), f32_bits(keep[k]), err_msg=k)
    for k in ("terminateds", "truncateds", "t", "eps_id"):
        np.testing.assert_array_equal(getattr(plain, k), keep[k], err_msg=k)
    sb = ph.rllib.BatchedBaseEnv(_env()).sample(T, policy=pol, explore=True, value_fn=critic, gamma=0.99, lambda_=0.95)["default_policy"]
    np.testing.assert_array_equal(f32_bits(sb["advantages"]), f32_bits(keep["advantages"].reshape(-1)))
    with pytest.raises(ValueError, match="value_fn"):
        _env().sample(T, value_fn=lambda x: x)
