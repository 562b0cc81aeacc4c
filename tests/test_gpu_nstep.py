"""phx_nstep (include/phantom_amd_nstep.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the numpy
restatement (tests/nstep_ref.py) over row counts around the successor scan's chunk depth, column counts around the workgroups', every
n, observation width and gamma of the issue, every combination of the optional planes, misaligned inputs, NaN in what the call does
not read, columns that never or always act, subnormal discounts, every refusal, the kernel names; then DeviceEnv.nstep on real plain,
FSM and Stackelberg rollouts whose episodes end inside the fragment, and PhantomEnv.sample(n_step=) against a twin env sampled without
the keyword, compacted and not."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compact_ref as cr
import nstep_ref as ns
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import f32_bits, market_env, supply_chain_env
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_nstep.hip")).read()
K = int(re.search(r"constexpr int NS_K = (\d+);", SRC).group(1))                  # the successor scan's chunk depth (rows)
WG = int(re.search(r"constexpr int NS_LANES = (\d+);", SRC).group(1))             # its workgroup (columns)
TS = (1, 2, K - 1, K, K + 1, 2 * K + 1, 40)
NS = (1, 63, 64, 65, 257)
STEPS_N = (1, 2, 3, 5, 64)
DS = (1, 3, 5, None)
GAMMAS = (0.0, 0.5, 0.99, 1.0)
INPUTS = ("reward", "truncated", "terminated", "acted", "next_row", "next_obs")
OPTIONAL = ("terminated", "acted", "next_row")
OUT_DTYPES = dict(succ_row=torch.int32, nstep_reward=torch.float32, nstep_discount=torch.float32, nstep_last=torch.int32,
                  nstep_terminated=torch.uint8, nstep_truncated=torch.uint8, nstep_next_row=torch.int32, nstep_next_obs=torch.float32)
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


def _bits(a):
    return f32_bits(a) if a.dtype == np.float32 else a


class Call:
    """one phx_nstep call: device inputs (reward and next_obs NaN wherever no result depends on them), every output fenced.  `case`
    holds next_obs [T, N, D] for a call with nstep_next_obs; `byte_offset` / `word_offset`: bytes past a 16-byte boundary the u8 and
    the 4-byte inputs start at.  succ_row is always passed: without `acted` it must stay untouched"""

    def __init__(self, case, n, gamma, nulls=(), byte_offset=0, word_offset=0, poison=True):
        self.case, self.nulls, self.n, self.gamma = case, set(nulls), n, gamma
        T, N = case["reward"].shape
        self.T, self.N, self.D = T, N, (case["next_obs"].shape[-1] if "next_obs" in case else 0)
        self.ref = {k: (None if k in self.nulls else case.get(k)) for k in INPUTS}
        self.want = ns.nstep(n=n, gamma=gamma, **self.ref)
        host = dict(self.ref)
        if poison:
            rd = ns.reads(n=n, gamma=gamma, **{k: self.ref[k] for k in INPUTS[:5]})
            host["reward"] = np.where(rd["reward"], case["reward"], NAN)
            if self.D:
                host["next_obs"] = np.where(rd["next_obs"][..., None], case["next_obs"], NAN)
        self.dev = {k: _offset(v, byte_offset if v.dtype == np.uint8 else word_offset) for k, v in host.items() if v is not None}
        self.before = {k: v.cpu().numpy().copy() for k, v in self.dev.items()}
        self.out, self.whole = {}, {}
        for k, dtype in OUT_DTYPES.items():
            self.out[k], self.whole[k] = fenced((T, N, self.D) if k == "nstep_next_obs" else (T, N), dtype, _dev()) if (k != "nstep_next_obs" or self.D) else (None, None)
        p = lambda k: self.dev[k].data_ptr() if k in self.dev else None
        o = lambda k: self.out[k].data_ptr() if self.out[k] is not None else None
        self.io = _abi.PhxNstepIO(T=T, D=self.D, N=N, n=n, gamma=gamma, **{k: p(k) for k in INPUTS}, **{k: o(k) for k in OUT_DTYPES})

    def launch(self):
        return _abi.load_library().phx_nstep(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        for k in OUT_DTYPES:
            if self.out[k] is None:
                continue
            assert_fences(self.whole[k], self.T, what + k)
            if k == "succ_row" and "acted" in self.nulls:
                assert_poison(self.whole[k], what + "succ_row without acted")
                continue
            assert_written(self.out[k], what + k)
            np.testing.assert_array_equal(_bits(self.out[k].cpu().numpy()), _bits(self.want[k]), err_msg=what + k)
        for k, v in self.dev.items():                   # the inputs are byte-identical after the call
            np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), self.before[k].view(np.uint8), err_msg=what + k)

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k in OUT_DTYPES:
            if self.whole[k] is not None:
                assert_poison(self.whole[k], f"{what}: {k}")


def _case(T, N, D=None, seed=0):
    return ns.random_case(np.random.default_rng([seed, T, N]), T, N, D=D)


def _run(T, N, n=3, gamma=0.99, D=None, seed=0, **kw):
    call = Call(_case(T, N, D, seed), n, gamma, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} n={n} gamma={gamma} D={D} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    """every T with every n; D and gamma cycle so that each value meets each T and each n"""
    for i, T in enumerate(TS):
        for j, n in enumerate(STEPS_N):
            _run(T, N, n, GAMMAS[(i + j) % 4], DS[(i + 2 * j) % 4])


def test_every_n_gamma_and_width_together():
    T, N = 2 * K + 1, 65
    for n, gamma, D in itertools.product(STEPS_N, GAMMAS, DS):
        _run(T, N, n, gamma, D)
    case = _case(T, N)                                  # what these cases hold (tests/test_nstep_cpu.py has the full condition)
    act = case["acted"] != 0
    assert not act[:, 10].any() and act[:, 11].all() and act[:, 12].all()      # a column that never acts, columns that act in every row
    m, stop = ns.stats(n=3, gamma=0.99, **{k: case[k] for k in INPUTS[:5]})
    assert {ns.STOPS[i] for i in np.unique(stop[act])} == set(ns.STOPS) and (m >= 2).sum() * 4 >= act.sum()


def test_many_workgroups_and_chunks():
    _run(4 * K + 3, 61 * 9 * 5 + 1, 5, 0.97, 3)         # 43 workgroups of the scan and 11 of the fold, the last ones with one live lane


@pytest.mark.parametrize("gather", [False, True])
def test_every_combination_of_the_optional_planes(gather):
    for r in range(len(OPTIONAL) + 1):
        for nulls in itertools.combinations(OPTIONAL, r):
            for n in (1, 4):
                _run(2 * K + 1, 65, n, 0.9, 3 if gather else None, nulls=nulls)


@pytest.mark.parametrize("byte_offset,word_offset", [(1, 4), (3, 12), (7, 8)])
def test_inputs_that_are_row_slices_of_a_longer_recording(byte_offset, word_offset):
    for T, N in ((2 * K + 1, 65), (K, 257), (5, 3)):    # (a slice [t0:t1] of a recording whose rows are no multiple of 16 bytes)
        _run(T, N, 3, 0.99, 3, byte_offset=byte_offset, word_offset=word_offset)
        _run(T, N, 4, 0.5, None, byte_offset=byte_offset, word_offset=word_offset)


def test_nan_in_the_unread_elements_and_any_bit_pattern_in_the_copied_ones():
    T, N, D = 2 * K + 1, 130, 3
    case = _case(T, N, D, seed=4)
    rng = np.random.default_rng(4)
    w = rng.integers(0, 2 ** 32, (T, N, D), dtype=np.uint64).astype(np.uint32)      # NaN payloads, infinities, -0.0, denormals: words are copied
    w[w == 0xA5A5A5A5] = 0                              # (the fence's poison word stays the sign of an unwritten one)
    w[:, 11, 0] = 0x80000000; w[:, 11, 1] = 0x7fc00001; w[:, 11, 2] = 0xff800001      # (column 11 acts in every row)
    case["next_obs"] = w.view(np.float32)
    call = Call(case, 3, 0.99)                          # (poison=True: NaN wherever ns.reads says no result depends on the element)
    assert np.isnan(call.before["reward"]).any() and (~np.isnan(call.before["reward"])).any()
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check("arbitrary words: ")
    got = f32_bits(call.out["nstep_next_obs"].cpu().numpy())
    assert (got == 0x80000000).any() and (got == 0x7fc00001).any() and (got == 0xff800001).any()
    assert not np.isnan(call.out["nstep_reward"].cpu().numpy()).any()


def test_reduction_n_equals_one_is_the_inputs_bit_for_bit():
    T, N, D = 2 * K + 1, 257, 3
    case = _case(T, N, D, seed=21)
    case["reward"][0, :8] = np.float32(-0.0); case["acted"][0, :8] = 1
    call = Call(case, 1, 0.37, poison=False)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check()
    d, o = call.dev, call.out
    act = d["acted"] != 0
    rows = torch.arange(T, device=_dev(), dtype=torch.int32)[:, None].expand(T, N)
    eq = lambda a, b: bool((a[act] == b[act]).all())
    assert eq(o["nstep_reward"].view(torch.int32), d["reward"].view(torch.int32)) and bool((o["nstep_reward"][0, :8].view(torch.int32) == -2 ** 31).all())
    assert bool((o["nstep_discount"][act] == torch.tensor(0.37, dtype=torch.float32)).all())
    assert eq(o["nstep_last"], rows) and eq(o["nstep_next_row"], d["next_row"])
    assert eq(o["nstep_terminated"], (d["terminated"] != 0).to(torch.uint8))
    assert eq(o["nstep_truncated"], ((d["terminated"] == 0) & (d["truncated"] != 0)).to(torch.uint8))
    assert bool((o["nstep_next_obs"].view(torch.int32)[act] == d["next_obs"].view(torch.int32)[act]).all())
    assert bool(((d["terminated"] != 0) & (d["truncated"] != 0) & act).any())


def test_a_subnormal_discount_is_kept():
    """the header's (d): gamma = 1e-10 makes p subnormal at m = 4 (1e-40) and 0 at m = 5; the kernels keep it as IEEE 754 does"""
    T, N = 7, 5
    reward = np.zeros((T, N), np.float32)
    reward[4] = np.float32(1e38)
    reward[:, 1] = np.float32(1e-42)                    # (subnormal rewards as well)
    case = dict(reward=reward, truncated=np.zeros((T, N), np.uint8))
    for n in (4, 5, 6):
        call = Call(case, n, 1e-10, nulls=OPTIONAL, poison=False)
        assert call.launch() == 0, _abi.load_library().phx_last_error()
        call.check(f"n={n}: ")
        p = call.out["nstep_discount"][0, 0].item()
        assert (0.0 < p < 1.2e-38) if n == 4 else p == 0.0
    got = call.out["nstep_reward"].cpu().numpy()
    assert got[0, 0] > 0.009 and got[0, 1] > 0.0        # row 0 folds p4 * 1e38 with the subnormal p4 = 1e-40


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _abi.load_library()
    call = Call(_case(K + 1, 65, 3, seed=1), 3, 0.99)
    good = {n: getattr(call.io, n) for n, _ in call.io._fields_}

    def refused(what, **patch):
        for n, v in good.items():
            setattr(call.io, n, v)
        for k, v in patch.items():
            setattr(call.io, k, v(good[k]) if callable(v) else v)
        assert call.launch() == -1, what                # PHX_EINVAL
        assert b"phx_nstep" in lib.phx_last_error(), what
        call.check_untouched(what)

    for k in ("reward", "truncated", "nstep_reward", "nstep_discount", "nstep_last", "nstep_terminated", "nstep_truncated", "nstep_next_row"):
        refused(f"{k} NULL", **{k: None})
    refused("acted without succ_row", succ_row=None)
    refused("nstep_next_obs without next_obs", next_obs=None)
    for bad in (0, -1, 65, 1 << 20):
        refused(f"D = {bad}", D=bad)
    for bad in (0, -1, 65, 1 << 20):
        refused(f"n = {bad}", n=bad)
    for bad in (-0.0001, 1.0001, float("nan"), float("inf"), -float("inf")):
        refused(f"gamma = {bad}", gamma=bad)
    for k in ("reward", "next_row", "next_obs"):
        refused(f"{k} misaligned", **{k: lambda p: p + 2})
    for k in OUT_DTYPES:
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 4})
    refused("T = 0", T=0)
    refused("T < 0", T=-3)
    refused("N = 0", N=0)
    refused("N < 0", N=-1)
    refused("N beyond the scan's grid", N=WG * 0x7fffffff + 1)
    refused("N beyond the gather's grid", N=WG * 0x7fffffff, D=64)
    assert lib.phx_nstep(None, None) == -1 and b"phx_nstep" in lib.phx_last_error()
    for n, v in good.items():                           # and the same buffers receive a good call
        setattr(call.io, n, v)
    assert call.launch() == 0, lib.phx_last_error()
    call.check("after the refusals: ")


def test_last_kernel_names_the_kernels_launched():
    lib = _abi.load_library()
    s, f, g = _abi.NSTEP_SUCC_KERNEL, _abi.NSTEP_FOLD_KERNEL, _abi.NSTEP_GATHER_KERNEL
    _run(3, 7)
    assert lib.phx_last_kernel() == b"phx_nstep_succ_kernel+phx_nstep_fold_kernel" == f"{s}+{f}".encode()
    _run(3, 7, D=2)
    assert lib.phx_last_kernel() == b"phx_nstep_succ_kernel+phx_nstep_fold_kernel+phx_nstep_gather_kernel" == f"{s}+{f}+{g}".encode()
    _run(3, 7, nulls=("acted",))
    assert lib.phx_last_kernel() == b"phx_nstep_fold_kernel" == f.encode()
    _run(3, 7, D=2, nulls=("acted",))
    assert lib.phx_last_kernel() == b"phx_nstep_fold_kernel+phx_nstep_gather_kernel" == f"{f}+{g}".encode()


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(_case(2 * K + 1, 257, 3, seed=11), 5, 0.99)
    b = Call(_case(K - 1, 130, 5, seed=12), 2, 0.5, nulls=("acted",))
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
# 10-step episodes, 25-row fragments: two episodes end inside the fragment.  The shops of the FSM chain act in every other step and
# the episode ends in a step they do not act in
T = 25
FIELDS = ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "t", "eps_id", "obs_valid", "new_obs_valid", "reward_valid",
          "stage", "vf_preds", "advantages", "value_targets", "trajectory_rewards", "trajectory_next_row", "trajectory_new_obs",
          "trajectory_terminateds", "trajectory_truncateds", "raw_actions", "action_logp", "dist_inputs", "target_logp", "vtrace_vs",
          "vtrace_pg_advantages")
NSTEP_FIELDS = ("nstep_rewards", "nstep_discounts", "nstep_new_obs", "nstep_terminateds", "nstep_truncateds")


def _plain_env(seed=5):
    env = supply_chain_env(4, [3] * 4, 10, 7, seed=seed, exogenous="device")
    env.reset()
    return env


def _fsm_env(seed=5):
    env = supply_chain_env(3, [2] * 3, 10, 6, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


def _stk_env(seed=5):
    env = market_env(2, 3, 2, 6, 7, seed=seed, exogenous="device")
    env.reset()
    return env


def _critic(x):
    return 0.5 * x[:, 0] - 0.25 * torch.tanh(x[:, 1]) + 0.125 * x[:, -1] * x[:, -1] + 0.75


def _tm(a):
    return np.ascontiguousarray(np.moveaxis(a, 2, 0))   # [B, S, T, ..] -> [T, B, S, ..]


def _transitions(batch):
    """the time-major inputs of the n-step call from a batch sampled WITHOUT the keyword: its one-step transition fields"""
    if batch.obs_valid is None:
        return dict(reward=_tm(batch.rewards), truncated=_tm(batch.truncateds).astype(np.uint8), terminated=_tm(batch.terminateds).astype(np.uint8),
                    acted=None, next_row=None, next_obs=_tm(batch.new_obs))
    return dict(reward=_tm(batch.trajectory_rewards), truncated=_tm(batch.trajectory_truncateds).astype(np.uint8),
                terminated=_tm(batch.trajectory_terminateds).astype(np.uint8), acted=_tm(batch.obs_valid),
                next_row=_tm(batch.trajectory_next_row), next_obs=_tm(batch.trajectory_new_obs))


@pytest.mark.parametrize("make", [_plain_env, _fsm_env, _stk_env])
def test_device_env_nstep_on_a_real_rollout(make):
    env = make()
    batch = env.sample(T)
    assert len(batch.episodes()) >= 3                   # episodes end inside the fragment
    p = _transitions(batch)
    dev = env._device()
    to = lambda a: None if a is None else torch.from_numpy(a).to(dev.device)
    args = tuple(to(p[k]) for k in INPUTS)
    got = dev.nstep(*args, n=3, gamma=0.9)
    masked = p["acted"] is not None
    assert dev.last_kernel() == ("phx_nstep_succ_kernel+" if masked else "") + "phx_nstep_fold_kernel+phx_nstep_gather_kernel"
    want = ns.nstep(n=3, gamma=0.9, **p)
    m, stop = ns.stats(n=3, gamma=0.9, **{k: p[k] for k in INPUTS[:5]})
    assert (m == 3).any() and (m == 2).any() and ((m == 1) & (stop >= 0)).any()      # chains of every length: cut by the episodes' ends
    if masked:
        assert 0.2 < (p["acted"] != 0).mean() < 0.8
    assert [g.dtype for g in got] == [OUT_DTYPES[k] for k in ns.OUTPUTS]
    for g, name in zip(got, ns.OUTPUTS):
        assert tuple(g.shape) == want[name].shape
        np.testing.assert_array_equal(_bits(g.cpu().numpy()), _bits(want[name]), err_msg=name)
    # without the observations: no gather, the same six planes, [T, N] views, n = 1
    flat = lambda x: None if x is None else x.reshape(T, -1)
    six = dev.nstep(*(flat(x) for x in args[:5]), n=1, gamma=1.0)
    assert six[6] is None and "gather" not in dev.last_kernel()
    want1 = ns.nstep(n=1, gamma=1.0, **{k: p[k] for k in INPUTS[:5]})
    for g, name in zip(six[:6], ns.OUTPUTS):
        np.testing.assert_array_equal(_bits(g.cpu().numpy()), _bits(want1[name].reshape(T, -1)), err_msg=name)
    # refusals at this level come before any launch and leave caller-owned outputs untouched
    shape = tuple(args[0].shape)
    D = args[5].shape[-1]
    outs = [fenced(shape + (D,) if k == "nstep_next_obs" else shape, OUT_DTYPES[k], dev.device) for k in ns.OUTPUTS + ("succ_row",)]
    out = tuple(o[0] for o in outs)
    bad_args = [("rewards", 0, args[0].double()), ("truncations", 1, args[1].to(torch.int32)), ("terminations", 2, args[2][:-1]),
                ("next_obs", 5, args[5][..., :-1].contiguous().double()), ("rewards", 0, args[0].cpu())]
    if masked:
        bad_args += [("acted", 3, args[3].to(torch.float32)), ("next_row", 4, args[4].to(torch.int64))]
    for name, i, bad in bad_args:
        a = list(args); a[i] = bad
        with pytest.raises(ValueError, match=name):
            dev.nstep(*a, n=3, gamma=0.9, out=out)
    for kw in (dict(n=0), dict(n=65), dict(n=2.0), dict(n=True), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan"))):
        with pytest.raises(ValueError, match="n =|gamma"):
            dev.nstep(*args, **{**dict(n=3, gamma=0.9), **kw}, out=out)
    with pytest.raises(ValueError, match=r"out\[6\]"):
        dev.nstep(*args[:5], n=3, gamma=0.9, out=out)   # a next_obs output without next_obs
    for i in range(8):                                  # a misaligned out[i]
        raw = torch.full((out[i].numel() * out[i].element_size() + 16,), 0xA5, dtype=torch.uint8, device=dev.device)
        off = raw[4:4 + out[i].numel() * out[i].element_size()].view(out[i].dtype).view(out[i].shape)
        o = list(out); o[i] = off
        with pytest.raises(ValueError, match=rf"out\[{i}\]"):
            dev.nstep(*args, n=3, gamma=0.9, out=tuple(o))
        assert_poison(raw, f"a refused call with out[{i}] misaligned")
    torch.cuda.synchronize()
    for _, whole in outs:
        assert_poison(whole, "a refused DeviceEnv.nstep call")
    res = dev.nstep(*args, n=3, gamma=0.9, out=out)     # and a good call fills them, the caller's scratch included
    assert len(res) == 7 and all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
    for (plane, whole), name in zip(outs, ns.OUTPUTS + ("succ_row",)):
        assert_fences(whole, T, name)
        if name == "succ_row" and not masked:
            assert_poison(whole, "succ_row without acted")
            continue
        assert_written(plane, name)
        np.testing.assert_array_equal(_bits(plane.cpu().numpy()), _bits(want[name]), err_msg=name)


def _same_fields(got, want, names):
    for k in names:
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None), k
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, k
            assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), k


def _check_nstep_fields(batch, twin_batch, n, gamma):
    """every field a batch had before is bit-equal to the twin's; the five new ones are the restatement on the twin's one-step fields"""
    _same_fields(batch, twin_batch, FIELDS)
    assert all(getattr(twin_batch, k) is None for k in NSTEP_FIELDS)
    want = ns.nstep(n=n, gamma=gamma, **_transitions(twin_batch))
    for field, name, dtype in zip(NSTEP_FIELDS, ("nstep_reward", "nstep_discount", "nstep_next_obs", "nstep_terminated", "nstep_truncated"),
                                  (np.float32, np.float32, np.float32, bool, bool)):
        g = getattr(batch, field)
        assert g.dtype == dtype and g.shape == getattr(batch, "new_obs" if field == "nstep_new_obs" else "rewards").shape, field
        np.testing.assert_array_equal(_bits(_tm(g)) if dtype != bool else _tm(g), _bits(want[name]) if dtype != bool else want[name] != 0, err_msg=field)
    cols, old = batch.to_sample_batches()["default_policy"], twin_batch.to_sample_batches()["default_policy"]
    assert set(cols) == set(old) | set(NSTEP_FIELDS)
    for k, w in old.items():                            # the one-step columns stay as they are
        assert cols[k].dtype == w.dtype and cols[k].tobytes() == w.tobytes(), k
    keep = np.ones(batch.rewards.shape, bool) if batch.obs_valid is None else batch.obs_valid != 0
    for field in NSTEP_FIELDS:
        np.testing.assert_array_equal(cols[field], getattr(batch, field)[keep], err_msg=field)
    return want


@pytest.mark.parametrize("with_critic", [False, True])
@pytest.mark.parametrize("make", [_plain_env, _fsm_env, _stk_env])
def test_sample_with_n_step_against_a_twin_sampled_without(make, with_critic):
    env, twin = make(), make()
    kw = dict(value_fn=_critic, gamma=0.97, lambda_=0.95) if with_critic else dict(gamma=0.97)
    batch = env.sample(T, n_step=3, **kw)
    assert env._device().last_kernel().endswith("phx_nstep_fold_kernel+phx_nstep_gather_kernel")      # (the thread's last call: the fold comes last)
    old = twin.sample(T, **kw)
    assert "nstep" not in twin._device().last_kernel()
    want = _check_nstep_fields(batch, old, 3, 0.97)
    act = np.ones((T,) + batch.rewards.shape[:2], bool) if batch.obs_valid is None else _tm(batch.obs_valid) != 0
    disc = want["nstep_discount"][act]
    g = np.float32(0.97)
    assert {float(x) for x in np.unique(disc)} == {float(g), float(g * g), float(np.float32(g * g) * g)}      # chains of 1, 2 and 3 transitions
    sb = ph.rllib.BatchedBaseEnv(make()).sample(T, n_step=3, **kw)["default_policy"]      # the same columns through the RLlib adapter
    cols = batch.to_sample_batches()["default_policy"]
    assert set(sb) == set(cols)
    for name in NSTEP_FIELDS + ("rewards", "new_obs"):
        np.testing.assert_array_equal(sb[name], cols[name], err_msg=name)
    again, old2 = env.sample(7, n_step=2, **kw), twin.sample(7, **kw)      # a second call continues where the first one stopped
    _check_nstep_fields(again, old2, 2, 0.97)
    one, old3 = env.sample(9, n_step=1, **kw), twin.sample(9, **kw)         # n_step = 1: the one-step transitions themselves
    _check_nstep_fields(one, old3, 1, 0.97)
    p = _transitions(old3)
    rows = act[:1].repeat(9, axis=0) if old3.obs_valid is None else _tm(old3.obs_valid) != 0
    np.testing.assert_array_equal(f32_bits(_tm(one.nstep_rewards))[rows], f32_bits(p["reward"])[rows])
    np.testing.assert_array_equal(f32_bits(_tm(one.nstep_new_obs))[rows], f32_bits(p["next_obs"])[rows])
    for bad in (0, -1, 65, 2.5, True, "3"):
        with pytest.raises(ValueError, match="n_step"):
            env.sample(T, n_step=bad)
    with pytest.raises(ValueError, match="gamma"):
        env.sample(T, n_step=2, gamma=1.5)


def test_sample_with_n_step_and_an_exploring_device_policy():
    rng = np.random.default_rng(2)
    ws = [rng.normal(0, 0.7, (16, 3)).astype(np.float32), rng.normal(0, 0.3, (2, 16)).astype(np.float32)]
    bs = [rng.normal(0, 0.3, (16,)).astype(np.float32), np.array([0.1, -0.5], np.float32)]
    pol = ph.MLPPolicy(ws, bs, activation="relu", out_scale=50.0, out_bias=50.0, out_lo=0.0, out_hi=100.0)
    env, twin = _plain_env(), _plain_env()             # (the exploration noise comes from the env's own generator: same seed, same draws)
    kw = dict(policy=pol, explore=True, value_fn=_critic, gamma=0.9, lambda_=0.95)
    batch, old = env.sample(T, n_step=5, **kw), twin.sample(T, **kw)
    assert batch.raw_actions is not None and batch.advantages is not None
    _check_nstep_fields(batch, old, 5, 0.9)


@pytest.mark.parametrize("with_critic", [False, True])
@pytest.mark.parametrize("make", [_fsm_env, _stk_env])
def test_compact_gives_the_same_sample_batches(make, with_critic):
    kw = dict(value_fn=_critic, gamma=0.97, lambda_=0.95) if with_critic else dict(gamma=0.97)
    a, b = make(), make()
    frag, batch = a.sample(T, n_step=3, compact=True, **kw), b.sample(T, n_step=3, **kw)
    assert isinstance(frag, ph.rollout.CompactFragment) and set(NSTEP_FIELDS) <= set(frag.columns)
    assert frag.columns["nstep_terminateds"].dtype == frag.columns["nstep_truncateds"].dtype == np.bool_
    cr.assert_same_batches(frag.to_sample_batches(), batch.to_sample_batches(), "one policy: ")
    cr.assert_same_batches(frag.to_sample_batches(lambda aid: str(aid)), batch.to_sample_batches(lambda aid: str(aid)), "a policy per agent: ")
    assert set(NSTEP_FIELDS) <= set(batch.to_sample_batches()["default_policy"])
    plain = a.sample(5, compact=True, **kw)              # without the keyword: the columns it had
    assert not (set(NSTEP_FIELDS) & set(plain.columns))


def test_sample_without_the_keyword_has_todays_key_set():
    base = {"obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "eps_id", "agent_index", "t", "env_id"}
    env = _plain_env()
    batch = env.sample(T)
    assert all(getattr(batch, k) is None for k in NSTEP_FIELDS)
    assert set(batch.to_sample_batches()["default_policy"]) == base
    assert "nstep" not in env._device().last_kernel()
    cols = _plain_env().sample(T, value_fn=_critic).to_sample_batches()["default_policy"]
    assert set(cols) == base | {"vf_preds", "advantages", "value_targets"}
    fsm = _fsm_env()
    fb = fsm.sample(T)
    assert all(getattr(fb, k) is None for k in NSTEP_FIELDS) and fsm._device().last_kernel() == "phx_gae_masked_kernel"
    assert set(fb.to_sample_batches()["default_policy"]) == base | {"trajectory_next_row"}
