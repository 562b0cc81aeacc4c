"""phx_traj_next (include/phantom_amd_traj.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the
numpy restatement (tests/traj_next_ref.py) over row counts around the kernel's chunk depth, column counts around the workgroup's and
three observation widths, every combination of the optional planes, misaligned inputs, NaN in what the call does not read, the
reduction, every refusal; then DeviceEnv.traj_next on real FSM and Stackelberg rollouts and PhantomEnv.sample()'s four trajectory
fields against a twin env's rollout() planes -- on an FSM env whose episodes end in a step the shops do not act in."""
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
import traj_next_ref as tn
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import f32_bits, market_env, supply_chain_env
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_traj_next.hip")).read()
K = int(re.search(r"constexpr int TN_K = (\d+);", SRC).group(1))                  # the scan's chunk depth (rows)
WG = int(re.search(r"constexpr int TN_LANES = (\d+);", SRC).group(1))             # the scan's workgroup (columns)
TS = (1, K - 1, K, K + 1, 2 * K, 2 * K + 1, 40)
NS = (1, 63, 64, 65, 257)
DS = (1, 3, 5)
FLAGS = ("truncated", "terminated", "acted", "new_obs_valid")
OPTIONAL = FLAGS[1:]
OUTPUTS = ("next_row", "next_terminated", "next_truncated", "next_obs")
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
    """one phx_traj_next call: device inputs (obs / new_obs NaN wherever no result depends on them), fenced outputs.  `case` holds obs
    and new_obs [T, N, D] for a call with next_obs; `flag_offset` / `obs_offset`: bytes past a 16-byte boundary the inputs start at"""

    def __init__(self, case, nulls=(), flag_offset=0, obs_offset=0, poison=True):
        self.case, self.nulls = case, set(nulls)
        T, N = case["truncated"].shape
        self.T, self.N, self.D = T, N, (case["obs"].shape[-1] if "obs" in case else 0)
        self.ref = {k: (None if k in self.nulls else case.get(k)) for k in FLAGS + ("obs", "new_obs")}
        self.want = dict(zip(OUTPUTS, tn.traj_next(**self.ref)))
        rd = tn.reads(self.want["next_row"], self.ref["acted"])
        self.dev = {}
        for k in FLAGS:
            if k not in self.nulls:
                self.dev[k] = _offset(case[k], flag_offset)
        for k in ("obs", "new_obs"):
            if self.D:
                self.dev[k] = _offset(np.where(rd[k][..., None], case[k], NAN) if poison else case[k], obs_offset)
        self.before = {k: v.cpu().numpy().copy() for k, v in self.dev.items()}
        self.out, self.whole = {}, {}
        for k, dtype in zip(OUTPUTS, (torch.int32, torch.uint8, torch.uint8, torch.float32)):
            self.out[k], self.whole[k] = fenced((T, N, self.D) if k == "next_obs" else (T, N), dtype, _dev()) if (k != "next_obs" or self.D) else (None, None)
        p = lambda k: self.dev[k].data_ptr() if k in self.dev else None
        o = lambda k: self.out[k].data_ptr() if self.out[k] is not None else None
        self.io = _abi.PhxTrajNextIO(T=T, D=self.D, N=N, truncated=p("truncated"), terminated=p("terminated"), acted=p("acted"),
                                     new_obs_valid=p("new_obs_valid"), obs=p("obs"), new_obs=p("new_obs"), next_row=o("next_row"),
                                     next_terminated=o("next_terminated"), next_truncated=o("next_truncated"), next_obs=o("next_obs"))

    def launch(self):
        return _abi.load_library().phx_traj_next(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        for k in OUTPUTS:
            if self.out[k] is None:
                continue
            assert_fences(self.whole[k], self.T, what + k)
            assert_written(self.out[k], what + k)
            got, want = self.out[k].cpu().numpy(), self.want[k]
            np.testing.assert_array_equal(f32_bits(got) if k == "next_obs" else got, f32_bits(want) if k == "next_obs" else want, err_msg=what + k)
        for k, v in self.dev.items():                   # the inputs are byte-identical after the call
            np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), self.before[k].view(np.uint8), err_msg=what + k)

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k in OUTPUTS:
            if self.whole[k] is not None:
                assert_poison(self.whole[k], f"{what}: {k}")


def _case(T, N, D=None, seed=0):
    return tn.random_case(np.random.default_rng([seed, T, N]), T, N, D=D)


def _run(T, N, D=None, seed=0, **kw):
    call = Call(_case(T, N, D, seed), **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} D={D} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    for T in TS:
        for D in DS:
            call = _run(T, N, D)
        if N >= 63 and T >= 15:                         # (every class of row is there: tests/test_traj_next_cpu.py)
            assert all(tn.features(call.case).values())


def test_many_workgroups_and_chunks():
    _run(4 * K + 3, 61 * 9 * 5 + 1, 3)                  # 43 workgroups of the scan, the last one with one live lane; 5 chunks


@pytest.mark.parametrize("gather", [False, True])
def test_every_combination_of_the_optional_planes(gather):
    for r in range(len(OPTIONAL) + 1):
        for nulls in itertools.combinations(OPTIONAL, r):
            _run(2 * K + 1, 65, 3 if gather else None, nulls=nulls)


@pytest.mark.parametrize("flag_offset,obs_offset", [(1, 4), (4, 4)])
def test_inputs_that_are_row_slices_of_a_longer_recording(flag_offset, obs_offset):
    for T, N in ((2 * K + 1, 65), (K, 257), (5, 3)):    # (a slice [t0:t1] of a recording whose rows are no multiple of 16 bytes)
        _run(T, N, 3, flag_offset=flag_offset, obs_offset=obs_offset)
        _run(T, N, None, flag_offset=flag_offset)


def test_nan_in_the_unread_elements_and_any_bit_pattern_in_the_read_ones():
    T, N, D = 2 * K + 1, 130, 3
    case = _case(T, N, D, seed=4)
    rng = np.random.default_rng(4)
    for k in ("obs", "new_obs"):                        # NaN payloads, infinities, -0.0, denormals: words are copied
        case[k] = rng.integers(0, 2 ** 32, (T, N, D), dtype=np.uint64).astype(np.uint32).view(np.float32)
        case[k].view(np.uint32)[case[k].view(np.uint32) == 0xA5A5A5A5] = 0      # (the fence's poison word stays the sign of an unwritten one)
    case["new_obs"].view(np.uint32)[:, 0] = (0x80000000, 0x7fc00001, 0xff800001)
    call = Call(case)                                   # (poison=True: NaN wherever tn.reads says no result depends on the element)
    assert np.isnan(call.before["obs"]).any() and np.isnan(call.before["new_obs"]).any()
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check("arbitrary words: ")
    got = f32_bits(call.out["next_obs"].cpu().numpy())
    assert (got == 0x80000000).any() and (got == 0x7fc00001).any()


@pytest.mark.parametrize("ones", [False, True])
def test_reduction_against_the_input_planes(ones):
    """acted and new_obs_valid NULL (or all one): next_row[t] == t, the flags are the step's own (terminated wins), next_obs == new_obs"""
    T, N, D = 2 * K + 1, 257, 3
    case = _case(T, N, D, seed=21)
    case["acted"] = case["new_obs_valid"] = np.ones((T, N), np.uint8)
    call = Call(case, nulls=() if ones else ("acted", "new_obs_valid"), poison=False)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check()
    d, o = call.dev, call.out
    assert bool((o["next_row"] == torch.arange(T, device=_dev(), dtype=torch.int32)[:, None]).all())
    assert bool((o["next_terminated"] == (d["terminated"] != 0)).all())
    assert bool((o["next_truncated"] == ((d["terminated"] == 0) & (d["truncated"] != 0))).all())
    assert bool((o["next_obs"].view(torch.int32) == d["new_obs"].view(torch.int32)).all())
    assert bool(((d["terminated"] != 0) & (d["truncated"] != 0)).any())


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _abi.load_library()
    case = _case(K + 1, 65, 3, seed=1)
    call = Call(case)
    good = {n: getattr(call.io, n) for n, _ in call.io._fields_}

    def refused(what, **patch):
        for n, v in good.items():
            setattr(call.io, n, v)
        for k, v in patch.items():
            setattr(call.io, k, v(good[k]) if callable(v) else v)
        assert call.launch() == -1, what                # PHX_EINVAL
        assert b"phx_traj_next" in lib.phx_last_error(), what
        call.check_untouched(what)

    for k in ("truncated", "next_row", "next_terminated", "next_truncated"):
        refused(f"{k} NULL", **{k: None})
    refused("next_obs without obs", obs=None)
    refused("next_obs without new_obs", new_obs=None)
    refused("next_obs without either", obs=None, new_obs=None)
    for bad in (0, -1, 65, 1 << 20):
        refused(f"D = {bad}", D=bad)
    for k in ("obs", "new_obs"):
        refused(f"{k} misaligned", **{k: lambda p: p + 2})
    for k in OUTPUTS:
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 4})
    refused("T = 0", T=0)
    refused("T < 0", T=-3)
    refused("N = 0", N=0)
    refused("N < 0", N=-1)
    refused("N beyond the scan's grid", N=WG * 0x7fffffff + 1)
    refused("N beyond the gather's grid", N=WG * 0x7fffffff, D=64)
    assert lib.phx_traj_next(None, None) == -1 and b"phx_traj_next" in lib.phx_last_error()
    for n, v in good.items():                           # and the same buffers receive a good call
        setattr(call.io, n, v)
    assert call.launch() == 0, lib.phx_last_error()
    call.check("after the refusals: ")


def test_last_kernel_names_the_kernels():
    lib = _abi.load_library()
    _run(3, 7)
    assert lib.phx_last_kernel() == b"phx_traj_next_kernel" == _abi.TRAJ_NEXT_KERNEL.encode()
    _run(3, 7, 2)
    assert lib.phx_last_kernel() == b"phx_traj_next_kernel+phx_traj_gather_kernel"
    assert lib.phx_last_kernel() == (_abi.TRAJ_NEXT_KERNEL + "+" + _abi.TRAJ_GATHER_KERNEL).encode()
    _run(3, 7)
    assert lib.phx_last_kernel() == b"phx_traj_next_kernel"


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(_case(2 * K + 1, 257, 3, seed=11))
    b = Call(_case(K - 1, 130, 5, seed=12), nulls=("acted",))
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
# 8-step episodes: the shops of the FSM supply chain act in RESTOCK steps (even t), the episode ends in step 7, a SELL step
S, B, STEPS, T = 5, 13, 8, 20


def _fsm_env(seed=5):
    env = supply_chain_env(S, [3] * S, STEPS, B, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


def _stk_env(seed=5):
    env = market_env(2, 3, 2, 6, 7, seed=seed, exogenous="device")
    env.reset()
    return env


def _plain_env(seed=5):
    env = supply_chain_env(9, [6] * 9, 7, 11, seed=seed, exogenous="device")
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
        rows = {k: [] for k in ("obs", "new_obs", "acted", "nvalid", "truncations", "terminations")}
        done, ends = 0, []
        while done < T:
            n = min(T - done, N - self.cur)
            tr = self.env.rollout(n)
            rows["obs"] += [self.cur_obs[None].clone(), tr.observations[:n - 1].clone()]
            rows["acted"] += [self.cur_valid[None].clone(), tr.obs_valid[:n - 1].clone()]
            for k, x in (("new_obs", tr.observations), ("nvalid", tr.obs_valid), ("truncations", tr.truncations), ("terminations", tr.terminations)):
                rows[k].append(x.clone())
            self.cur_obs = tr.last_obs.clone()
            self.cur += n
            self.cur_valid = self.reset_valid if self.cur == N else tr.obs_valid[n - 1].clone()
            self.cur %= N
            done += n
            ends.append(done - 1)
        return {k: torch.cat(v).cpu().numpy() for k, v in rows.items()}, ends


def _want(p):
    return tn.traj_next(p["truncations"], p["terminations"], p["acted"], p["nvalid"], p["obs"], p["new_obs"])


def _critic(x):
    return 0.5 * x[:, 0] - 0.25 * torch.tanh(x[:, 1]) + 0.125 * x[:, -1] * x[:, -1] + 0.75


@pytest.mark.parametrize("make", [_fsm_env, _stk_env])
def test_device_env_traj_next_on_a_real_rollout(make):
    twin = Twin(make)
    p, ends = twin.planes(T)
    assert len(ends) >= 3 and 0.2 < (p["acted"] != 0).mean() < 0.8
    dev = twin.env._device()
    to = lambda a: torch.from_numpy(a).to(dev.device)
    args = tuple(to(p[k]) for k in ("truncations", "terminations", "acted", "nvalid", "obs", "new_obs"))
    got = dev.traj_next(*args)
    assert dev.last_kernel() == "phx_traj_next_kernel+phx_traj_gather_kernel"
    want = _want(p)
    assert got[0].dtype == torch.int32 and got[1].dtype == got[2].dtype == torch.uint8 and got[3].dtype == torch.float32
    for g, w, name in zip(got, want, OUTPUTS):
        assert tuple(g.shape) == w.shape
        np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32) if name == "next_obs" else g.cpu().numpy(),
                                      f32_bits(w) if name == "next_obs" else w, err_msg=name)
    # without the observations: no gather, the same three planes, [T, N] views
    flat = lambda x: x.reshape(T, -1)
    three = dev.traj_next(*(flat(x) for x in args[:4]))
    assert dev.last_kernel() == "phx_traj_next_kernel" and three[3] is None
    for g, w in zip(three[:3], want[:3]):
        np.testing.assert_array_equal(g.cpu().numpy(), w.reshape(T, -1))
    # refusals at this level leave caller-owned outputs untouched
    shape = tuple(args[0].shape)
    D = args[4].shape[-1]
    outs = [fenced(shape, torch.int32, dev.device), fenced(shape, torch.uint8, dev.device), fenced(shape, torch.uint8, dev.device),
            fenced(shape + (D,), torch.float32, dev.device)]
    out = tuple(o[0] for o in outs)
    for name, i, bad in (("truncations", 0, args[0].to(torch.int32)), ("terminations", 1, args[1][:-1]), ("acted", 2, args[2].to(torch.float32)),
                         ("new_obs_valid", 3, args[3][:, :-1].contiguous()), ("new_obs", 5, args[5].double()), ("obs", 4, args[4][..., :-1].contiguous()),
                         ("acted", 2, args[2].cpu())):
        a = list(args); a[i] = bad
        with pytest.raises(ValueError, match=name):
            dev.traj_next(*a, out=out)
    with pytest.raises(ValueError, match="come together"):
        dev.traj_next(*args[:5], out=out)                                   # obs without new_obs
    with pytest.raises(ValueError, match="come together"):
        dev.traj_next(*args[:4], None, args[5], out=out)                    # and the reverse
    for i in range(4):                                                      # a misaligned out[i]
        raw = torch.full((out[i].numel() * out[i].element_size() + 16,), 0xA5, dtype=torch.uint8, device=dev.device)
        off = raw[4:4 + out[i].numel() * out[i].element_size()].view(out[i].dtype).view(out[i].shape)
        o = list(out); o[i] = off
        with pytest.raises(ValueError, match=rf"out\[{i}\]"):
            dev.traj_next(*args, out=tuple(o))
        assert_poison(raw, f"a refused call with out[{i}] misaligned")
    torch.cuda.synchronize()
    for _, whole in outs:
        assert_poison(whole, "a refused DeviceEnv.traj_next call")
    res = dev.traj_next(*args, out=out)                                     # and a good call fills them
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
    for (plane, whole), w, name in zip(outs, want, OUTPUTS):
        assert_fences(whole, T, name)
        assert_written(plane, name)
        np.testing.assert_array_equal(plane.cpu().numpy().view(np.uint32) if name == "next_obs" else plane.cpu().numpy(),
                                      f32_bits(w) if name == "next_obs" else w, err_msg=name)


def _check_fields(batch, p):
    """the four fields against the restatement on the twin's planes; to_sample_batches() takes its columns from them"""
    tm = lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0))          # [B, S, T, ..] -> [T, B, S, ..]
    nr, nte, ntr, nob = _want(p)
    assert batch.trajectory_next_row.dtype == np.int32 and batch.trajectory_terminateds.dtype == batch.trajectory_truncateds.dtype == bool
    assert batch.trajectory_new_obs.dtype == np.float32 and batch.trajectory_new_obs.shape == batch.new_obs.shape
    np.testing.assert_array_equal(tm(batch.trajectory_next_row), nr)
    np.testing.assert_array_equal(tm(batch.trajectory_terminateds), nte != 0)
    np.testing.assert_array_equal(tm(batch.trajectory_truncateds), ntr != 0)
    np.testing.assert_array_equal(f32_bits(tm(batch.trajectory_new_obs)), f32_bits(nob))
    # the step-aligned planes stay what the steps returned
    np.testing.assert_array_equal(f32_bits(tm(batch.new_obs)), f32_bits(p["new_obs"]))
    np.testing.assert_array_equal(tm(batch.truncateds), p["truncations"] != 0)
    np.testing.assert_array_equal(tm(batch.terminateds), p["terminations"] != 0)
    acted = p["acted"] != 0
    np.testing.assert_array_equal(tm(batch.obs_valid) != 0, acted)
    cols = batch.to_sample_batches()["default_policy"]
    am = lambda a: np.moveaxis(a, 0, 2)[np.moveaxis(acted, 0, 2)]      # the masked plane in (env, agent, step) order
    assert len(cols["obs"]) == int(acted.sum())
    np.testing.assert_array_equal(f32_bits(cols["new_obs"]), f32_bits(am(nob)))
    np.testing.assert_array_equal(cols["terminateds"], am(nte != 0))
    np.testing.assert_array_equal(cols["truncateds"], am(ntr != 0))
    np.testing.assert_array_equal(cols["trajectory_next_row"], am(nr))
    return cols, (nr, nte, ntr, nob)


@pytest.mark.parametrize("with_critic", [False, True])
@pytest.mark.parametrize("make", [_fsm_env, _stk_env])
def test_sample_fills_the_four_fields(make, with_critic):
    env, twin = make(), Twin(make)
    kw = dict(value_fn=_critic, gamma=0.99, lambda_=0.95) if with_critic else {}
    batch = env.sample(T, **kw)
    assert env._device().last_kernel() == "phx_gae_masked_kernel"      # traj_next is issued before it
    p, ends = twin.planes(T)
    assert len(ends) >= 3                                              # at least three episode pieces
    cols, (nr, nte, ntr, nob) = _check_fields(batch, p)
    assert (batch.vf_preds is not None) == with_critic and batch.trajectory_rewards is not None
    # the same columns through the RLlib adapter (same seed, fresh env)
    sb = ph.rllib.BatchedBaseEnv(make()).sample(T, **kw)["default_policy"]
    for name in ("new_obs", "terminateds", "truncateds", "trajectory_next_row", "rewards", "obs"):
        np.testing.assert_array_equal(sb[name], cols[name], err_msg=name)
    # a second call continues where the first one stopped
    again = env.sample(5, **kw)
    p2, _ = twin.planes(5)
    _check_fields(again, p2)
    if make is not _fsm_env:
        return
    # ---- the gap this closes, on the FSM supply chain whose episodes end in a SELL step ------------------------------------------
    Bn, Sn = batch.B, batch.S
    acted = batch.obs_valid != 0                                        # [B, S, T]
    assert (batch.stage[:, STEPS - 1] == batch.stage_ids.index("SELL")).all() and batch.truncateds[:, :, STEPS - 1].all()
    assert not acted[:, :, STEPS - 1].any()                             # nobody acts in the step that ends the episode
    assert not (batch.truncateds & acted).any() and not (batch.terminateds & acted).any()      # no kept row shows a step-aligned flag
    assert (batch.trajectory_truncateds & acted & ~batch.truncateds).any()
    differs = (f32_bits(batch.trajectory_new_obs) != f32_bits(batch.new_obs)).any(axis=-1)
    assert (differs & acted).any()
    finished = [e for e in ends if (e + 1) % STEPS == 0]                # fragment rows that end an episode
    assert len(finished) == 2
    done = (batch.trajectory_truncateds | batch.trajectory_terminateds) & acted
    assert (done.sum(axis=2) == len(finished)).all()                    # per env instance and agent: one flag per finished episode
    n_kept = acted.sum(axis=2)
    eps = np.broadcast_to(batch.eps_id[:, None, :], acted.shape)
    for b in range(Bn):
        for s in range(Sn):
            kept = np.flatnonzero(acted[b, s])
            for i in np.flatnonzero(done[b, s][kept]):                  # each done row is the last kept row of its eps_id
                assert i + 1 == len(kept) or eps[b, s, kept[i + 1]] != eps[b, s, kept[i]], (b, s, kept[i])
            # and every kept row but the agent's last is a complete transition
            complete = done[b, s][kept] | (batch.trajectory_next_row[b, s][kept] >= 0)
            assert complete[:-1].all(), (b, s)
    assert n_kept.min() >= 3
    # in the sample batch: the flag rows split an agent's rows into its episodes
    c_done = cols["truncateds"] | cols["terminateds"]
    assert int(c_done.sum()) == Bn * Sn * len(finished)
    ends_of_eps = np.flatnonzero((np.diff(cols["eps_id"]) != 0) | (np.diff(cols["agent_index"]) != 0) | (np.diff(cols["env_id"]) != 0))
    last_episode = cols["eps_id"] // Bn == batch.eps_id.max() // Bn     # (unfinished: the fragment stops inside it)
    np.testing.assert_array_equal(np.flatnonzero(c_done), [i for i in ends_of_eps if not last_episode[i]])


def test_a_plain_envs_sample_is_what_it_was():
    env = _plain_env()
    batch = env.sample(T, value_fn=_critic, gamma=0.99, lambda_=0.95)
    assert env._device().last_kernel() == "phx_gae_kernel"
    assert batch.trajectory_next_row is None and batch.trajectory_new_obs is None
    assert batch.trajectory_terminateds is None and batch.trajectory_truncateds is None
    cols = batch.to_sample_batches()["default_policy"]
    assert "trajectory_next_row" not in cols
    np.testing.assert_array_equal(f32_bits(cols["new_obs"]), f32_bits(batch.new_obs.reshape(-1, batch.new_obs.shape[-1])))
    np.testing.assert_array_equal(cols["truncateds"], batch.truncateds.reshape(-1))
    np.testing.assert_array_equal(cols["terminateds"], batch.terminateds.reshape(-1))
    env2 = _plain_env()
    env2.sample(T)
    assert env2._device().last_kernel() != "" and "phx_traj" not in env2._device().last_kernel() and "gae" not in env2._device().last_kernel()
