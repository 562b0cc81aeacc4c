"""phx_episode_stats (include/phantom_amd_episodes.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with
the numpy restatement (tests/episode_ref.py) over row counts around the scan's chunk depth, column counts around the workgroup's,
groups of 2 and 3 input columns, class sizes around the reduction's 256 lanes, every combination of the optional inputs and outputs,
misaligned inputs, NaN in what the call does not read, columns that never act, carries with open episodes, every refusal, the kernel
names; then DeviceEnv.episode_stats on real plain, FSM and Stackelberg rollouts whose episodes end inside the fragment, and
PhantomEnv.sample(episode_stats=) over consecutive calls that cut episodes, compacted and not, against twin envs."""
import ctypes as C
import itertools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import episode_ref as er
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import f32_bits, market_env, supply_chain_env
from phantom_amd import _abi

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_episodes.hip")).read()
EP_K = int(re.search(r"constexpr int EP_K = (\d+);", SRC).group(1))               # the scan's chunk depth (items)
WG = int(re.search(r"constexpr int EP_LANES = (\d+);", SRC).group(1))             # its workgroup (output columns)
SHAPES = er.gpu_shapes(EP_K)
INPUTS = ("reward", "truncated", "terminated", "acted", "reward_valid")
OPT_IN = ("terminated", "acted", "reward_valid")
OPT_OUT = ("carry", "episode_return", "episode_len", "summary")
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


def _divisors(C):
    return [k for k in (1, 2, 3, 5, 7, 13, 63, 64, 257) if C % k == 0]


def _records(t):
    """a fenced i64 [n, 6] plane of 48-byte records on the host"""
    return t.cpu().numpy().view(np.uint8).reshape(-1).view(er.DTYPE)


class Call:
    """one phx_episode_stats call: device inputs (reward NaN wherever reward_valid says it is not read), every output fenced -- the
    two per-row planes, col_stats and summary as i64 [n, 6] (a 48-byte record is six words: none of them reads as the poison), the
    carry (in / out) filled with open and closed episodes.  An output in `nulls` is passed as NULL and its buffer must stay poison.
    `byte_offset` / `word_offset`: bytes past a 16-byte boundary the u8 and the f32 inputs start at"""

    def __init__(self, case, G=1, K=1, nulls=(), byte_offset=0, word_offset=0, carry=None):
        self.nulls, self.G, self.K = set(nulls), G, K
        T, N = case["reward"].shape
        self.T, self.N, self.C = T, N, N // G
        Cn = self.C
        self.ref = {k: (None if k in self.nulls else case[k]) for k in INPUTS}
        rng = np.random.default_rng([T, N, G])
        if carry is None:                                   # a third of the columns come in with an episode open
            carry = (rng.normal(0, 2, Cn).astype(np.float32), np.where(rng.random(Cn) < 0.33, rng.integers(0, 5, Cn), -1).astype(np.int32))
        self.carry_in = None if "carry" in self.nulls else carry
        self.want = er.episode_stats(G=G, K=K, carry=self.carry_in, **self.ref)
        host = dict(self.ref)
        if self.ref["reward_valid"] is not None:
            host["reward"] = np.where(self.ref["reward_valid"] == 1, case["reward"], NAN)
        self.dev = {k: _offset(v, byte_offset if v.dtype == np.uint8 else word_offset) for k, v in host.items() if v is not None}
        self.before = {k: v.cpu().numpy().copy() for k, v in self.dev.items()}
        shapes = dict(episode_return=((T, Cn), torch.float32), episode_len=((T, Cn), torch.int32), col_stats=((Cn, 6), torch.int64),
                      summary=((K, 6), torch.int64), carry_return=((Cn,), torch.float32), carry_len=((Cn,), torch.int32))
        self.out, self.whole = {}, {}
        for k, (shape, dtype) in shapes.items():
            self.out[k], self.whole[k] = fenced(shape, dtype, _dev())
        if self.carry_in is not None:
            self.out["carry_return"].copy_(torch.from_numpy(carry[0]))
            self.out["carry_len"].copy_(torch.from_numpy(carry[1]))
        p = lambda k: self.dev[k].data_ptr() if k in self.dev else None
        given = lambda k: (k not in self.nulls) and not (k.startswith("carry_") and "carry" in self.nulls)
        self.given = {k: given(k) for k in shapes}
        self.io = _abi.PhxEpisodeIO(T=T, G=G, N=N, K=K, **{k: p(k) for k in INPUTS},
                                    **{k: (self.out[k].data_ptr() if self.given[k] else None) for k in shapes})

    def launch(self):
        return _abi.load_library().phx_episode_stats(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        w = self.want
        for k, plane in self.out.items():
            assert_fences(self.whole[k], plane.shape[0], what + k)
            if not self.given[k]:
                assert_poison(self.whole[k], what + k + " passed as NULL")
                continue
            assert_written(plane, what + k)
            got = plane.cpu().numpy()
            if k in ("col_stats", "summary"):
                er.assert_same_stats(_records(plane), w[k], what + k + ": ")
            elif got.dtype == np.float32:
                np.testing.assert_array_equal(f32_bits(got), f32_bits(w[k]), err_msg=what + k)
            else:
                np.testing.assert_array_equal(got, w[k], err_msg=what + k)
        for k, v in self.dev.items():                   # the inputs are byte-identical after the call
            np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), self.before[k].view(np.uint8), err_msg=what + k)

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k, whole in self.whole.items():
            if k.startswith("carry_") and self.carry_in is not None:
                got = self.out[k].cpu().numpy()
                np.testing.assert_array_equal(got.view(np.uint32), self.carry_in[k == "carry_len"].view(np.uint32), err_msg=f"{what}: {k}")
                assert_fences(whole, self.out[k].shape[0], f"{what}: {k}")
            else:
                assert_poison(whole, f"{what}: {k}")


def _run(T, Cn, G=1, K=1, seed=0, **kw):
    call = Call(er.case(T, Cn, G, seed), G, K, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} C={Cn} G={G} K={K} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("Cn", [1, 63, 64, 65, 257])
def test_bit_equal_to_the_restatement_one_column_per_agent(Cn):
    """every T of the list with every C; the number of classes cycles over the divisors of C"""
    ks = _divisors(Cn)
    for i, (T, _, G) in enumerate(s for s in SHAPES if s[1] == Cn and s[2] == 1):
        _run(T, Cn, G, ks[i % len(ks)])


@pytest.mark.parametrize("G", [2, 3])
def test_bit_equal_to_the_restatement_groups_of_input_columns(G):
    for i, (T, Cn, _) in enumerate(s for s in SHAPES if s[2] == G):
        ks = _divisors(Cn)
        _run(T, Cn, G, ks[i % len(ks)])
    case = er.case(2 * EP_K + 1, 65, G)                 # what these cases hold (tests/test_episode_stats_cpu.py has the full condition)
    want = er.episode_stats(G=G, **case)
    assert want["col_stats"]["count"][2] == 0 and not case["acted"][:, 2 * G:3 * G].any()      # a column that never acts and never closes
    assert (want["col_stats"]["count"] >= 2).any() and (want["carry_len"] >= 0).any()


@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_class_sizes_around_the_reduction_s_lanes(M):
    for K, G in ((1, 1), (3, 1), (2, 2)):
        _run(EP_K + 1, M * K, G, K)


def test_many_workgroups_and_chunks():
    _run(4 * EP_K + 3, 43 * WG + 1, 1, 1)               # 44 workgroups of the scan, the last one with one live lane
    _run(3 * EP_K + 2, 9 * WG + 1, 3, 1)


@pytest.mark.parametrize("G", [1, 2])
def test_every_combination_of_the_optional_inputs_and_outputs(G):
    for r in range(len(OPT_IN) + 1):
        for nin in itertools.combinations(OPT_IN, r):
            for q in range(len(OPT_OUT) + 1):
                for nout in itertools.combinations(OPT_OUT, q):
                    _run(2 * EP_K + 1, 65, G, 5, nulls=nin + nout)


@pytest.mark.parametrize("byte_offset,word_offset", [(1, 4), (3, 12), (2, 8)])
def test_inputs_that_are_row_slices_of_a_longer_recording(byte_offset, word_offset):
    for T, Cn, G in ((2 * EP_K + 1, 65, 1), (EP_K, 257, 1), (5, 3, 1), (EP_K + 1, 65, 3)):
        _run(T, Cn, G, 1, byte_offset=byte_offset, word_offset=word_offset)


def test_nan_in_the_unread_rewards_and_carries_with_open_episodes():
    call = _run(2 * EP_K + 1, 130, 1, 2, seed=4)
    assert np.isnan(call.before["reward"]).any() and (~np.isnan(call.before["reward"])).any()
    assert not np.isnan(call.out["episode_return"].cpu().numpy()).any()
    assert (call.carry_in[1] >= 0).any() and (call.carry_in[1] < 0).any()
    rows = np.arange(1, 2 * EP_K + 2)[:, None]
    assert (call.want["episode_len"] > rows).any()      # an episode longer than its rows in this fragment: the carry's steps count
    # a carry below -1 reads as "no episode open"
    T, Cn = EP_K + 1, 65
    bad = (np.zeros(Cn, np.float32), np.full(Cn, -7, np.int32))
    bad[1][1] = -1
    _run(T, Cn, carry=bad)


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _abi.load_library()
    call = Call(er.case(EP_K + 1, 66, 2, seed=1), 2, 3)
    good = {n: getattr(call.io, n) for n, _ in call.io._fields_}

    def refused(what, **patch):
        for n, v in good.items():
            setattr(call.io, n, v)
        for k, v in patch.items():
            setattr(call.io, k, v(good[k]) if callable(v) else v)
        assert call.launch() == -1, what                # PHX_EINVAL
        assert b"phx_episode_stats" in lib.phx_last_error(), what
        call.check_untouched(what)

    for k in ("reward", "truncated", "col_stats"):
        refused(f"{k} NULL", **{k: None})
    refused("carry_return without carry_len", carry_len=None)
    refused("carry_len without carry_return", carry_return=None)
    for bad in (0, -1):
        refused(f"T = {bad}", T=bad)
        refused(f"N = {bad}", N=bad)
        refused(f"K = {bad}", K=bad)
    for bad in (0, -1, 257, 1 << 20):
        refused(f"G = {bad}", G=bad)
    refused("N no multiple of G", N=131)
    refused("C no multiple of K", K=4)
    refused("reserved0", reserved0=1)
    refused("C beyond the grid", N=2 * (WG * 0x7fffffff + 3), K=1)
    for k in ("reward", "carry_return", "carry_len"):
        refused(f"{k} misaligned", **{k: lambda p: p + 2})
    for k in ("episode_return", "episode_len", "col_stats", "summary"):
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    assert lib.phx_episode_stats(None, None) == -1 and b"phx_episode_stats" in lib.phx_last_error()
    for n, v in good.items():                           # and the same buffers receive a good call
        setattr(call.io, n, v)
    assert call.launch() == 0, lib.phx_last_error()
    call.check("after the refusals: ")


def test_last_kernel_names_the_kernels_launched():
    lib = _abi.load_library()
    s, r = _abi.EPISODE_SCAN_KERNEL, _abi.EPISODE_REDUCE_KERNEL
    _run(3, 7)
    assert lib.phx_last_kernel() == b"phx_episode_scan_kernel+phx_episode_reduce_kernel" == f"{s}+{r}".encode()
    _run(3, 7, nulls=("summary",))
    assert lib.phx_last_kernel() == b"phx_episode_scan_kernel" == s.encode()
    _run(3, 4, G=2, nulls=("summary", "carry"))
    assert lib.phx_last_kernel() == s.encode()


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(er.case(2 * EP_K + 1, 257, 1, seed=11), 1, 257)
    b = Call(er.case(EP_K - 1, 64, 2, seed=12), 2, 2, nulls=("acted",))
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
# 10-step episodes, 25-row fragments: two episodes end inside the fragment, a third is cut
T = 25
FIELDS = ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "t", "eps_id", "obs_valid", "new_obs_valid", "reward_valid",
          "stage", "vf_preds", "advantages", "value_targets", "trajectory_rewards", "trajectory_next_row", "trajectory_new_obs",
          "trajectory_terminateds", "trajectory_truncateds", "nstep_rewards", "nstep_discounts", "nstep_new_obs", "nstep_terminateds",
          "nstep_truncateds")


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
    return None if a is None else np.ascontiguousarray(np.moveaxis(a, 2, 0))      # [B, S, T, ..] -> [T, B, S, ..]


def _planes(batch):
    """the step-aligned time-major planes of a batch, as the five inputs of the call"""
    return dict(reward=_tm(batch.rewards), truncated=_tm(batch.truncateds).astype(np.uint8), terminated=_tm(batch.terminateds).astype(np.uint8),
                acted=_tm(batch.obs_valid), reward_valid=_tm(batch.reward_valid))


@pytest.mark.parametrize("make", [_plain_env, _fsm_env, _stk_env])
def test_device_env_episode_stats_on_a_real_rollout(make):
    env = make()
    batch = env.sample(T)
    assert len(batch.episodes()) >= 3                   # episodes end inside the fragment
    p = _planes(batch)
    masked = p["acted"] is not None
    dev = env._device()
    B, S = env.batch_size, env.spec.n_strategic
    to = lambda a: None if a is None else torch.from_numpy(a).to(dev.device)
    args = tuple(to(p[k]) for k in INPUTS)
    for G, K in ((1, S), (S, 1)):
        Cn = B * S // G
        carry = (torch.zeros(Cn, dtype=torch.float32, device=dev.device), torch.full((Cn,), -1, dtype=torch.int32, device=dev.device))
        col, summ, eret, elen = dev.episode_stats(*args, group=G, classes=K, carry=carry, planes=True)
        assert dev.last_kernel() == "phx_episode_scan_kernel+phx_episode_reduce_kernel"
        want = er.episode_stats(G=G, K=K, **p)
        assert (want["col_stats"]["count"] >= 2).all() and (want["carry_len"] >= 0).any()
        assert col.dtype == summ.dtype == torch.uint8 and tuple(col.shape) == (Cn, 48) and tuple(summ.shape) == (K, 48)
        er.assert_same_stats(col.cpu().numpy().reshape(-1).view(_abi.EPISODE_STATS_DTYPE), want["col_stats"], "col_stats: ")
        er.assert_same_stats(summ.cpu().numpy().reshape(-1).view(_abi.EPISODE_STATS_DTYPE), want["summary"], "summary: ")
        np.testing.assert_array_equal(f32_bits(eret.cpu().numpy()), f32_bits(want["episode_return"]))
        np.testing.assert_array_equal(elen.cpu().numpy(), want["episode_len"])
        np.testing.assert_array_equal(f32_bits(carry[0].cpu().numpy()), f32_bits(want["carry_return"]))
        np.testing.assert_array_equal(carry[1].cpu().numpy(), want["carry_len"])
        # [T, N] views, no carry, no planes, no summary: one launch into caller-owned memory
        flat = lambda x: None if x is None else x.reshape(T, -1)
        mine, whole = fenced((Cn, 48), torch.uint8, dev.device)
        res = dev.episode_stats(*(flat(x) for x in args), group=G, classes=K, summary=False, out=(mine, None, None, None))
        assert dev.last_kernel() == "phx_episode_scan_kernel" and res[0].data_ptr() == mine.data_ptr() and res[1:] == (None, None, None)
        assert_fences(whole, Cn, "col_stats")
        er.assert_same_stats(mine.cpu().numpy().reshape(-1).view(_abi.EPISODE_STATS_DTYPE), er.episode_stats(G=G, K=K, **p)["col_stats"])
    # refusals at this level come before any launch and leave caller-owned outputs untouched
    mine, whole = fenced((B * S, 48), torch.uint8, dev.device)
    out = (mine, None, None, None)
    bad_args = [("rewards", 0, args[0].double()), ("truncations", 1, args[1].to(torch.int32)), ("terminations", 2, args[2][:-1]),
                ("rewards", 0, args[0].cpu())]
    if masked:
        bad_args += [("acted", 3, args[3].to(torch.float32)), ("reward_valid", 4, args[4].to(torch.int64))]
    for name, i, bad in bad_args:
        a = list(args); a[i] = bad
        with pytest.raises(ValueError, match=name):
            dev.episode_stats(*a, out=out)
    for kw in (dict(group=0), dict(group=257), dict(group=True), dict(group=2.0), dict(classes=0), dict(classes=B * S + 1), dict(group=B * S + 1)):
        with pytest.raises(ValueError, match="group|classes"):
            dev.episode_stats(*args, **kw, out=out)
    with pytest.raises(ValueError, match="carry"):
        dev.episode_stats(*args, carry=(torch.zeros(B * S, device=dev.device), torch.zeros(B * S, device=dev.device)), out=out)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        dev.episode_stats(*args, group=S, out=out)      # col_stats sized for G = 1
    torch.cuda.synchronize()
    assert_poison(whole, "a refused DeviceEnv.episode_stats call")


def _expected(env, planes, policy_mapping_fn=None):
    """what EpisodeStats must report after fragments with these planes (_planes of each batch, taken before the next sample() call:
    a batch's arrays are views of pinned buffers the next call of the same shape reuses): the restatement fragment by fragment with the
    carry handed over, its summaries folded in call order; and the restatement over the concatenated planes"""
    S = env.spec.n_strategic
    host = ph.EpisodeStats(env, policy_mapping_fn=policy_mapping_fn)
    ca = ce = None
    for p in planes:
        a, e = er.episode_stats(G=1, K=S, carry=ca, **p), er.episode_stats(G=S, K=1, carry=ce, **p)
        ca, ce = (a["carry_return"], a["carry_len"]), (e["carry_return"], e["carry_len"])
        host.add_summaries(np.concatenate([a["summary"], e["summary"]]))
    cat = {k: (None if planes[0][k] is None else np.concatenate([p[k] for p in planes])) for k in INPUTS}
    return host.result(), er.episode_stats(G=1, K=S, **cat), er.episode_stats(G=S, K=1, **cat), (ca, ce)


def _same_result(got, want, what=""):
    assert set(got) == set(want), what
    for k, w in want.items():
        pairs = [(got[k], w)] if not isinstance(w, dict) else [(got[k][a], w[a]) for a in w]
        assert not isinstance(w, dict) or set(got[k]) == set(w), what + k
        for g, x in pairs:
            assert (math.isnan(g) and math.isnan(x)) or g == x, (what, k, g, x)


def _check_against_the_whole(env, res, agents, envs):
    """the numbers of a result against the restatement over the concatenation: counts, lengths, min and max exactly, the means to the
    f64 rounding of a differently ordered sum.  With A the sum of the |returns| of the n episodes: either order rounds at most n
    times (adding +0.0 is exact), each by at most 2^-53 A, so the two sums differ by at most n 2^-52 A; either division rounds by at
    most 2^-53 A / n: (n + 1) 2^-52 A / n in all"""
    e, a = envs["summary"][0], agents["summary"]
    n = int(e["count"])
    assert res["episodes_this_iter"] == n >= 1
    assert res["episode_len_mean"] == int(e["len_sum"]) / n
    assert (res["episode_reward_min"], res["episode_reward_max"]) == (float(e["ret_min"]), float(e["ret_max"]))
    bound = lambda planes, count: (count + 1) * 2.0 ** -52 * float(np.abs(planes.astype(np.float64)).sum()) / count
    assert abs(res["episode_reward_mean"] - float(e["ret_sum"]) / n) <= bound(envs["episode_return"], n)
    ids = [env.spec.agent_ids[i] for i in env.spec.strategic_idx]
    S = len(ids)
    for s, aid in enumerate(ids):
        assert int(a["count"][s]) >= 1
        assert res["agent_episode_len_mean"][aid] == int(a["len_sum"][s]) / int(a["count"][s])
        assert (res["agent_reward_min"][aid], res["agent_reward_max"][aid]) == (float(a["ret_min"][s]), float(a["ret_max"][s]))
        assert abs(res["agent_reward_mean"][aid] - float(a["ret_sum"][s]) / int(a["count"][s])) <= bound(agents["episode_return"][:, s::S],
                                                                                                         int(a["count"][s]))


def _same_fields(got, want, names):
    for k in names:
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None), k
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, k
            assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), k


@pytest.mark.parametrize("make", [_plain_env, _fsm_env])
def test_sample_with_episode_stats_over_three_calls_that_cut_episodes(make):
    env, twin = make(), make()
    st = ph.EpisodeStats(env, policy_mapping_fn=lambda aid: str(aid)[:1])
    Ts = (13, 13, 13)                                   # 10-step episodes: every call cuts one
    old, ref = [], None
    for n in Ts:                                        # the batch is the one the call returns without the keyword
        g, w = env.sample(n, episode_stats=st), twin.sample(n)
        _same_fields(g, w, FIELDS)
        a, b = g.to_sample_batches()["default_policy"], w.to_sample_batches()["default_policy"]
        assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in b)
        old.append(_planes(w))
        ref = ref or {k: v.copy() for k, v in b.items()}
    want, agents, envs, (ca, ce) = _expected(env, old, policy_mapping_fn=lambda aid: str(aid)[:1])
    assert (ca[1] >= 0).any() and (ce[1] >= 0).any()    # an episode is open at the end: the next call goes on with it
    res = st.result()
    _same_result(res, want)
    _check_against_the_whole(env, res, agents, envs)
    assert res["episodes_this_iter"] == 3 * env.batch_size and "policy_reward_mean" in res
    np.testing.assert_array_equal(f32_bits(st._carry_agent[0].cpu().numpy()), f32_bits(ca[0]))
    np.testing.assert_array_equal(st._carry_agent[1].cpu().numpy(), ca[1])
    np.testing.assert_array_equal(f32_bits(st._carry_env[0].cpu().numpy()), f32_bits(ce[0]))
    np.testing.assert_array_equal(st._carry_env[1].cpu().numpy(), ce[1])
    empty = st.result()                                 # reset=True cleared the totals ..
    assert empty["episodes_this_iter"] == 0 and math.isnan(empty["episode_reward_mean"])
    more, old_more = env.sample(11, episode_stats=st, value_fn=_critic, n_step=2), twin.sample(11, value_fn=_critic, n_step=2)
    _same_fields(more, old_more, FIELDS)                # .. not the carries: the fourth call closes the episode the third one cut
    p = _planes(old_more)
    S = env.spec.n_strategic
    e4 = er.episode_stats(G=S, K=1, carry=ce, **p)
    r4 = st.result()
    n4 = int(e4["summary"]["count"][0])
    assert r4["episodes_this_iter"] == n4 == 2 * env.batch_size         # rows 39 .. 49 of 10-step episodes: two more end
    assert (e4["episode_len"][0] >= 0).all()            # .. the first of them in the call's first row, with the carry's nine steps
    assert r4["episode_len_mean"] == int(e4["summary"]["len_sum"][0]) / n4
    assert r4["episode_reward_mean"] == float(e4["summary"]["ret_sum"][0]) / n4
    st.drop_open()
    assert bool((st._carry_agent[1] == -1).all()) and bool((st._carry_env[1] == -1).all()) and bool((st._carry_env[0] == 0).all())
    # the same through the RLlib adapter
    third = make()
    st2 = ph.EpisodeStats(third)
    cols = ph.rllib.BatchedBaseEnv(third).sample(13, episode_stats=st2)["default_policy"]
    assert set(cols) == set(ref) and all(cols[k].tobytes() == ref[k].tobytes() for k in ref)
    first, _, _, _ = _expected(env, old[:1])
    _same_result(st2.result(), first)


@pytest.mark.parametrize("make", [_fsm_env, _stk_env])
def test_compact_sampling_reports_the_same_episodes(make):
    env, twin = make(), make()
    st = ph.EpisodeStats(env)
    Ts = (13, 9, 17) if make is _fsm_env else (8, 5, 9)       # the market's episodes are 6 steps long
    frags = [env.sample(n, compact=True, episode_stats=st) for n in Ts]
    assert all(isinstance(f, ph.rollout.CompactFragment) for f in frags)
    old = [_planes(twin.sample(n)) for n in Ts]
    want, agents, envs, _ = _expected(env, old)
    res = st.result()
    _same_result(res, want)
    _check_against_the_whole(env, res, agents, envs)


def test_each_closed_agent_return_is_the_f32_sum_of_the_rollout_container_s_rewards():
    env = _fsm_env()
    batch = env.sample(20)                              # two whole 10-step episodes
    p = _planes(batch)
    dev = env._device()
    to = lambda a: torch.from_numpy(a).to(dev.device)
    _, _, eret, elen = dev.episode_stats(*(to(p[k]) for k in INPUTS), planes=True, summary=False)
    eret, elen = eret.cpu().numpy().reshape(20, env.batch_size, -1), elen.cpu().numpy().reshape(20, env.batch_size, -1)
    rollouts = batch.rollouts()
    B = env.batch_size
    assert len(rollouts) == 2 * B
    seen = 0
    for i, (t0, n) in enumerate(batch.episodes()):
        for b in range(B):
            ro = rollouts[i * B + b]
            for s, aid in enumerate(batch.agent_ids):
                total = np.float32(0.0)
                for r in ro.rewards_for_agent(aid, drop_nones=True):
                    total = np.float32(total + np.float32(r))
                closes = np.flatnonzero(elen[t0:t0 + n, b, s] >= 0)
                assert list(closes) == [n - 1], (i, b, aid)
                assert f32_bits(eret[t0 + n - 1, b, s]) == f32_bits(total), (i, b, aid)
                seen += 1
    assert seen == 2 * B * len(batch.agent_ids)
