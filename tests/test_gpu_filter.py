"""phx_filter_update / phx_filter_apply (include/phantom_amd_filter.h) on the GPU, through the C ABI into fenced buffers: the state's
bytes bit-equal to the numpy restatement (tests/filter_ref.py) after every call of a three-update sequence -- N at the edges of the
256-lane fold, T below, at and across the column walks' chunks, D on each of their chunk depths, an empty class and a column of no
class, keep NULL / all zero / random -- and apply bit-equal for counts of 0, 1 and many, with and without a clamp, in place and out of
place, every element written; calls queued without a wait; every refusal; the kernel names; then ObsFilter behind
sample(obs_filter=...) on a plain and an FSM supply chain against an unfiltered twin, and a fused rollout with the filter folded into
an MLPPolicy."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import filter_ref as fr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import DeviceBatch

pytestmark = pytest.mark.gpu
EINVAL = -1
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_obs_filter.hip")).read()
WG = int(re.search(r"constexpr int FL_LANES = (\d+);", SRC).group(1))              # columns per workgroup of the column walks
FA_CHUNK = int(re.search(r"constexpr int FA_THREADS = (\d+);", SRC).group(1)) * int(re.search(r"constexpr int FA_U = (\d+);", SRC).group(1)) * 4
assert "return D <= 4 ? 8 : (D <= 8 ? 4 : 2);" in SRC                               # the walks' rows per chunk: TS below crosses each of them
TS = (1, 2, 7, 9, 17)
NS = (1, 255, 256, 257, 513)
DS = (1, 3, 16)
CLASSES_KEEP = [(c, k) for c in (1, 3, 16) for k in ("none", "zero", "random")]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    return _abi.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _up(a, byte_offset=0):
    """`a` on the device, `byte_offset` bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device=_dev())
    x = raw[byte_offset:byte_offset + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    x.copy_(torch.from_numpy(a))
    assert x.data_ptr() % 16 == byte_offset
    return x


class Filter:
    """a filter's device state (i64 [n_classes, 34]: 272-byte records; zero-filled) and workspace, both fenced, with the restatement
    of the state next to them"""

    def __init__(self, N, D, n_classes):
        self.N, self.D, self.n_classes = N, D, n_classes
        self.state, self.state_whole = fenced((n_classes, 34), torch.int64, _dev())
        self.state.zero_()
        self.ws, self.ws_whole = fenced((fr.workspace_bytes(N, D) // 8,), torch.float64, _dev())
        self.ref = fr.empty_state(n_classes)
        self.keepalive = []

    def update_io(self, obs, keep, cls, keep_offset=0):
        T = obs.shape[0]
        d = [_up(obs), None if keep is None else _up(keep, keep_offset), None if cls is None else _up(cls)]
        self.keepalive.append(d)
        p = lambda x: None if x is None else x.data_ptr()
        return _abi.PhxFilterUpdateIO(T=T, D=self.D, N=self.N, n_classes=self.n_classes, obs=p(d[0]), keep=p(d[1]), col_class=p(d[2]),
                                      state=self.state.data_ptr(), workspace=self.ws.data_ptr())

    def update(self, obs, keep, cls, keep_offset=0, check=True, what=""):
        io = self.update_io(obs, keep, cls, keep_offset)
        assert _lib().phx_filter_update(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        self.ref = fr.update(self.ref, obs, keep, cls)
        if check:
            self.check(what)

    def check(self, what=""):
        got = self.state.cpu().numpy().view(np.uint8).reshape(-1).view(fr.STATE_DTYPE)
        for name in fr.STATE_DTYPE.names:
            np.testing.assert_array_equal(_bits(got[name]), _bits(self.ref[name]), err_msg=f"{what}state.{name}: {got[name]} != {self.ref[name]}")
        assert_fences(self.state_whole, self.n_classes, what + "state")
        assert_fences(self.ws_whole, self.ws.shape[0], what + "workspace")

    def apply(self, x, keep, cls, clip, in_place, check=True, what=""):
        """one phx_filter_apply call into a fenced plane; returns a function that checks it (at once when `check`)"""
        T = x.shape[0]
        out, whole = fenced((T, self.N, self.D), torch.float32, _dev())
        if in_place:
            out.copy_(torch.from_numpy(x))
            obs = out
        else:
            obs = _up(x)
        d = [obs, None if keep is None else _up(keep), None if cls is None else _up(cls)]
        self.keepalive.append(d)
        p = lambda t: None if t is None else t.data_ptr()
        io = _abi.PhxFilterApplyIO(T=T, D=self.D, N=self.N, n_classes=self.n_classes, clip=clip, obs=p(obs), keep=p(d[1]), col_class=p(d[2]),
                                   state=self.state.data_ptr(), out=out.data_ptr())
        assert _lib().phx_filter_apply(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        want = fr.apply(self.ref, x, keep, cls, clip)

        def verify():
            w = f"{what}apply(clip={clip}, in_place={in_place}): "
            assert_fences(whole, T, w + "out")
            if not in_place:
                assert_written(out, w + "out")
                np.testing.assert_array_equal(_bits(obs.cpu().numpy()), _bits(x), err_msg=w + "obs changed")
            np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want), err_msg=w + "out")
        if check:
            verify()
        return verify


def _with_outliers(rng, obs):
    """a plane to normalise: the case's values, 2 % of them 50 times as large -- a clamp at 10 standard deviations bites"""
    return (obs * np.where(rng.uniform(size=obs.shape) < 0.02, 50.0, 1.0)).astype(np.float32)


def _sequence(T, N, D, n_classes, keep, seed, applies=True):
    rng = np.random.default_rng([seed, T, N, D, n_classes])
    what = f"T={T} N={N} D={D} classes={n_classes} keep={keep}: "
    f = Filter(N, D, n_classes)
    x0, k0, cls = fr.random_case(rng, T, N, D, n_classes, keep)
    if applies:                                               # count 0 everywhere: the identity, the clamp included
        f.apply(_with_outliers(rng, x0), k0, cls, 10.0, False, what=what + "fresh: ")
    for u in range(3):
        obs, k, cls_u = fr.random_case(rng, T, N, D, n_classes, keep, offset=30.0 * u)
        f.update(obs, k, cls, keep_offset=u % 2, what=what + f"update {u}: ")
    assert keep == "zero" or f.ref["count"].sum() > 0
    if applies:
        x = _with_outliers(rng, x0)
        for clip, in_place in ((0.0, False), (10.0, False), (10.0, True), (0.0, True)):
            f.apply(x, k0, cls, clip, in_place, what=what)
        f.check(what + "after the applies: ")                 # apply never writes the state
    return f


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_state_and_apply_are_bit_equal_to_the_restatement(N, D):
    for i, T in enumerate(TS):
        for j, (n_classes, keep) in enumerate(CLASSES_KEEP):
            if (i + j) % 3 == 0 or T == 7:                    # every T with every third combination, T = 7 with all nine
                _sequence(T, N, D, n_classes, keep, seed=1)


@pytest.mark.parametrize("D", [2, 4, 5, 8, 9])
def test_the_other_feature_counts(D):
    """D = 4: an element is one 16-byte piece; 5 and 8: the walks' four-row chunks; 9: the two-row ones"""
    for T in (3, 5, 9):
        _sequence(T, 130, D, 3, "random", seed=2)


def test_many_workgroups_and_a_long_fragment():
    f = _sequence(100, 20 * WG + 7, 3, 2, "random", seed=3)
    assert f.N * 3 * 100 > 4 * FA_CHUNK


def test_apply_with_a_count_of_one():
    x = np.array([[[4.0, -2.0, 0.5], [1.0, 1.0, 1.0]], [[8.0, 8.0, 8.0], [0.0, 0.0, 0.0]]], np.float32)      # T = 2, N = 2, D = 3
    keep = np.array([[1, 0], [0, 0]], np.uint8)
    f = Filter(2, 3, 2)
    f.update(x, keep, np.array([0, 1], np.int32))
    assert f.ref["count"].tolist() == [1, 0] and f.ref["mean"][0, :3].tolist() == [4.0, -2.0, 0.5]
    for clip in (0.0, 10.0):
        for in_place in (False, True):
            f.apply(x * 3, None, np.array([0, 1], np.int32), clip, in_place)
            f.apply(x * 3, None, None, clip, in_place)        # every column class 0
    want = fr.apply(f.ref, x * 3, None, None, 0.0)
    assert want[1, 0].tolist() == [(np.float32(24) - np.float32(4)) / (np.float32(4) + np.float32(1e-8)),
                                   (np.float32(24) + np.float32(2)) / (np.float32(2) + np.float32(1e-8)),
                                   (np.float32(24) - np.float32(0.5)) / (np.float32(0.5) + np.float32(1e-8))]


def test_calls_queued_without_a_wait_between_them():
    rng = np.random.default_rng(5)
    T, N, D, n_classes = 9, 300, 3, 3
    f = Filter(N, D, n_classes)
    verify = []
    for u in range(3):
        obs, k, cls = fr.random_case(rng, T, N, D, n_classes, "random", offset=1000.0 * u)
        verify.append(f.apply(_with_outliers(rng, obs), k, cls, 10.0, u == 1, check=False, what=f"queued {u}: "))      # with the state before ..
        f.update(obs, k, cls, check=False)                                                                          # .. this update
    verify.append(f.apply(obs, None, cls, 0.0, False, check=False, what="queued last: "))
    for v in verify:
        v()
    f.check("queued: ")
    assert f.ref["updates"].tolist() == [3, 3, 0]


def test_last_kernel_names_the_kernels_launched():
    f = _sequence(3, 70, 3, 2, "random", seed=6, applies=False)
    assert _lib().phx_last_kernel() == fr.UPDATE_KERNELS.encode() == _abi.FILTER_UPDATE_KERNELS.encode()
    f.apply(np.zeros((3, 70, 3), np.float32), None, None, 0.0, False)
    assert _lib().phx_last_kernel() == fr.APPLY_KERNEL.encode() == _abi.FILTER_APPLY_KERNEL.encode()
    assert all(f"void {k}(" in SRC for k in fr.UPDATE_KERNELS.split("+") + [fr.APPLY_KERNEL])


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _lib()
    rng = np.random.default_rng(8)
    T, N, D, n_classes = 5, 66, 3, 3
    obs, k, cls = fr.random_case(rng, T, N, D, n_classes, "random")
    f = Filter(N, D, n_classes)
    f.update(obs, k, cls)                                     # a state that is not all zero
    before = f.state_whole.cpu().numpy().copy()
    ws_before = f.ws_whole.cpu().numpy().copy()
    out, out_whole = fenced((T, N, D), torch.float32, _dev())
    uio = f.update_io(obs, k, cls)
    d = f.keepalive[-1]
    aio = _abi.PhxFilterApplyIO(T=T, D=D, N=N, n_classes=n_classes, clip=10.0, obs=d[0].data_ptr(), keep=d[1].data_ptr(), col_class=d[2].data_ptr(),
                                state=f.state.data_ptr(), out=out.data_ptr())
    calls = {"phx_filter_update": (uio, lib.phx_filter_update), "phx_filter_apply": (aio, lib.phx_filter_apply)}

    def refused(fn, what, **patch):
        io, call = calls[fn]
        good = type(io).from_buffer_copy(io)                  # (a copy: getattr of an array field is a view of the struct)
        for name, v in patch.items():
            setattr(io, name, v(getattr(good, name)) if callable(v) else v)
        rc, err = call(C.byref(io), _stream()), lib.phx_last_error()
        C.memmove(C.byref(io), C.byref(good), C.sizeof(io))
        assert rc == EINVAL and fn.encode() in err, (fn, what, rc, err)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(f.state_whole.cpu().numpy(), before, err_msg=f"{fn}: {what}: state")
        np.testing.assert_array_equal(_bits(f.ws_whole.cpu().numpy()), _bits(ws_before), err_msg=f"{fn}: {what}: workspace")
        assert_poison(out_whole, f"{fn}: {what}: out")

    for fn in calls:
        for name in ("obs", "state"):
            refused(fn, f"{name} NULL", **{name: None})
            refused(fn, f"{name} off a 16-byte boundary", **{name: lambda p: p + 8})
        refused(fn, "col_class misaligned", col_class=lambda p: p + 2)
        for bad in (0, -1):
            refused(fn, f"T = {bad}", T=bad)
            refused(fn, f"N = {bad}", N=bad)
        for bad in (0, -1, 17):
            refused(fn, f"D = {bad}", D=bad)
            refused(fn, f"n_classes = {bad}", n_classes=bad)
        for i in (0, 1):
            r = (C.c_int64 * 2)()
            r[i] = 1
            refused(fn, f"reserved[{i}]", reserved=r)
    refused("phx_filter_update", "workspace NULL", workspace=None)
    refused("phx_filter_update", "workspace misaligned", workspace=lambda p: p + 8)
    refused("phx_filter_update", "reserved0", reserved0=1)
    refused("phx_filter_update", "N beyond the grid", N=WG * 0x7fffffff + 1)
    refused("phx_filter_apply", "out NULL", out=None)
    refused("phx_filter_apply", "out misaligned", out=lambda p: p + 4)
    for bad in (-1.0, -0.5, float("nan"), float("-inf")):
        refused("phx_filter_apply", f"clip = {bad}", clip=bad)
    refused("phx_filter_apply", "out overlaps obs from behind", out=lambda p: aio.obs + 16)
    refused("phx_filter_apply", "out overlaps obs from the front", out=lambda p: aio.obs - 16)
    refused("phx_filter_apply", "a row beyond 32 bits", N=(0x7fffffff - FA_CHUNK) // D + 1)
    refused("phx_filter_apply", "the plane beyond the grid", T=0x7fffffff, N=0x7fffffff // 16, D=16)
    for fn, (_, call) in calls.items():
        assert call(None, None) == EINVAL and fn.encode() in lib.phx_last_error()
    assert lib.phx_filter_apply(C.byref(aio), _stream()) == 0, lib.phx_last_error()       # and the same buffers receive good calls
    assert_fences(out_whole, T, "after the refusals: out")
    assert_written(out, "after the refusals: out")
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(fr.apply(f.ref, obs, k, cls, 10.0)))
    assert lib.phx_filter_update(C.byref(uio), _stream()) == 0, lib.phx_last_error()
    f.ref = fr.update(f.ref, obs, k, cls)
    f.check("after the refusals: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
T_E2E = 12                                                    # 10-step episodes: the fragments cut one and the second call finishes it


def _plain_env(seed=5):
    env = supply_chain_env(4, [3] * 4, 10, 7, seed=seed, exogenous="device")
    env.reset()
    return env


def _fsm_env(seed=5):
    env = supply_chain_env(3, [2] * 3, 10, 6, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


def _tm(a):
    return None if a is None else np.ascontiguousarray(np.moveaxis(a, 2, 0))      # [B, S, T, ..] -> [T, B, S, ..]


def _mapping(env):
    ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
    return lambda aid: "even" if ids.index(aid) % 2 == 0 else "odd"


def _same_state(f, ref, what):
    got = f.state()
    for name in fr.STATE_DTYPE.names:
        np.testing.assert_array_equal(_bits(got[name]), _bits(ref[name]), err_msg=f"{what}: state.{name}")


def _expected(ref, twin_batch, cls):
    """the restatement's (obs, new_obs) planes [T, B, S, D] of a filtered call from the unfiltered twin's batch, and the state after it"""
    obs, new_obs = _tm(twin_batch.obs), _tm(twin_batch.new_obs)
    T, B, S, D = obs.shape
    acted, nvalid = _tm(twin_batch.obs_valid), _tm(twin_batch.new_obs_valid)
    flat = lambda x: None if x is None else x.reshape(T, B * S)
    want_obs = fr.apply(ref, obs.reshape(T, B * S, D), flat(acted), cls, 10.0).reshape(obs.shape)
    want_new = fr.apply(ref, new_obs.reshape(T, B * S, D), flat(nvalid), cls, 10.0).reshape(obs.shape)
    return want_obs, want_new, fr.update(ref, obs.reshape(T, B * S, D), flat(acted), cls)


@pytest.mark.parametrize("make", [_plain_env, _fsm_env], ids=["plain", "fsm"])
def test_sample_with_an_obs_filter_against_an_unfiltered_twin(make):
    env, twin = make(), make()
    fn = _mapping(env)
    f = ph.ObsFilter(env, policy_mapping_fn=fn)
    B, S = env.batch_size, env.spec.n_strategic
    cls = np.tile(f.agent_class, B)
    assert f.n_classes == 2 and f.clip == 10.0
    ref = fr.empty_state(2)
    kw = dict(n_step=2, gamma=0.9)
    for call in range(2):
        got, raw = env.sample(T_E2E, obs_filter=f, **kw), twin.sample(T_E2E, **kw)
        want_obs, want_new, new_ref = _expected(ref, raw, cls)
        if call == 0:                                         # a fresh filter: the batch the call returns without the keyword
            a, b = got.to_sample_batches(fn), raw.to_sample_batches(fn)
            assert set(a) == set(b) == {"even", "odd"}
            for pid in b:
                assert set(a[pid]) == set(b[pid])
                for name, x in b[pid].items():
                    np.testing.assert_array_equal(_bits(a[pid][name]), _bits(x), err_msg=f"first call: {pid}: {name}")
            for name, x in vars(raw).items():                 # (and every plane of a fragment without holes)
                if isinstance(x, np.ndarray) and raw.obs_valid is None:
                    np.testing.assert_array_equal(_bits(getattr(got, name)), _bits(x), err_msg=f"first call: {name}")
        else:
            assert (_bits(got.obs) != _bits(raw.obs)).any()
        np.testing.assert_array_equal(_bits(_tm(got.obs)), _bits(want_obs), err_msg=f"call {call}: obs")
        np.testing.assert_array_equal(_bits(_tm(got.new_obs)), _bits(want_new), err_msg=f"call {call}: new_obs")
        np.testing.assert_array_equal(_bits(got.rewards), _bits(raw.rewards), err_msg=f"call {call}: rewards")
        np.testing.assert_array_equal(_bits(got.actions), _bits(raw.actions), err_msg=f"call {call}: actions")
        if raw.trajectory_next_row is not None:               # the gathers copy the normalised planes bit for bit
            nrow, acted = _tm(raw.trajectory_next_row), _tm(raw.obs_valid) != 0
            gathered = np.take_along_axis(want_new, np.broadcast_to(np.clip(nrow, 0, None)[..., None], want_new.shape), 0)
            want_tn = np.where(acted[..., None], np.where((nrow >= 0)[..., None], gathered, want_obs), np.float32(0.0))
            np.testing.assert_array_equal(_bits(_tm(got.trajectory_new_obs)), _bits(want_tn), err_msg=f"call {call}: trajectory_new_obs")
        else:                                                 # a plain env: n-step's new_obs is new_obs of the last row folded
            last = _tm(np.where(raw.nstep_discounts == np.float32(0.9), 0, 1)) + np.arange(T_E2E)[:, None, None]
            want_ns = np.take_along_axis(want_new, np.broadcast_to(last[..., None], want_new.shape), 0)
            np.testing.assert_array_equal(_bits(_tm(got.nstep_new_obs)), _bits(want_ns), err_msg=f"call {call}: nstep_new_obs")
        ref = new_ref
        _same_state(f, ref, f"call {call}")
    assert (ref["count"] > 0).all() and ref["updates"].tolist() == [2, 2]
    stats = f.stats()
    assert list(stats) == ["even", "odd"] and stats["even"][0] == ref["count"][0]


def test_sample_with_an_obs_filter_and_a_batcher_on_the_plain_env():
    env, twin = _plain_env(), _plain_env()
    fn = _mapping(env)
    f, tb = ph.ObsFilter(env, policy_mapping_fn=fn), ph.TrainBatcher(env, seed=3, policy_mapping_fn=fn)
    B, S = env.batch_size, env.spec.n_strategic
    cls = np.tile(f.agent_class, B)
    ref = fr.empty_state(2)
    for call in range(2):
        got, raw = env.sample(T_E2E, obs_filter=f, batcher=tb), twin.sample(T_E2E)
        want_obs, want_new, ref = _expected(ref, raw, cls)
        for pid, db in got.items():
            assert isinstance(db, DeviceBatch)
            row, col = db.row.cpu().numpy(), db.col.cpu().numpy()
            flat = lambda x: x.reshape(T_E2E, B * S, -1)[row, col]
            np.testing.assert_array_equal(_bits(db.columns["obs"].cpu().numpy()), _bits(flat(want_obs)), err_msg=f"call {call} {pid}: obs")
            np.testing.assert_array_equal(_bits(db.columns["new_obs"].cpu().numpy()), _bits(flat(want_new)), err_msg=f"call {call} {pid}: new_obs")
            if call == 0:
                np.testing.assert_array_equal(_bits(db.columns["obs"].cpu().numpy()), _bits(flat(_tm(raw.obs))))
        _same_state(f, ref, f"call {call}")
    adapter = ph.rllib.BatchedBaseEnv(_plain_env())           # the RLlib adapter passes the keyword through
    g = ph.ObsFilter(adapter.env)
    adapter.sample(T_E2E, obs_filter=g)
    assert g.stats()["default_policy"][0] == T_E2E * B * S


def test_compact_sampling_on_the_fsm_env_gives_the_same_filtered_columns():
    env, twin = _fsm_env(), _fsm_env()
    fn = _mapping(env)
    f, g = ph.ObsFilter(env, policy_mapping_fn=fn), ph.ObsFilter(twin, policy_mapping_fn=fn)
    for call in range(2):
        got = env.sample(T_E2E, obs_filter=f, compact=True).to_sample_batches(fn)
        want = twin.sample(T_E2E, obs_filter=g).to_sample_batches(fn)         # (held against the restatement by the test above)
        assert set(got) == set(want)
        for pid in want:
            assert set(got[pid]) == set(want[pid])
            for name, x in want[pid].items():
                np.testing.assert_array_equal(_bits(got[pid][name]), _bits(x), err_msg=f"call {call} {pid}: {name}")
        _same_state(f, g.state(), f"call {call}")
    assert (f.state()["count"] > 0).all()


def test_a_fused_rollout_with_the_filter_folded_into_the_policy():
    env = _plain_env()
    f = ph.ObsFilter(env, clip=None)
    env.sample(T_E2E, obs_filter=f)                           # statistics to fold
    rng = np.random.default_rng(2)
    ws = [rng.normal(0, 0.7, (16, 3)).astype(np.float32), rng.normal(0, 0.3, (1, 16)).astype(np.float32)]
    bs = [rng.normal(0, 0.3, (16,)).astype(np.float32), np.array([0.1], np.float32)]
    pol = ph.MLPPolicy(ws, bs, activation="tanh", out_scale=50.0, out_bias=50.0)
    W0, b0 = f.fold(pol.weights, pol.biases)
    mean_f, den_f, _ = fr.table(f.state(), 3)
    for got, want in zip((W0, b0), fr.fold_layer(ws[0], bs[0], mean_f[0], den_f[0])):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    assert (W0 != ws[0]).any()
    pol.update([W0, ws[1]], [b0, bs[1]])
    for got, want in zip((pol.weights[0], pol.biases[0]), (W0, b0)):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    before = f.state()
    batch = env.sample(T_E2E, policy=pol, obs_filter=f)       # the fused policy rollout acts on raw observations
    assert np.isfinite(batch.actions).all() and len(np.unique(batch.actions)) > 10
    assert f.state()["count"][0] == before["count"][0] + T_E2E * env.batch_size * env.spec.n_strategic
    with pytest.raises(ValueError, match="clip"):
        ph.ObsFilter(env).fold(ws, bs)
