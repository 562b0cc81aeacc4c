"""phx_traj_compact (include/phantom_amd_compact.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with
the numpy restatement (tests/compact_ref.py) of start, out_row, out_col and every plane over row counts around the scatter's chunk
depth, column counts around its tile width and one beyond the scan's block, four element sizes and every density of the generator;
the capacity clip, the plane counts, the optional index outputs, row slices at odd offsets, the reduction, every refusal; then
DeviceEnv.compact on a real FSM rollout and PhantomEnv.sample(compact=True) against a twin env's sample()."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compact_ref as cr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, fenced
from helpers import market_env, supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import CompactFragment, FragmentBatch

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_traj_compact.hip")).read()
R = int(re.search(r"constexpr int CP_R = (\d+);", SRC).group(1))                  # the scatter's chunk depth (rows)
CW = int(re.search(r"constexpr int CP_C = (\d+);", SRC).group(1))                 # the scatter's tile width (columns)
SB = int(re.search(r"constexpr int CP_SB = (\d+);", SRC).group(1))                # the scan's block (entries)
TS = (1, R - 1, R, R + 1, 2 * R + 1)
NS = (1, CW - 1, CW, CW + 1, 4 * CW + 1)
ELEM_BYTES = (1, 4, 12, 20)
EINVAL = -1


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _offset(host, nbytes):
    """`host` on the device, starting `nbytes` bytes past a 16-byte boundary (0: on one)"""
    a = np.ascontiguousarray(host)
    a = a if a.dtype == np.uint8 else a.view(np.int32)      # (u32 words travel as i32: the bytes are what is compared)
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device=_dev())
    assert raw.data_ptr() % 16 == 0
    x = raw[nbytes:nbytes + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    x.copy_(torch.from_numpy(a))
    assert x.data_ptr() % 16 == nbytes
    return x


class Call:
    """one phx_traj_compact call: device inputs, fenced and poisoned outputs.  `planes`: the elem_bytes of each plane, in order;
    `capacity` None: T * N; `rows` / `cols`: out_row / out_col given; `keep_offset` / `byte_offset` / `word_offset`: bytes past a
    16-byte boundary at which keep, the byte planes and the word planes start"""

    def __init__(self, keep, planes=ELEM_BYTES, capacity=None, rows=True, cols=True, keep_offset=0, byte_offset=0, word_offset=0, seed=0):
        T, N = keep.shape
        self.T, self.N, self.keep = T, N, keep
        self.capacity = T * N if capacity is None else capacity
        rng = np.random.default_rng([seed, T, N])
        self.src = {f"{i}:{eb}": cr.plane_case(rng, T, N, eb) for i, eb in enumerate(planes)}
        self.want = cr.compact(keep, self.src, self.capacity)
        self.K = int(self.want[0][N])
        self.dev_keep = _offset(keep, keep_offset)
        self.dev_src = {k: _offset(v, byte_offset if v.dtype == np.uint8 else word_offset) for k, v in self.src.items()}
        self.out, self.whole = {}, {}
        self.out["start"], self.whole["start"] = fenced((N + 1,), torch.int64, _dev())
        for name, given in (("out_row", rows), ("out_col", cols)):
            self.out[name], self.whole[name] = fenced((self.capacity,), torch.int32, _dev()) if given else (None, None)
        for k, v in self.src.items():
            self.out[k], self.whole[k] = fenced((self.capacity,) + v.shape[2:], torch.uint8 if v.dtype == np.uint8 else torch.int32, _dev())
        def o(k):                                       # (an empty plane -- capacity 0 -- has no data_ptr(): the byte behind the leading guard)
            if self.out[k] is None:
                return None
            w = self.whole[k]
            return w.data_ptr() + (w.shape[0] - self.out[k].shape[0]) // 2 * (w[0].numel() * w.element_size())
        self.io = _abi.PhxTrajCompactIO(T=T, n_planes=len(self.src), N=N, capacity=self.capacity, keep=self.dev_keep.data_ptr(),
                                        start=o("start"), out_row=o("out_row"), out_col=o("out_col"))
        for i, (k, v) in enumerate(self.src.items()):
            self.io.plane[i] = _abi.PhxCompactPlane(src=self.dev_src[k].data_ptr(), dst=o(k), elem_bytes=int(k.split(":")[1]), reserved=0)

    def launch(self):
        return _abi.load_library().phx_traj_compact(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        start, out_row, out_col, dense = self.want
        n_out = min(self.K, self.capacity)
        assert_fences(self.whole["start"], self.N + 1, what + "start")
        np.testing.assert_array_equal(self.out["start"].cpu().numpy(), start, err_msg=what + "start")      # complete whatever the capacity
        for k, want in [("out_row", out_row), ("out_col", out_col)] + list(dense.items()):
            if self.out[k] is None:
                continue
            assert_fences(self.whole[k], self.capacity, what + k)
            got = self.out[k][:n_out].cpu().numpy()
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what}{k}: the first {n_out} elements differ"
            assert_poison(self.out[k][n_out:], f"{what}{k}: elements [{n_out}, {self.capacity})")
        # the inputs are byte-identical after the call
        assert self.dev_keep.cpu().numpy().tobytes() == self.keep.tobytes(), what + "keep"
        for k, v in self.src.items():
            assert self.dev_src[k].cpu().numpy().tobytes() == v.tobytes(), what + k

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k, w in self.whole.items():
            if w is not None:
                assert_poison(w, f"{what}: {k}")


def _keep(T, N, density, seed=0):
    return cr.keep_case(np.random.default_rng([seed, T, N, cr.DENSITIES.index(density)]), T, N, density)


def _run(T, N, density, seed=0, **kw):
    call = Call(_keep(T, N, density, seed), seed=seed, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} {density} {sorted(kw.items())}: ")
    return call


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    for T in TS:
        for density in cr.DENSITIES:                    # (planes of 1, 4, 12 and 20 bytes in every call; capacity > K: poison stays behind K)
            call = _run(T, N, density, capacity=T * N + 5)
            assert call.K < call.capacity and (call.K == T * N) == (density == "all" or (call.keep != 0).all())


def test_columns_beyond_one_block_of_the_scan():
    for density in ("random 0.5", "alternating", "all"):
        _run(3, SB + 65, density)                       # two blocks of the scan (the second one short), 66 tiles of the scatter
    _run(2, 2 * SB, "random 0.9", planes=(4,))          # N a multiple of the block: start[N] is the third block's only entry


def test_wide_elements():
    for eb in (8, 128, 132, 256):                       # w = 2, 32, 33 (one element per store instruction from here on), 64
        _run(R + 1, CW + 1, "random 0.5", planes=(eb,))


def test_capacity_clips_the_stores_and_nothing_else():
    for T, N in ((R + 1, CW + 1), (5, 4 * CW + 1)):
        K = int((_keep(T, N, "random 0.5") != 0).sum())
        assert K > 2
        for cap in (K - 1, K // 2, 0, K, K + 1):
            call = _run(T, N, "random 0.5", capacity=cap)
            assert call.K == K


def test_plane_counts_and_the_optional_index_outputs():
    lib = _abi.load_library()
    for rows in (False, True):
        for cols in (False, True):
            _run(R + 1, CW + 1, "random 0.5", rows=rows, cols=cols)
            assert lib.phx_last_kernel() == _abi.COMPACT_KERNELS.encode()
            _run(R + 1, CW + 1, "alternating", planes=(), rows=rows, cols=cols)         # n_planes = 0: counts and offsets (and the indices)
            assert lib.phx_last_kernel() == (_abi.COMPACT_KERNELS if rows or cols else _abi.COMPACT_COUNT_KERNEL + "+" + _abi.COMPACT_SCAN_KERNEL).encode()
    sixteen = (1, 4, 12, 20) * 4
    assert len(sixteen) == _abi.COMPACT_MAX_PLANES
    _run(R + 1, 2 * CW + 1, "random 0.5", planes=sixteen)
    _run(3, 5, "random 0.5", planes=sixteen, rows=False, cols=False)


@pytest.mark.parametrize("keep_offset,byte_offset,word_offset", [(1, 3, 4), (7, 1, 12)])
def test_inputs_that_are_row_slices_of_a_longer_recording(keep_offset, byte_offset, word_offset):
    for T, N in ((R + 1, CW + 1), (3, 4 * CW + 1), (5, 3)):
        _run(T, N, "random 0.5", keep_offset=keep_offset, byte_offset=byte_offset, word_offset=word_offset)


def test_reduction_against_the_input_planes():
    """every keep byte non-zero: each dst is the [N][T] transpose of its src, start[n] = n * T, out_row cycles 0 .. T - 1"""
    T, N = R + 1, 2 * CW + 1
    call = _run(T, N, "all")
    assert call.K == T * N
    assert bool((call.out["start"] == torch.arange(N + 1, device=_dev()) * T).all())
    assert bool((call.out["out_row"].view(N, T) == torch.arange(T, device=_dev(), dtype=torch.int32)).all())
    assert bool((call.out["out_col"].view(N, T) == torch.arange(N, device=_dev(), dtype=torch.int32)[:, None]).all())
    for k, src in call.dev_src.items():
        assert bool((call.out[k].view((N, T) + tuple(src.shape[2:])) == src.movedim(0, 1)).all()), k
    words = call.out["3:20"].cpu().numpy().view(np.uint32)
    assert (words == 0x80000000).any() and (words == 0x7fc00001).any() and (words == 0xff800001).any()      # -0.0 and NaN payloads survive


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _abi.load_library()
    call = Call(_keep(R + 1, CW + 1, "random 0.5", seed=1), seed=1)
    scalars = ("T", "n_planes", "N", "capacity", "keep", "start", "out_row", "out_col")
    good = {n: getattr(call.io, n) for n in scalars}
    good_planes = [(p.src, p.dst, p.elem_bytes, p.reserved) for p in call.io.plane]

    def restore():
        for n, v in good.items():
            setattr(call.io, n, v)
        for i, (src, dst, eb, res) in enumerate(good_planes):
            call.io.plane[i] = _abi.PhxCompactPlane(src=src, dst=dst, elem_bytes=eb, reserved=res)

    def refused(what, plane=None, **patch):
        restore()
        for k, v in patch.items():
            target = call.io if plane is None else call.io.plane[plane]
            setattr(target, k, v(getattr(target, k)) if callable(v) else v)
        assert call.launch() == EINVAL, what
        assert b"phx_traj_compact" in lib.phx_last_error(), what
        call.check_untouched(what)

    refused("keep NULL", keep=None)
    refused("start NULL", start=None)
    for k, bad in (("T", 0), ("T", -3), ("N", 0), ("N", -1), ("n_planes", -1), ("n_planes", 17), ("capacity", -1)):
        refused(f"{k} = {bad}", **{k: bad})
    refused("N beyond one launch's grid", N=CW * 0x7fffffff + 1, out_col=None)
    refused("out_col with N > 2^31 - 1", N=1 << 31)
    for i in (0, 3):
        refused(f"plane {i} src NULL", plane=i, src=None)
        refused(f"plane {i} dst NULL", plane=i, dst=None)
        refused(f"plane {i} reserved", plane=i, reserved=1)
        refused(f"plane {i} dst off a 16-byte boundary", plane=i, dst=lambda p: p + 4)
        for bad in (0, -4, 2, 3, 6, 260, 1 << 20):
            refused(f"plane {i} elem_bytes = {bad}", plane=i, elem_bytes=bad)
    refused("a word plane's src off a 4-byte boundary", plane=1, src=lambda p: p + 2)
    for k in ("start", "out_row", "out_col"):
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    assert lib.phx_traj_compact(None, None) == EINVAL and b"phx_traj_compact" in lib.phx_last_error()
    restore()                                           # and the same buffers receive a good call
    assert call.launch() == 0, lib.phx_last_error()
    call.check("after the refusals: ")


def test_last_kernel_names_the_kernels():
    lib = _abi.load_library()
    _run(3, 7, "random 0.5")
    assert lib.phx_last_kernel() == b"phx_compact_count_kernel+phx_compact_scan_kernel+phx_compact_scatter_kernel"
    _run(3, 7, "random 0.5", capacity=0)                # nothing to write: no scatter
    assert lib.phx_last_kernel() == b"phx_compact_count_kernel+phx_compact_scan_kernel"
    _run(3, 7, "none")
    assert lib.phx_last_kernel() == _abi.COMPACT_KERNELS.encode()


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(_keep(2 * R + 1, 4 * CW + 1, "random 0.5", seed=11), seed=11)
    b = Call(_keep(R - 1, 2 * CW + 2, "alternating", seed=12), planes=(20, 1), cols=False, seed=12)
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
# 8-step episodes: the shops of the FSM supply chain act in RESTOCK steps (even t); T = 20 crosses two episode boundaries
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


def _critic(x):
    return 0.5 * x[:, 0] - 0.25 * torch.tanh(x[:, 1]) + 0.125 * x[:, -1] * x[:, -1] + 0.75


def test_device_env_compact_on_a_real_rollout():
    env = _fsm_env()
    tr = env.rollout(STEPS)
    dev = env._device()
    keep = tr.obs_valid
    n = STEPS * B * S
    planes = {"obs": tr.observations, "rewards": tr.rewards, "truncations": tr.truncations,
              "index": torch.arange(n, dtype=torch.int32, device=dev.device).view(STEPS, B, S)}
    start, out_row, out_col, dense = dev.compact(keep, planes)
    assert dev.last_kernel() == _abi.COMPACT_KERNELS
    K = int(start[-1])
    assert 0 < K < n and K == int((keep != 0).sum())
    flat = lambda x: x.reshape((STEPS, B * S) + tuple(x.shape[3:]))
    mask = flat(keep).movedim(0, 1) != 0
    assert start.dtype == torch.int64 and out_row.dtype == out_col.dtype == torch.int32 and tuple(out_row.shape) == tuple(out_col.shape) == (n,)
    assert bool((start[1:] - start[:-1] == mask.sum(dim=1)).all()) and int(start[0]) == 0
    for name, x in planes.items():
        want = flat(x).movedim(0, 1)[mask]
        assert dense[name].dtype == x.dtype and tuple(dense[name].shape) == (n,) + tuple(x.shape[3:])
        assert bool((dense[name][:K].view(torch.int32 if x.dtype != torch.uint8 else torch.uint8) ==
                     want.view(torch.int32 if x.dtype != torch.uint8 else torch.uint8)).all()), name
    assert bool((out_row[:K].long() * (B * S) + out_col[:K].long() == dense["index"][:K].long()).all())
    # caller-owned outputs, a smaller capacity, [T, N] views, no index outputs
    cap = K - 3
    outs = {"start": fenced((B * S + 1,), torch.int64, dev.device), "rewards": fenced((cap,), torch.float32, dev.device),
            "obs": fenced((cap, 3), torch.float32, dev.device)}
    two = {"rewards": flat(tr.rewards), "obs": flat(tr.observations)}
    out = (outs["start"][0], None, None, {k: outs[k][0] for k in two})
    # refusals at this level leave caller-owned outputs untouched
    for name, bad_keep, bad_planes in (("keep", keep.to(torch.int32), two), ("keep", flat(keep).cpu(), two),
                                       ("rewards", flat(keep), dict(two, rewards=two["rewards"][:-1])),
                                       ("rewards", flat(keep), dict(two, rewards=two["rewards"].double())),
                                       ("obs", flat(keep), dict(two, obs=two["obs"].to(torch.uint8)))):
        with pytest.raises(ValueError, match=name):
            dev.compact(bad_keep, bad_planes, cap, out=out)
    with pytest.raises(ValueError, match="capacity"):
        dev.compact(flat(keep), two, -1, out=out)
    with pytest.raises(ValueError, match="out"):
        dev.compact(flat(keep), two, cap, out=(out[0], None, None, {"rewards": out[3]["rewards"]}))
    with pytest.raises(ValueError, match=r"out\[0\]"):
        dev.compact(flat(keep), two, cap, out=(out[0][:-1], None, None, out[3]))
    torch.cuda.synchronize()
    for k, (_, whole) in outs.items():
        assert_poison(whole, f"a refused DeviceEnv.compact call: {k}")
    res = dev.compact(flat(keep), two, cap, out=out)
    assert res[0].data_ptr() == out[0].data_ptr() and res[1] is None and res[2] is None
    assert bool((res[0] == start).all())
    for k in two:
        assert_fences(outs[k][1], cap, k)
        assert bool((res[3][k].view(torch.int32) == dense[k][:cap].view(torch.int32)).all()), k
    assert_fences(outs["start"][1], B * S + 1, "start")
    # more than 16 planes: further launches, the same results
    many = {f"p{i}": (two["obs"] if i % 2 else two["rewards"]) for i in range(19)}
    r19 = dev.compact(flat(keep), many)
    assert bool((r19[0] == start).all()) and bool((r19[1][:K] == out_row[:K]).all()) and bool((r19[2][:K] == out_col[:K]).all())
    for i in range(19):
        ref = dense["obs" if i % 2 else "rewards"]
        assert bool((r19[3][f"p{i}"][:K].view(torch.int32) == ref[:K].view(torch.int32)).all()), i


MAPPINGS = (None, lambda aid: str(aid))


@pytest.mark.parametrize("with_critic", [False, True])
@pytest.mark.parametrize("make", [_fsm_env, _stk_env])
def test_sample_compact_gives_the_sample_batches_of_sample(make, with_critic):
    env, twin = make(), make()
    kw = dict(value_fn=_critic, gamma=0.99, lambda_=0.95) if with_critic else {}
    buffers = None
    for call in range(2):                               # the second call continues the episodes and reuses the kept buffers
        frag = env.sample(T, compact=True, **kw)
        assert env._device().last_kernel() == _abi.COMPACT_KERNELS
        batch = twin.sample(T, **kw)
        assert isinstance(frag, CompactFragment) and isinstance(batch, FragmentBatch)
        assert (frag.B, frag.S, frag.T) == (batch.B, batch.S, batch.T) and frag.agent_ids == batch.agent_ids
        assert 0 < frag.K < T * frag.B * frag.S and frag.K == int((batch.obs_valid != 0).sum())      # a fragment with holes
        assert len(np.unique(batch.eps_id[0])) >= 3                                                   # T crosses episode boundaries
        np.testing.assert_array_equal(frag.col_start[1:] - frag.col_start[:-1], (batch.obs_valid != 0).sum(axis=2).reshape(-1))
        np.testing.assert_array_equal(frag.t, batch.t)
        np.testing.assert_array_equal(frag.eps_id, batch.eps_id)
        for fn in MAPPINGS:
            cr.assert_same_batches(frag.to_sample_batches(fn), batch.to_sample_batches(fn), f"call {call}: ")
        assert ("vf_preds" in frag.columns) == with_critic
        held = {k: (d.data_ptr(), h.data_ptr()) for k, (d, h) in env._compact_bufs.items()}
        assert buffers is None or held == buffers
        buffers = held
    # the same columns through the RLlib adapter (same seed, fresh envs)
    adapter = ph.rllib.BatchedBaseEnv(make()).sample(T, compact=True, **kw)
    cr.assert_same_batches(adapter, ph.rllib.BatchedBaseEnv(make()).sample(T, **kw), "BatchedBaseEnv: ")


def test_compact_is_refused_where_it_does_not_apply():
    env = _plain_env()
    with pytest.raises(ValueError, match="compact"):
        env.sample(T, compact=True)
    batch = env.sample(T, value_fn=_critic, gamma=0.99, lambda_=0.95)       # and a plain env's sample() is what it was
    assert isinstance(batch, FragmentBatch) and env._device().last_kernel() == "phx_gae_kernel"
    cols = batch.to_sample_batches()["default_policy"]
    assert set(cols) == {"obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "eps_id", "agent_index", "t", "env_id",
                         "vf_preds", "advantages", "value_targets"}
    twin = _plain_env()
    cr.assert_same_batches(batch.to_sample_batches(), twin.sample(T, value_fn=_critic, gamma=0.99, lambda_=0.95, compact=False).to_sample_batches())
    fsm = _fsm_env()
    with pytest.raises(ValueError, match="policy"):
        fsm.sample(T, compact=True, policy=object())
    with pytest.raises(ValueError, match="target_logp_fn"):
        fsm.sample(T, compact=True, target_logp_fn=lambda o, a: a)
