"""phx_train_batch (include/phantom_amd_batch.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the
numpy restatement (tests/batch_ref.py) of start, records, out_row, out_col and moments over row counts around the scatter's chunk
depth, column counts around its tile width and one beyond the scan's block, K on both sides of powers of 4, byte and word planes,
record sizes 4 .. 256 words with gaps, keep = NULL, classes, both shuffle settings and the standardized plane; the capacity rule,
row slices at odd offsets, every refusal, phx_last_kernel, two calls on one stream; then DeviceEnv.train_batch on a real FSM rollout."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_ref as br
import compact_ref as cr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, fenced
from helpers import market_env, supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import DeviceBatch

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_train_batch.hip")).read()
R = int(re.search(r"constexpr int BT_R = (\d+);", SRC).group(1))                  # the scatter's chunk depth (rows)
CW = int(re.search(r"constexpr int BT_C = (\d+);", SRC).group(1))                 # the scatter's tile width (columns)
SB = int(re.search(r"constexpr int BT_SB = (\d+);", SRC).group(1))                # the scan's block (entries)
TS = (1, R - 1, R, R + 1, 2 * R + 1)
NS = (1, CW - 1, CW, CW + 1, 4 * CW + 1)
EINVAL = -1
# elem_bytes, word_offs (None: packed in order), row_words (None: the default); with a standardized plane, a 4-byte one appended:
# its word_off and the row_words then
LAYOUTS = {"packed": ((1, 4, 12, 20), None, None, None, None),
           "lone byte": ((1,), (0,), 4, 5, 8),
           "gaps": ((1, 4, 12, 20), (2, 17, 5, 9), 20, 15, 20),             # words 0-1, 3-4, 8, 14-16, 18-19 belong to no plane
           "widest": ((4, 1, 256, 12, 20), (250, 255, 3, 70, 100), 256, 0, 256)}

def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _offset(host, nbytes):
    """`host` on the device, starting `nbytes` bytes past a 16-byte boundary (0: on one)"""
    a = np.ascontiguousarray(host)
    a = a if a.dtype == np.uint8 else a.view(np.int32)
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device=_dev())
    assert raw.data_ptr() % 16 == 0
    x = raw[nbytes:nbytes + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    x.copy_(torch.from_numpy(a))
    assert x.data_ptr() % 16 == nbytes
    return x


def _std_source(rng, keep_mask, T, N):
    """f32 3 * N(0, 1) + 1 as u32 bit patterns; what is not kept may hold anything: a NaN and an infinity where there is room"""
    x = (3.0 * rng.standard_normal((T, N)) + 1.0).astype(np.float32)
    holes = np.argwhere(~keep_mask)
    for (t, n), bad in zip(holes[:2], (np.nan, np.inf)):
        x[t, n] = bad
    return x.view(np.uint32)


class Call:
    """one phx_train_batch call: device inputs, fenced and poisoned outputs, the restatement's result in `want`"""

    def __init__(self, T, N, keep, layout="packed", std=False, shuffle=1, seed=0, epoch=0, col_class=None, class_id=0, capacity=None, rows=True,
                 cols=True, keep_offset=0, byte_offset=0, word_offset=0, case=0):
        self.T, self.N, self.keep = T, N, keep
        elem_bytes, offs, row_words, std_off, std_row_words = LAYOUTS[layout]
        if offs is None:
            offs, row_words = br.default_layout(elem_bytes + ((4,) if std else ()))
        elif std:
            offs, row_words = list(offs) + [std_off], std_row_words
        self.row_words, self.offs = row_words, offs
        self.capacity = T * N + 3 if capacity is None else capacity
        rng = np.random.default_rng([case, T, N])
        mask = br.kept_mask(T, N, keep, col_class, class_id)
        self.src = [cr.plane_case(rng, T, N, eb) for eb in elem_bytes] + ([_std_source(rng, mask, T, N)] if std else [])
        self.elem_bytes = list(elem_bytes) + ([4] if std else [])
        self.std_plane = len(self.src) - 1 if std else -1
        self.kw = dict(keep=keep, col_class=col_class, class_id=class_id, shuffle=shuffle, seed=seed, epoch=epoch, std_plane=self.std_plane)
        self.want = br.train_batch(T, N, list(zip(self.src, offs)), row_words, capacity=self.capacity, **self.kw)
        self.K = self.want["K"]
        self.dev_keep = None if keep is None else _offset(keep, keep_offset)
        self.dev_class = None if col_class is None else _offset(np.asarray(col_class, np.uint8), 1)
        self.dev_src = [_offset(v, byte_offset if v.dtype == np.uint8 else word_offset) for v in self.src]
        i32, u8 = torch.int32, torch.uint8
        shapes = {"start": ((N + 1,), torch.int64), "records": ((self.capacity, row_words), i32),
                  "out_row": ((self.capacity,), i32) if rows else None, "out_col": ((self.capacity,), i32) if cols else None,
                  "moments": ((32,), u8) if std else None, "workspace": ((16 * N,), u8) if std else None}
        self.out, self.whole = {}, {}
        for k, sd in shapes.items():
            self.out[k], self.whole[k] = fenced(sd[0], sd[1], _dev()) if sd else (None, None)

        def o(k):                                       # (an empty buffer has no data_ptr(): the byte behind the leading guard)
            if self.out[k] is None:
                return None
            w = self.whole[k]
            return w.data_ptr() + (w.shape[0] - self.out[k].shape[0]) // 2 * (w[0].numel() * w.element_size())
        p = lambda x: None if x is None else x.data_ptr()
        self.io = _abi.PhxTrainBatchIO(T=T, N=N, capacity=self.capacity, n_planes=len(self.src), row_words=row_words,
                                       S=1 if col_class is None else len(col_class), class_id=class_id, std_plane=self.std_plane, shuffle=shuffle,
                                       seed=seed, epoch=epoch, keep=p(self.dev_keep), col_class=p(self.dev_class),
                                       **{k: o(k) for k in shapes})
        for i, eb in enumerate(self.elem_bytes):
            self.io.plane[i] = _abi.PhxBatchPlane(src=self.dev_src[i].data_ptr(), elem_bytes=eb, word_off=offs[i])

    def launch(self):
        return _abi.load_library().phx_train_batch(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        w = self.want
        for k, whole in self.whole.items():
            if whole is not None:
                assert_fences(whole, self.out[k].shape[0], what + k)
        np.testing.assert_array_equal(self.out["start"].cpu().numpy(), w["start"], err_msg=what + "start")
        if self.std_plane >= 0:
            got = self.out["moments"].cpu().numpy().view(br.MOMENTS_DTYPE)[0]
            assert got.tobytes() == w["moments"].tobytes(), f"{what}moments: {got} != {w['moments']}"
        n_out = self.K if self.K <= self.capacity else 0          # (K > capacity: nothing but start and moments is written)
        for k in ("records", "out_row", "out_col"):
            if self.out[k] is None:
                continue
            if n_out:
                got = self.out[k][:n_out].cpu().numpy()
                bad = np.flatnonzero((got.view(np.uint32) != w[k].view(np.uint32)).reshape(n_out, -1).any(axis=1))
                assert bad.size == 0, f"{what}{k}: {bad.size} of {n_out} records differ, first at {bad[:5]}"
            assert_poison(self.out[k][n_out:], f"{what}{k}: records [{n_out}, {self.capacity})")
        if self.dev_keep is not None:                           # the inputs are byte-identical after the call
            assert self.dev_keep.cpu().numpy().tobytes() == self.keep.tobytes(), what + "keep"
        for i, v in enumerate(self.src):
            assert self.dev_src[i].cpu().numpy().tobytes() == v.tobytes(), f"{what}plane {i}"

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k, w in self.whole.items():
            if w is not None:
                assert_poison(w, f"{what}: {k}")


def _keep(T, N, density, seed=0):
    return cr.keep_case(np.random.default_rng([seed, T, N, cr.DENSITIES.index(density)]), T, N, density)


def _keep_exactly(T, N, K, seed=0):
    """a keep plane with exactly K kept elements, anywhere"""
    rng = np.random.default_rng([seed, T, N, K])
    k = np.zeros(T * N, np.uint8)
    k[rng.permutation(T * N)[:K]] = rng.integers(1, 256, K)
    return k.reshape(T, N)


def _run(T, N, keep, **kw):
    call = Call(T, N, keep, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} {sorted((k, v) for k, v in kw.items() if k != 'col_class')}: ")
    return call


# the rest of the parameter space, walked along the (T, density) grid of every N
CONFIGS = (dict(layout="packed", std=False, shuffle=1), dict(layout="packed", std=True, shuffle=1), dict(layout="lone byte", shuffle=1),
           dict(layout="gaps", std=True, shuffle=0), dict(layout="widest", std=True, shuffle=1), dict(layout="gaps", shuffle=1),
           dict(layout="packed", std=True, shuffle=0), dict(layout="widest", shuffle=0), dict(layout="lone byte", std=True, shuffle=1))


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    i = NS.index(N)
    for T in TS:
        for density in cr.DENSITIES:
            for cfg in (CONFIGS[i % len(CONFIGS)], CONFIGS[(i + 4) % len(CONFIGS)]):
                call = _run(T, N, _keep(T, N, density), seed=0xDEADBEEF12345678 + i, epoch=i, case=i, **cfg)
                assert call.K <= T * N < call.capacity
                i += 1


def test_k_on_both_sides_of_powers_of_four():
    """w, h and the mask change where K passes a power of 4: keep planes with exactly that many kept elements"""
    for T, N in ((2 * R + 1, 4 * CW + 1), (R + 1, CW + 1)):
        for j in range(1, 7):
            for K in (4 ** j - 1, 4 ** j, 4 ** j + 1):
                if K <= T * N:
                    call = _run(T, N, _keep_exactly(T, N, K), layout="packed", std=(j % 2 == 0), seed=j, epoch=K)
                    assert call.K == K
    for K in (0, 1, 2):
        _run(R + 1, CW + 1, _keep_exactly(R + 1, CW + 1, K), std=True, seed=3)


def test_keep_null_keeps_everything():
    for T, N in ((1, 1), (R + 1, CW + 1), (2 * R + 1, 4 * CW + 1)):
        for cfg in CONFIGS[:4]:
            assert _run(T, N, None, seed=T, **cfg).K == T * N


def test_classes_select_their_columns():
    classes = np.array([0, 1, 0], np.uint8)                      # S = 3: agents 0 and 2 share a policy
    for N in (3, CW - 1, 4 * CW + 2):
        for T in (1, R + 1):
            total = 0
            for class_id in (0, 1, 2):
                for keep in (None, _keep(T, N, "random 0.5")):
                    call = _run(T, N, keep, std=True, col_class=classes, class_id=class_id, seed=7, epoch=class_id)
                total += call.K
                assert class_id != 2 or call.K == 0               # a class no column belongs to
            assert total == int((keep != 0).sum())               # the classes partition the kept elements
    three = np.array([2, 0, 1], np.uint8)
    assert sum(_run(R, 3 * CW, None, col_class=three, class_id=c).K for c in range(3)) == R * 3 * CW


def test_a_permutation_cannot_be_clipped():
    for T, N in ((R + 1, CW + 1), (5, 4 * CW + 1)):
        K = int((_keep(T, N, "random 0.5") != 0).sum())
        assert K > 2
        for cap in (K - 1, K // 2, 0, K, K + 1):
            for std in (False, True):
                call = _run(T, N, _keep(T, N, "random 0.5"), std=std, capacity=cap, seed=9)
                assert call.K == K and (call.want["records"] is None) == (cap < K)


def test_optional_outputs_and_last_kernel():
    lib = _abi.load_library()
    T, N = R + 1, CW + 1
    for rows in (False, True):
        for cols in (False, True):
            _run(T, N, _keep(T, N, "random 0.5"), rows=rows, cols=cols, std=True)
            assert lib.phx_last_kernel() == _abi.BATCH_KERNELS.encode()
    _run(T, N, _keep(T, N, "random 0.5"))
    assert lib.phx_last_kernel() == b"phx_batch_count_kernel+phx_batch_scan_kernel+phx_batch_scatter_kernel"
    _run(T, N, _keep(T, N, "random 0.5"), capacity=0, std=True)           # nothing to write: no scatter
    assert lib.phx_last_kernel() == b"phx_batch_count_kernel+phx_batch_scan_kernel+phx_batch_moments_kernel"
    _run(T, N, _keep(T, N, "none"), capacity=0)
    assert lib.phx_last_kernel() == b"phx_batch_count_kernel+phx_batch_scan_kernel"
    call = Call(T, N, _keep(T, N, "alternating"))                         # n_planes = 0 without records: the indices alone
    call.io.n_planes, call.io.records = 0, None
    assert call.launch() == 0, lib.phx_last_error()
    torch.cuda.synchronize()
    assert_poison(call.whole["records"], "records were not given")
    call.whole["records"] = call.out["records"] = None
    call.check("n_planes = 0: ")


@pytest.mark.parametrize("keep_offset,byte_offset,word_offset", [(1, 3, 4), (7, 1, 12)])
def test_inputs_that_are_row_slices_of_a_longer_recording(keep_offset, byte_offset, word_offset):
    for T, N in ((R + 1, CW + 1), (3, 4 * CW + 1), (5, 3)):
        for cfg in (CONFIGS[1], CONFIGS[4]):
            _run(T, N, _keep(T, N, "random 0.5"), keep_offset=keep_offset, byte_offset=byte_offset, word_offset=word_offset, **cfg)


def test_columns_beyond_one_block_of_the_scan():
    for density in ("random 0.5", "alternating"):
        _run(3, SB + 65, _keep(3, SB + 65, density), std=True, seed=5)
    _run(2, 2 * SB, _keep(2, 2 * SB, "random 0.9"), layout="lone byte")


def test_special_words_survive():
    T, N = R + 1, 2 * CW + 1
    call = _run(T, N, None, layout="packed", shuffle=1, seed=1)
    words = call.out["records"][:call.K].cpu().numpy().view(np.uint32)
    assert all((words == s).any() for s in cr.SPECIAL_WORDS)
    assert (words[:, 10:] == 0).all()                            # the words behind the last plane


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(2 * R + 1, 4 * CW + 1, _keep(2 * R + 1, 4 * CW + 1, "random 0.5", seed=11), std=True, seed=11)
    b = Call(R - 1, 2 * CW + 2, _keep(R - 1, 2 * CW + 2, "alternating", seed=12), layout="gaps", cols=False, seed=12)
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _abi.load_library()
    T, N = R + 1, 3 * CW                                # (N % 3 == 0: S = 3 is a good value to start from)
    call = Call(T, N, _keep(T, N, "random 0.5", seed=1), std=True, col_class=np.array([0, 0, 0], np.uint8), seed=1)
    names = [n for n, _ in _abi.PhxTrainBatchIO._fields_ if n not in ("plane", "reserved")]
    good = {n: getattr(call.io, n) for n in names}
    good_planes = [(p.src, p.elem_bytes, p.word_off) for p in call.io.plane]

    def restore():
        for n, v in good.items():
            setattr(call.io, n, v)
        call.io.reserved[0] = call.io.reserved[1] = 0
        for i, (src, eb, off) in enumerate(good_planes):
            call.io.plane[i] = _abi.PhxBatchPlane(src=src, elem_bytes=eb, word_off=off)

    def refused(what, plane=None, **patch):
        restore()
        for k, v in patch.items():
            target = call.io if plane is None else call.io.plane[plane]
            setattr(target, k, v(getattr(target, k)) if callable(v) else v)
        assert call.launch() == EINVAL, what
        assert b"phx_train_batch" in lib.phx_last_error(), what
        call.check_untouched(what)

    refused("start NULL", start=None)
    refused("records NULL with planes", records=None)
    for k, bad in (("T", 0), ("T", -3), ("T", 1 << 31), ("N", 0), ("N", -1), ("S", 0), ("S", -1), ("S", 5), ("S", N + 3), ("n_planes", -1),
                   ("n_planes", 33), ("capacity", -1), ("row_words", 0), ("row_words", 8), ("row_words", 18), ("row_words", 260),
                   ("std_plane", -2), ("std_plane", 5), ("std_plane", 0), ("std_plane", 2), ("shuffle", 2), ("shuffle", -1)):
        refused(f"{k} = {bad}", **{k: bad})
    refused("T * N > 2^62", T=(1 << 31) - 1, N=3 << 31, out_col=None)
    refused("N beyond one launch's grid", N=3 * ((CW * 0x7fffffff) // 3 + 1), out_col=None)
    refused("out_col with N > 2^31 - 1", N=3 << 30)
    refused("moments NULL with std_plane", moments=None)
    refused("workspace NULL with std_plane", workspace=None)
    for r in (0, 1):
        restore()
        call.io.reserved[r] = 1
        assert call.launch() == EINVAL and b"phx_train_batch" in lib.phx_last_error()
        call.check_untouched(f"reserved[{r}]")
    for i in (0, 3):
        refused(f"plane {i} src NULL", plane=i, src=None)
        for bad in (0, -4, 2, 3, 6, 260, 1 << 20):
            refused(f"plane {i} elem_bytes = {bad}", plane=i, elem_bytes=bad)
        refused(f"plane {i} before the record", plane=i, word_off=-1)
        refused(f"plane {i} beyond the record", plane=i, word_off=call.row_words - (0 if i == 0 else 4))
    refused("plane 2 overlaps plane 3", plane=2, word_off=call.offs[3] - 1)
    refused("plane 0 overlaps plane 1", plane=0, word_off=call.offs[1])
    refused("a word plane's src off a 4-byte boundary", plane=1, src=lambda p: p + 2)
    for k in ("start", "records", "out_row", "out_col", "moments", "workspace"):
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    assert lib.phx_train_batch(None, None) == EINVAL and b"phx_train_batch" in lib.phx_last_error()
    restore()                                           # and the same buffers receive a good call
    assert call.launch() == 0, lib.phx_last_error()
    call.check("after the refusals: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
T_E2E = 20                                               # crosses two episode boundaries of the envs below


def _fsm_env(seed=5):
    env = supply_chain_env(5, [3] * 5, 8, 4, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


def _stk_env(seed=5):
    env = market_env(2, 3, 2, 6, 4, seed=seed, exogenous="device")
    env.reset()
    return env


def _plain_env(seed=5):
    env = supply_chain_env(9, [6] * 9, 7, 8, seed=seed, exogenous="device")
    env.reset()
    return env


def _critic(x):
    return 0.5 * x[:, 0] - 0.25 * torch.tanh(x[:, 1]) + 0.125 * x[:, -1] * x[:, -1] + 0.75


def _policy():
    rng = np.random.default_rng(2)
    ws = [rng.normal(0, 0.7, (16, 3)).astype(np.float32), rng.normal(0, 0.3, (2, 16)).astype(np.float32)]
    bs = [rng.normal(0, 0.3, (16,)).astype(np.float32), np.array([0.1, -0.5], np.float32)]
    return ph.MLPPolicy(ws, bs, activation="relu", out_scale=50.0, out_bias=50.0, out_lo=0.0, out_hi=100.0)


def _bits(x):
    a = np.ascontiguousarray(x)
    return a.view(np.uint8) if a.dtype == np.bool_ else a


def _by_col_row(db):
    """the order that sorts a DeviceBatch's records by (column, row): to_sample_batches()'s row order"""
    return np.lexsort((db.row.cpu().numpy(), db.col.cpu().numpy()))


@pytest.mark.parametrize("make,kw", [(_fsm_env, dict(value_fn=_critic, gamma=0.99, lambda_=0.95)),
                                     (_stk_env, dict(value_fn=_critic, gamma=0.99, lambda_=0.95, n_step=3)),
                                     (_plain_env, dict(policy="policy", explore=True, value_fn=_critic, gamma=0.99, lambda_=0.95))],
                         ids=["fsm", "stackelberg", "plain"])
def test_sample_with_a_batcher_gives_the_sample_batches_on_the_device(make, kw):
    env, twin = make(), make()
    if kw.get("policy"):
        kw = dict(kw, policy=_policy())
    ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
    fn = lambda aid: "even" if ids.index(aid) % 2 == 0 else "odd"
    tb = ph.TrainBatcher(env, seed=0xDEADBEEF12345678, policy_mapping_fn=fn)
    st, st_twin = ph.EpisodeStats(env), ph.EpisodeStats(twin)
    masked = make is not _plain_env
    B, S = env.batch_size, env.spec.n_strategic
    for call in range(2):                                   # the second call continues the episodes under the next epoch
        got = env.sample(T_E2E, batcher=tb, episode_stats=st, **kw)
        assert env._device().last_kernel() == _abi.BATCH_KERNELS and tb.calls == call + 1
        batch = twin.sample(T_E2E, episode_stats=st_twin, **kw)
        want = batch.to_sample_batches(fn)
        assert set(got) == set(want) == {"even", "odd"}
        keep = None if not masked else np.ascontiguousarray(np.moveaxis(batch.obs_valid, 2, 0)).reshape(T_E2E, B * S)
        adv = np.ascontiguousarray(np.moveaxis(batch.advantages, 2, 0)).reshape(T_E2E, B * S)
        for c, pid in enumerate(tb.policies):
            db = got[pid]
            assert isinstance(db, DeviceBatch) and db.epoch == call and db.standardized == "advantages"
            assert masked or db._count is not None          # a plain env's count is known without a wait
            K = db.count
            assert K == len(want[pid]["obs"]) and (not masked or 0 < K < db.records.shape[0])
            order = _by_col_row(db)
            cols = db.columns
            device_names = set(want[pid]) - {"eps_id", "agent_index", "t", "env_id", "action_prob"}
            assert set(cols) == device_names, set(cols) ^ device_names
            for name in device_names - {"advantages"}:
                g, w = cols[name].cpu().numpy()[order], want[pid][name]
                assert g.dtype == w.dtype and g.shape == w.shape, (pid, name, g.dtype, w.dtype, g.shape, w.shape)
                assert _bits(g).tobytes() == _bits(w).tobytes(), (call, pid, name)
            col = db.col.cpu().numpy()[order]
            np.testing.assert_array_equal(col // S, want[pid]["env_id"])
            np.testing.assert_array_equal(col % S, want[pid]["agent_index"])
            np.testing.assert_array_equal(batch.t[col // S, db.row.cpu().numpy()[order]], want[pid]["t"])
            # advantages: the restatement's standardized values, and with them the shuffle and the moments, bit for bit
            ref = br.train_batch(T_E2E, B * S, [(adv.view(np.uint32), 0)], 4, keep=keep, col_class=tb.col_class, class_id=c, shuffle=1,
                                 seed=tb.seed, epoch=call, std_plane=0)
            assert ref["K"] == K and db.moments.cpu().numpy().tobytes() == ref["moments"].tobytes()
            assert cols["advantages"].cpu().numpy().view(np.uint32).tobytes() == ref["records"][:, 0].tobytes(), (call, pid)
            np.testing.assert_array_equal(db.row.cpu().numpy(), ref["out_row"])
            np.testing.assert_array_equal(db.col.cpu().numpy(), ref["out_col"])
            sizes = [len(mb["obs"]) for mb in db.minibatches(7)]
            assert sum(sizes) == K and all(n == 7 for n in sizes[:-1]) and [len(mb["obs"]) for mb in db.minibatches(7, drop_last=True)] == [7] * (K // 7)
            if c == 0:                                      # the next epoch's order: a permutation of the same records
                before = tb.calls
                again = tb.reshuffle(db)
                assert tb.calls == before + 1 and again.epoch == before and again.count == K
                assert again.records.data_ptr() != db.records.data_ptr()
                o2 = _by_col_row(again)
                assert (again.records[:K].cpu().numpy()[o2] == db.records[:K].cpu().numpy()[order]).all()
                assert K < 8 or (again.row.cpu().numpy() != db.row.cpu().numpy()).any() or (again.col.cpu().numpy() != db.col.cpu().numpy()).any()
                tb.calls = before                           # (the twin comparison below counts sample() calls as epochs)
    np.testing.assert_equal(st.result(), st_twin.result())
    plain = {k: v for k, v in kw.items() if k != "n_step"}
    cr.assert_same_batches(env.sample(T_E2E, **plain).to_sample_batches(fn), twin.sample(T_E2E, **plain).to_sample_batches(fn), "afterwards: ")
    # the RLlib adapter passes the keyword through
    adapter = ph.rllib.BatchedBaseEnv(make()).sample(T_E2E, batcher=ph.TrainBatcher(make(), policy_mapping_fn=fn), **kw)
    assert set(adapter) == {"even", "odd"} and all(isinstance(v, DeviceBatch) for v in adapter.values())
    with pytest.raises(ValueError, match="batcher"):
        env.sample(T_E2E, batcher=tb, compact=True)


def test_device_env_train_batch_checks_its_arguments_before_any_launch():
    env = _fsm_env()
    tr = env.rollout(8)
    dev = env._device()
    B, S = dev.B, dev.S
    planes = {"obs": tr.observations, "rewards": tr.rewards, "truncateds": tr.truncations}
    start, records, row, col, moments, layout = dev.train_batch(planes, keep=tr.obs_valid, standardize="rewards", seed=3, epoch=1)
    assert dev.last_kernel() == _abi.BATCH_KERNELS
    assert layout == {"obs": (0, 3, torch.float32), "rewards": (3, 1, torch.float32), "truncateds": (4, 1, torch.uint8)}
    assert tuple(records.shape) == (8 * B * S, 16) and records.dtype == torch.int32 and tuple(start.shape) == (B * S + 1,)
    src = [np.ascontiguousarray(x.cpu().numpy()).reshape((8, B * S) + tuple(x.shape[3:])) for x in planes.values()]
    src = [s if s.dtype == np.uint8 else s.view(np.uint32) for s in src]
    ref = br.train_batch(8, B * S, list(zip(src, (0, 3, 4))), 16, keep=tr.obs_valid.cpu().numpy().reshape(8, -1), seed=3, epoch=1, std_plane=1)
    K = ref["K"]
    assert 0 < K < 8 * B * S and int(start[-1]) == K
    assert records[:K].cpu().numpy().view(np.uint32).tobytes() == ref["records"].tobytes()
    assert moments.cpu().numpy().tobytes() == ref["moments"].tobytes()
    # caller-owned outputs: nothing is allocated, refusals leave them untouched
    outs = {"start": fenced((B * S + 1,), torch.int64, dev.device), "records": fenced((K, 8), torch.int32, dev.device),
            "row": fenced((K,), torch.int32, dev.device), "moments": fenced((32,), torch.uint8, dev.device),
            "workspace": fenced((B * S, 2), torch.float64, dev.device)}
    out = (outs["start"][0], outs["records"][0], outs["row"][0], None, outs["moments"][0], outs["workspace"][0])
    good = dict(keep=tr.obs_valid, standardize="rewards", row_words=8, capacity=K, out=out, seed=3, epoch=1)
    for match, bad in (("keep", dict(keep=tr.obs_valid.to(torch.int32))), ("keep", dict(keep=tr.obs_valid.cpu())), ("standardize", dict(standardize="obs")),
                       ("standardize", dict(standardize="nothing")), ("row_words", dict(row_words=6)), ("row_words", dict(row_words=4)),
                       ("capacity", dict(capacity=-1)), (r"out\[1\]", dict(capacity=K + 1)), ("class_id", dict(class_id=256)),
                       ("col_class", dict(col_class=torch.zeros(S + 1, dtype=torch.uint8, device=dev.device))), ("seed", dict(seed=-1)),
                       ("epoch", dict(epoch=2 ** 64)), ("out", dict(out=out[:5])), (r"out\[4\]", dict(out=out[:4] + (None, None)))):
        with pytest.raises(ValueError, match=match):
            dev.train_batch(planes, **dict(good, **bad))
    with pytest.raises(ValueError, match="rewards"):
        dev.train_batch(dict(planes, rewards=tr.rewards.double()), **good)
    with pytest.raises(ValueError, match="planes"):
        dev.train_batch({f"p{i}": tr.rewards for i in range(33)}, keep=tr.obs_valid)
    torch.cuda.synchronize()
    for k, (_, whole) in outs.items():
        assert_poison(whole, f"a refused DeviceEnv.train_batch call: {k}")
    res = dev.train_batch(planes, **good)
    assert res[1].data_ptr() == out[1].data_ptr() and res[3] is None
    for k, (plane, whole) in outs.items():
        assert_fences(whole, plane.shape[0], k)
    rec8 = res[1].cpu().numpy().view(np.uint32)
    assert (rec8[:, :5] == ref["records"][:, :5]).all() and (rec8[:, 5:] == 0).all()
    assert (res[2].cpu().numpy() == ref["out_row"]).all()
