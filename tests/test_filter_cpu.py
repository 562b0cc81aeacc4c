"""CPU: the definition of phx_filter_update / phx_filter_apply (include/phantom_amd_filter.h) as tests/filter_ref.py restates it -- the two
forms against each other, the header's known answers, an empty class, counts of 0 and 1 in apply, a large-offset case that a
sumsq / K - m * m variance fails, ObsFilter.fold against its restatement and the folded network against the unfolded one; the structs
against the header as a C compiler lays them out, the symbols and the naming rule between the headers, no scratch in any kernel;
FragmentOps.filter_*'s fields and refusals in front of a stand-in library and ObsFilter on a stand-in env and device."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import filter_ref as fr
from phantom_amd import _abi, build

STRUCTS = ((_abi.PhxFilterState, "phx_filter_state", 272), (_abi.PhxFilterUpdateIO, "phx_filter_update_io", 80),
           (_abi.PhxFilterApplyIO, "phx_filter_apply_io", 80))
OTHERS = ("phx_train_batch", "phx_seq_batch", "phx_traj", "phx_replay", "phx_prio")     # the other headers' tests scan every header for these
# (T, N, D, n_classes, keep): N across the fold's 256 lanes, an empty class and a column of no class where n_classes >= 3
CASES = [(3, 5, 2, 2, "random"), (1, 1, 1, 1, "none"), (7, 257, 3, 3, "random"), (2, 513, 16, 16, "none"), (4, 300, 3, 3, "zero"),
         (2, 255, 1, 3, "random"), (5, 256, 4, 1, "random")]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("T,N,D,n_classes,keep", CASES)
def test_the_two_forms_agree_bit_for_bit(T, N, D, n_classes, keep):
    rng = np.random.default_rng([T, N, D, n_classes])
    st = fr.empty_state(n_classes)
    for u in range(3):
        obs, k, cls = fr.random_case(rng, T, N, D, n_classes, keep, offset=100.0 * u)
        a, b = fr.update_loop(st, obs, k, cls), fr.update(st, obs, k, cls)
        np.testing.assert_array_equal(_bits(a), _bits(b))
        st = a
        for clip in (0.0, 1.5):
            np.testing.assert_array_equal(_bits(fr.apply_loop(st, obs, k, cls, clip)), _bits(fr.apply(st, obs, k, cls, clip)))
    if keep != "zero":
        assert (st["count"][:max(1, n_classes - 1) if n_classes >= 3 else n_classes] > 0).any()
    if n_classes >= 3:
        assert _bits(st[n_classes - 1]).max() == 0           # the empty class: all zero still
    v = rng.normal(size=(700, 3))
    np.testing.assert_array_equal(fr.fold(v), [fr.fold_loop(v[:, j]) for j in range(3)])


def test_known_answers_of_the_header():
    header = open(os.path.join(ROOT, "include", "phantom_amd_filter.h")).read()
    st = fr.empty_state(2)
    for u in range(3):
        st = fr.update_loop(st, fr.known_obs(u), None, fr.KNOWN_CLASS)
    assert "col_class = 0 1 0 1 0" in header and "x[t][n][d] = (float)(((u * 7 + 3 * t + 5 * n + 11 * d) % 13) - 4) / 2" in header
    for c in range(2):
        line = (f"class {c}: count {st['count'][c]}, updates {st['updates'][c]}, mean {float(st['mean'][c, 0])!r} {float(st['mean'][c, 1])!r}, "
                f"m2 {float(st['m2'][c, 0])!r} {float(st['m2'][c, 1])!r}\n")
        assert line in header, line
    assert st["count"].tolist() == [27, 18] and (st["mean"][:, 2:] == 0).all() and (st["m2"][:, 2:] == 0).all()
    # against numpy's own two-pass moments of the concatenated data (these values are exact in f64 up to rounding of the merge)
    x = np.concatenate([fr.known_obs(u) for u in range(3)]).astype(np.float64)
    for c in range(2):
        a = x[:, fr.KNOWN_CLASS == c].reshape(-1, 2)
        np.testing.assert_allclose(st["mean"][c, :2], a.mean(0), rtol=1e-14)
        np.testing.assert_allclose(st["m2"][c, :2], ((a - a.mean(0)) ** 2).sum(0), rtol=1e-13)


def test_a_class_without_kept_elements_keeps_its_bytes():
    rng = np.random.default_rng(3)
    obs, k, cls = fr.random_case(rng, 4, 40, 3, 2, "random")
    cls[:] = np.arange(40) % 2
    st = fr.update(fr.empty_state(2), obs, k, cls)
    before = st.copy()
    k2 = k.copy()
    k2[:, cls == 1] = 0                                       # class 1 sees nothing in the second update
    for f in (fr.update, fr.update_loop):
        st2 = f(st, obs + 1, k2, cls)
        np.testing.assert_array_equal(_bits(st2[1]), _bits(before[1]))
        assert st2["updates"].tolist() == [2, 1] and st2["count"][0] > before["count"][0]
    np.testing.assert_array_equal(_bits(fr.update(st, obs, np.zeros_like(k), cls)), _bits(before))


def test_apply_with_counts_of_zero_and_one():
    x = np.array([[[-0.0, 3.0], [2.5, -1e30], [7.0, 7.0]]], np.float32)      # T = 1, N = 3, D = 2
    cls = np.array([0, 1, 2], np.int32)
    st = fr.empty_state(2)
    for f in (fr.apply, fr.apply_loop):
        out = f(st, x, None, cls, clip=1.0)                   # count 0: the identity, no clamp; the column of no class: +0.0
        np.testing.assert_array_equal(_bits(out[0, :2]), _bits(x[0, :2]))
        np.testing.assert_array_equal(_bits(out[0, 2]), _bits(np.zeros(2, np.float32)))
    st = fr.update(st, np.array([[[4.0, -2.0]]], np.float32))           # count 1 in class 0: var = mean * mean
    assert st["count"].tolist() == [1, 0] and st["mean"][0, :2].tolist() == [4.0, -2.0] and (st["m2"] == 0).all()
    mean_f, den_f, seen = fr.table(st, 2)
    assert mean_f[0].tolist() == [4.0, -2.0] and den_f[0].tolist() == [np.float32(4.0) + np.float32(1e-8), np.float32(2.0) + np.float32(1e-8)]
    assert den_f[1].tolist() == [1.0, 1.0] and seen.tolist() == [True, False]
    for f in (fr.apply, fr.apply_loop):
        out = f(st, x, np.array([[1, 1, 0]], np.uint8), np.array([0, 1, 0], np.int32), clip=0.5)
        assert out[0, 0].tolist() == [-0.5, 0.5]             # (0 - 4) / 4 = -1 and (3 + 2) / 2 = 2.5, clamped
        np.testing.assert_array_equal(_bits(out[0, 1]), _bits(x[0, 1]))
        np.testing.assert_array_equal(_bits(out[0, 2]), _bits(np.zeros(2, np.float32)))


def _large_offset():
    rng = np.random.default_rng(20261021)
    T, N, D = 20, 300, 3
    st, xs = fr.empty_state(1), []
    for _ in range(3):
        x = (1e6 + rng.uniform(-1, 1, (T, N, D))).astype(np.float32)
        st = fr.update(st, x)
        xs.append(x.reshape(-1, D).astype(np.float64))
    return st, np.concatenate(xs)


def test_the_running_variance_survives_a_large_offset():
    """1e6 + U(-1, 1), three updates of 6 000 elements: the running variance against numpy's f64 two-pass variance over the
    concatenated data.  Measured on the CPU: a relative error of 1.59e-12; allowed 8x, 1.27e-11.  The same data through
    sumsq / K - m * m in f64 is off by 0.54 -- it does not meet the bound, which is what the two centred passes are for."""
    st, a = _large_offset()
    K = len(a)
    var = ((a - a.mean(0)) ** 2).sum(0) / (K - 1)
    got = st["m2"][0, :3] / (st["count"][0] - 1)
    rel = (np.abs(got - var) / var).max()
    print("relative error of the running variance:", rel)
    bound = 8 * 1.59e-12
    assert st["count"][0] == K and rel <= bound
    m = a.sum(0) / K
    naive = ((a * a).sum(0) / K - m * m) * K / (K - 1)
    naive_rel = (np.abs(naive - var) / var).min()
    print("relative error of sumsq / K - m * m:", naive_rel)
    assert naive_rel > bound


class _Spec:
    agent_ids = ["a", "b", "c", "d", "e", "bank"]
    strategic_idx = [0, 1, 2, 3, 4]
    n_strategic = 5
    obs_dim = 3


_Env = SimpleNamespace(spec=_Spec, batch_size=2)


class _Dev:
    """stands in for DeviceEnv.filter_update / filter_apply on CPU tensors: the restatement, and a record of what was asked"""
    device = "cpu"

    def __init__(self):
        self.asked = []

    def filter_update(self, obs, state, keep=None, col_class=None, n_classes=1, workspace=None):
        import torch
        self.asked.append(("update", keep, col_class, n_classes, workspace))
        st = state.numpy().reshape(-1).view(fr.STATE_DTYPE)
        new = fr.update(st, obs.numpy(), None if keep is None else keep.numpy(), None if col_class is None else col_class.numpy())
        state.copy_(torch.from_numpy(new.view(np.uint8).reshape(state.shape).copy()))

    def filter_apply(self, obs, state, keep=None, col_class=None, n_classes=1, clip=0.0, out=None):
        import torch
        self.asked.append(("apply", keep, col_class, n_classes, clip, out))
        st = state.numpy().reshape(-1).view(fr.STATE_DTYPE)
        y = torch.from_numpy(fr.apply(st, obs.numpy(), None if keep is None else keep.numpy(),
                                      None if col_class is None else col_class.numpy(), clip))
        if out is None:
            return y
        out.copy_(y)
        return out


def _filled_filter(clip=None, mapping=None, seed=7):
    import torch
    import phantom_amd as ph
    rng = np.random.default_rng(seed)
    f = ph.ObsFilter(_Env, policy_mapping_fn=mapping, clip=clip)
    dev = _Dev()
    obs = torch.from_numpy(rng.uniform(0, 100, (6, 2, 5, 3)).astype(np.float32))
    keep = torch.from_numpy((rng.uniform(size=(6, 2, 5)) < 0.7).astype(np.uint8))
    f.update(dev, obs, keep)
    return f, dev, obs, keep


def test_fold_is_bit_equal_to_its_restatement():
    rng = np.random.default_rng(11)
    f, _, _, _ = _filled_filter()
    mean_f, den_f = f.table()
    ref_mean, ref_den, _ = fr.table(f.state(), 3)
    np.testing.assert_array_equal(_bits(mean_f), _bits(ref_mean[0]))
    np.testing.assert_array_equal(_bits(den_f), _bits(ref_den[0]))
    W, b = rng.normal(0, 0.5, (32, 3)).astype(np.float32), rng.normal(0, 0.1, 32).astype(np.float32)
    got = f.fold([W, np.zeros((1, 32), np.float32)], [b, np.zeros(1, np.float32)])
    for want in (fr.fold_layer(W, b, mean_f, den_f), fr.fold_layer_loop(W, b, mean_f, den_f)):
        for g, w in zip(got, want):
            assert g.dtype == np.float32
            np.testing.assert_array_equal(_bits(g), _bits(w))
    for g, w in zip(f.fold(W, b), got):                       # layer 0's arrays themselves
        np.testing.assert_array_equal(_bits(g), _bits(w))
    fresh = __import__("phantom_amd").ObsFilter(_Env, clip=None)         # a filter that has seen nothing folds to the layer itself
    for g, w in zip(fresh.fold(W, b), (W, b)):
        np.testing.assert_array_equal(_bits(g), _bits(w))


def test_the_folded_network_on_raw_observations_is_the_network_on_normalised_ones():
    """a 3-32-1 tanh network in f64 on the host: folded weights on raw observations in [0, 100) against the unfolded weights on
    apply's output.  Measured on the CPU: a largest difference of 2.0e-7 (the f32 roundings of W', b' and of apply's two f32
    operations); allowed 8x, 1.6e-6."""
    rng = np.random.default_rng(7)
    D, H = 3, 32
    st = fr.update(fr.empty_state(1), rng.uniform(0, 100, (64, 1, D)).astype(np.float32))
    mean_f, den_f, _ = fr.table(st, D)
    W0, b0 = rng.normal(0, 0.5, (H, D)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)
    W1, b1 = rng.normal(0, 0.3, (1, H)).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32)
    W0f, b0f = fr.fold_layer(W0, b0, mean_f[0], den_f[0])
    raw = rng.uniform(0, 100, (256, 1, D)).astype(np.float32)
    y = fr.apply(st, raw).reshape(-1, D).astype(np.float64)
    f64 = lambda a: a.astype(np.float64)
    net = lambda W, b, z: np.tanh(z @ f64(W).T + f64(b)) @ f64(W1).T + f64(b1)
    diff = np.abs(net(W0, b0, y) - net(W0f, b0f, f64(raw.reshape(-1, D)))).max()
    print("largest difference between the folded and the unfolded network:", diff)
    assert diff <= 8 * 2.0e-7


def test_obs_filter_maps_policies_holds_the_state_and_checks_its_arguments():
    import torch
    import phantom_amd as ph
    mapping = lambda aid: "x" if aid in "ace" else "y"
    f, dev, obs, keep = _filled_filter(clip=10.0, mapping=mapping)
    assert f.agent_ids == ["a", "b", "c", "d", "e"] and (f.B, f.S, f.D, f.n_classes) == (2, 5, 3, 2) and f.clip == 10.0
    assert f.policies == {"x": [0, 2, 4], "y": [1, 3]} and f.agent_class.tolist() == [0, 1, 0, 1, 0] and f.agent_class.dtype == np.int32
    kind, k, cls, n, ws = dev.asked[0]
    assert kind == "update" and k is keep and n == 2 and cls.dtype == torch.int32 and cls.tolist() == [0, 1, 0, 1, 0] * 2
    assert ws.dtype == torch.float64 and ws.numel() * 8 == _abi.filter_workspace_bytes(10, 3) == fr.workspace_bytes(10, 3)
    want = fr.update(fr.empty_state(2), obs.numpy(), keep.numpy(), np.tile(f.agent_class, 2))
    np.testing.assert_array_equal(_bits(f.state()), _bits(want))
    stats = f.stats()
    assert list(stats) == ["x", "y"]
    for c, pid in enumerate(stats):
        count, mean, var = stats[pid]
        assert count == want["count"][c] > 1 and mean.shape == var.shape == (3,)
        np.testing.assert_array_equal(mean, want["mean"][c, :3])
        np.testing.assert_array_equal(var, want["m2"][c, :3] / (count - 1))
    out = f.apply(dev, obs, keep)
    np.testing.assert_array_equal(_bits(out.numpy()), _bits(fr.apply(want, obs.numpy(), keep.numpy(), np.tile(f.agent_class, 2), 10.0)))
    assert dev.asked[-1][0] == "apply" and dev.asked[-1][4] == 10.0
    same = f.apply(dev, obs, keep, out=obs)                   # in place
    assert same is obs and torch.equal(same, out)
    # a checkpoint: stats() into a fresh filter gives the same table up to the rounding of var * (count - 1)
    g = ph.ObsFilter(_Env, policy_mapping_fn=mapping, clip=None)
    g.set_stats(stats)
    assert g.state()["count"].tolist() == want["count"].tolist() and g.state()["updates"].tolist() == [1, 1]
    np.testing.assert_array_equal(g.state()["mean"], want["mean"])
    np.testing.assert_allclose(g.state()["m2"], want["m2"], rtol=4e-16)
    g.set_stats({"x": (0, np.zeros(3), np.zeros(3)), "y": (1, np.ones(3), np.ones(3))})
    assert g.state()["count"].tolist() == [0, 1] and (g.state()["m2"] == 0).all() and g.stats()["y"][2].tolist() == [1.0, 1.0, 1.0]
    one = ph.ObsFilter(_Env)
    assert one.policies == {"default_policy": [0, 1, 2, 3, 4]} and one.clip == 10.0
    one.update(dev, obs)
    assert dev.asked[-1][1] is None and dev.asked[-1][2] is None and dev.asked[-1][3] == 1      # one policy: no class plane
    for bad in (0, -1.0, float("nan"), float("inf"), True, "10"):
        with pytest.raises(ValueError, match="clip"):
            ph.ObsFilter(_Env, clip=bad)
    with pytest.raises(ValueError, match="policies"):
        ph.ObsFilter(SimpleNamespace(spec=SimpleNamespace(agent_ids=list(range(17)), strategic_idx=list(range(17)), n_strategic=17, obs_dim=3),
                                     batch_size=1), policy_mapping_fn=lambda aid: aid)
    with pytest.raises(ValueError, match="features"):
        ph.ObsFilter(SimpleNamespace(spec=SimpleNamespace(agent_ids=["a"], strategic_idx=[0], n_strategic=1, obs_dim=17), batch_size=1))
    with pytest.raises(ValueError, match="expected"):
        f.update(dev, obs[:, :1])
    with pytest.raises(ValueError, match="expected"):
        f.apply(dev, obs[..., :2])
    with pytest.raises(ValueError, match="clip"):
        f.fold(np.zeros((4, 3), np.float32), np.zeros(4, np.float32), "x")
    with pytest.raises(ValueError, match="name one"):
        g.fold(np.zeros((4, 3), np.float32), np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="no policy"):
        g.fold(np.zeros((4, 3), np.float32), np.zeros(4, np.float32), "z")
    with pytest.raises(ValueError, match="layer 0"):
        g.fold(np.zeros((4, 2), np.float32), np.zeros(4, np.float32), "x")
    for bad in ({"x": stats["x"]}, {"x": stats["x"], "y": (-1, np.zeros(3), np.zeros(3))}, {"x": stats["x"], "y": (2, np.zeros(2), np.zeros(3))},
                {"x": stats["x"], "y": (2, np.zeros(3), -np.ones(3))}):
        with pytest.raises(ValueError, match="set_stats"):
            g.set_stats(bad)


# ---- FragmentOps in front of a stand-in library ------------------------------------------------------------------------------------
def _ops(rc=0):
    import torch
    from test_fragment_ops_cpu import Ops, RecordingLib
    return Ops(RecordingLib(rc), torch.device("cpu"))


def _args():
    import torch
    T, B, S, D = 3, 2, 2, 3
    z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype)
    return dict(obs=z(torch.float32, T, B, S, D), state=z(torch.uint8, 2, 272), keep=z(torch.uint8, T, B, S), col_class=z(torch.int32, B * S),
                n_classes=2)


def test_fragment_ops_place_every_pointer_and_scalar():
    import torch
    from test_fragment_ops_cpu import fields
    kw = _args()
    ws = torch.zeros(_abi.filter_workspace_bytes(4, 3) // 8, dtype=torch.float64)
    ops = _ops()
    assert ops.filter_update(**kw, workspace=ws) is kw["state"]
    (name, io), = ops.lib.calls
    assert name == "phx_filter_update" and fields(io) == dict(
        T=3, D=3, N=4, n_classes=2, reserved0=0, obs=kw["obs"].data_ptr(), keep=kw["keep"].data_ptr(), col_class=kw["col_class"].data_ptr(),
        state=kw["state"].data_ptr(), workspace=ws.data_ptr(), reserved=[0, 0])
    ops = _ops()
    out = torch.zeros_like(kw["obs"])
    assert ops.filter_apply(**kw, clip=2.5, out=out) is out
    (name, io), = ops.lib.calls
    assert name == "phx_filter_apply" and fields(io) == dict(
        T=3, D=3, N=4, n_classes=2, clip=2.5, obs=kw["obs"].data_ptr(), keep=kw["keep"].data_ptr(), col_class=kw["col_class"].data_ptr(),
        state=kw["state"].data_ptr(), out=out.data_ptr(), reserved=[0, 0])
    ops = _ops()                                              # bare: everything optional omitted, in place allowed, [T, N, D] planes
    obs = torch.zeros(3, 4, 3)
    res = ops.filter_apply(obs, kw["state"][:1])
    ops.filter_apply(obs, kw["state"][:1], out=obs)
    ops.filter_update(obs, kw["state"][:1])
    assert res.shape == obs.shape and res.dtype == torch.float32 and res.data_ptr() != obs.data_ptr()
    a, b, c = (fields(io) for _, io in ops.lib.calls)
    assert a["keep"] == a["col_class"] == 0 and a["clip"] == 0.0 and a["n_classes"] == 1 and a["out"] == res.data_ptr() and b["out"] == obs.data_ptr()
    assert c["workspace"] != 0 and c["keep"] == c["col_class"] == 0 and (c["T"], c["N"], c["D"]) == (3, 4, 3)


def test_fragment_ops_refuse_before_any_call_into_the_library():
    import torch
    from test_fragment_ops_cpu import misaligned
    from phantom_amd.fragment_ops import DeviceError
    kw = _args()
    bad = [("obs", dict(obs=None)), ("obs", dict(obs=torch.zeros(3, 4))), ("obs", dict(obs=torch.zeros(3, 2, 2, 17))),
           ("obs", dict(obs=kw["obs"].double())), ("obs", dict(obs=misaligned(kw["obs"]))), ("T and N", dict(obs=torch.zeros(0, 2, 2, 3))),
           ("state", dict(state=None)), ("state", dict(state=kw["state"][:1])), ("state", dict(state=torch.zeros(2, 34, dtype=torch.int64))),
           ("state", dict(state=misaligned(kw["state"]))), ("keep", dict(keep=kw["keep"].float())), ("keep", dict(keep=kw["keep"][:2])),
           ("col_class", dict(col_class=kw["col_class"].long())), ("col_class", dict(col_class=kw["col_class"][:3])),
           ("n_classes", dict(n_classes=0)), ("n_classes", dict(n_classes=17)), ("n_classes", dict(n_classes=True)), ("n_classes", dict(n_classes=2.0))]
    for fn in ("filter_update", "filter_apply"):
        for match, patch in bad:
            ops = _ops()
            with pytest.raises(ValueError, match=match):
                getattr(ops, fn)(**dict(kw, **patch))
            assert ops.lib.calls == [], (fn, patch)
    ws = torch.zeros(_abi.filter_workspace_bytes(4, 3) // 8, dtype=torch.float64)
    out = torch.zeros(3 * 2 * 2 * 3 + 4)
    more = [("filter_update", "workspace", dict(workspace=ws[:-1])), ("filter_update", "workspace", dict(workspace=ws.float())),
            ("filter_update", "workspace", dict(workspace=misaligned(ws))),
            ("filter_apply", "clip", dict(clip=-1.0)), ("filter_apply", "clip", dict(clip=float("nan"))), ("filter_apply", "clip", dict(clip=True)),
            ("filter_apply", "clip", dict(clip=None)), ("filter_apply", r"out\[0\]", dict(out=torch.zeros(3, 2, 2, 2))),
            ("filter_apply", r"out\[0\]", dict(out=misaligned(kw["obs"]))), ("filter_apply", r"out\[0\]", dict(out=kw["obs"].double())),
            ("filter_apply", "overlaps", dict(obs=out[:36].view(3, 2, 2, 3), out=out[4:40].view(3, 2, 2, 3)))]
    for fn, match, patch in more:
        ops = _ops()
        with pytest.raises(ValueError, match=match):
            getattr(ops, fn)(**dict(kw, **patch))
        assert ops.lib.calls == [], (fn, patch)
    with pytest.raises(DeviceError, match=r"phx_filter_apply failed \(7\): stand-in"):
        _ops(rc=7).filter_apply(**kw)


# ---- the header, the symbols, the build --------------------------------------------------------------------------------------------
def test_struct_symbols_and_header(tmp_path):
    header = open(os.path.join(ROOT, "include", "phantom_amd_filter.h")).read()
    for fn in ("update", "apply"):
        assert f"int phx_filter_{fn}(const phx_filter_{fn}_io* io, void* stream);" in header
    for struct, name, size in STRUCTS:
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
        names = re.findall(r"(\w+)(?:\[\w+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
        assert names == [n for n, _ in struct._fields_], names
        assert ctypes.sizeof(struct) == size and re.search(rf"\}} {name};\s+/\* {size} bytes \*/", header)
    assert np.dtype(_abi.FILTER_STATE_DTYPE) == fr.STATE_DTYPE and fr.STATE_DTYPE.itemsize == _abi.FILTER_STATE_BYTES == 272
    assert _abi.FILTER_MAX_DIM == fr.MAX_DIM == 16 and "#define PHX_FILTER_MAX_DIM 16" in header
    assert _abi.FILTER_MAX_CLASSES == fr.MAX_CLASSES == 16 and "#define PHX_FILTER_MAX_CLASSES 16" in header
    # the naming rule, in both directions: every header's test scans all of include/ for its own identifiers
    for banned in OTHERS:
        assert banned not in header, banned
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "phantom_amd_filter.h":
            assert "phx_filter" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert _abi.FILTER_UPDATE_KERNELS == fr.UPDATE_KERNELS and f'"{_abi.FILTER_UPDATE_KERNELS}"' in header
    assert _abi.FILTER_APPLY_KERNEL == fr.APPLY_KERNEL and f'"{_abi.FILTER_APPLY_KERNEL}"' in header
    assert (_abi.FILTER_SUM_KERNEL, _abi.FILTER_MEAN_KERNEL, _abi.FILTER_CENTER_KERNEL, _abi.FILTER_M2_KERNEL,
            _abi.FILTER_MERGE_KERNEL) == tuple(_abi.FILTER_UPDATE_KERNELS.split("+"))
    assert "phx_obs_filter.hip" in build.SOURCES and any(h.endswith("phantom_amd_filter.h") for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS)
    assert set(_abi.FILTER_OPS) == {"phx_filter_update", "phx_filter_apply"}
    assert not set(_abi.FILTER_OPS) & (set(_abi.FRAGMENT_OPS) | set(_abi.PRIORITY_OPS))
    lib = _abi.load_library()
    for fn, io in _abi.FILTER_OPS.items():
        assert hasattr(lib, fn) and fn not in _abi.EXPORTS
        assert getattr(lib, fn)(None, None) == -1 and fn.encode() in lib.phx_last_error()      # refused before any launch
        assert getattr(lib, fn).restype is ctypes.c_int32 and getattr(lib, fn).argtypes[0] is ctypes.POINTER(io)
    assert _abi.ABI_VERSION == 10 and lib.phx_abi_version() == 10
    # the sizes and offsets a C compiler gives the header's structs
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [(name, n) for s, name, _ in STRUCTS for n, _ in s._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phantom_amd_filter.h"\nint main(void) {\n' +
                   "".join(f'  printf("%zu\\n", sizeof({name}));\n' for _, name, _ in STRUCTS) +
                   "".join(f'  printf("%zu\\n", offsetof({s}, {f}));\n' for s, f in fields) +
                   '  printf("%lld\\n", (long long)PHX_FILTER_WORKSPACE_BYTES(36864, 3));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out[:3]] == [272, 80, 80]
    assert [int(x) for x in out[3:-1]] == [getattr(s, n).offset for s, _, _ in STRUCTS for n, _ in s._fields_]
    assert int(out[-1]) == _abi.filter_workspace_bytes(36864, 3) == fr.workspace_bytes(36864, 3)


def test_no_kernel_uses_scratch(tmp_path):
    """every kernel of the file cross-compiled for gfx950 with the build's own flags reports ScratchSize 0: the D sums of a column and
    a chunk's loads stay in registers at every D"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_obs_filter.hip"), "-o", str(tmp_path / "f.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 32 + 32 + 3 + 16 and set(scratch) == {0}, sorted(set(scratch))
    for kernel in _abi.FILTER_UPDATE_KERNELS.split("+") + [_abi.FILTER_APPLY_KERNEL]:
        assert any(kernel in n for n in names), kernel
