"""CPU: the definition of phx_traj_compact (include/phantom_amd_compact.h) as tests/compact_ref.py restates it -- the positions formula
against the boolean mask of the transposed plane; the structs, the symbol and the headers; no scratch in any instantiation of the three
kernels; CompactFragment's sample batches against FragmentBatch's on the same arrays; a plain FragmentBatch's columns."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import compact_ref as cr
from phantom_amd import _abi, build
from phantom_amd.rollout import CompactFragment, FragmentBatch

SHAPES = [(1, 1), (1, 5), (2, 9), (7, 16), (63, 64), (64, 63), (65, 65), (129, 70), (3, 257)]


@pytest.mark.parametrize("T,N", SHAPES)
def test_the_two_restatements_agree(T, N):
    for i, density in enumerate(cr.DENSITIES):
        rng = np.random.default_rng([i, T, N])
        keep = cr.keep_case(rng, T, N, density)
        assert keep.dtype == np.uint8 and keep.shape == (T, N)
        planes = {str(eb): cr.plane_case(rng, T, N, eb) for eb in (1, 4, 12, 20)}
        start, out_row, out_col, dense = cr.compact(keep, planes)
        K = int((keep != 0).sum())
        assert start.dtype == np.int64 and start[0] == 0 and start[N] == K == len(out_row) == len(out_col)
        if density in ("all", "none", "one"):
            assert K == {"all": T * N, "none": 0, "one": 1}[density]
        np.testing.assert_array_equal(out_row, cr.by_mask(keep, np.broadcast_to(np.arange(T, dtype=np.int32)[:, None], (T, N))))
        np.testing.assert_array_equal(out_col, cr.by_mask(keep, np.broadcast_to(np.arange(N, dtype=np.int32)[None, :], (T, N))))
        for name, src in planes.items():
            assert dense[name].dtype == src.dtype and dense[name].tobytes() == cr.by_mask(keep, src).tobytes(), (density, name)
        if density == "all":                                   # the reduction: the [N][T] transpose
            assert (start == np.arange(N + 1) * T).all() and (out_row.reshape(N, T) == np.arange(T)).all()
            for name, src in planes.items():
                np.testing.assert_array_equal(dense[name].reshape((N, T) + src.shape[2:]), np.moveaxis(src, 0, 1))
        for cap in sorted({0, K // 2, max(K - 1, 0)}):        # the clip: the same prefix, the same start
            s2, r2, c2, d2 = cr.compact(keep, planes, cap)
            n_out = min(K, cap)
            assert (s2 == start).all() and len(r2) == len(c2) == n_out
            assert (r2 == out_row[:n_out]).all() and (c2 == out_col[:n_out]).all()
            assert all(d2[k].tobytes() == dense[k][:n_out].tobytes() for k in planes)


def test_the_cases_hold_the_special_words():
    src = cr.plane_case(np.random.default_rng(0), 5, 7, 12)
    assert src.dtype == np.uint32 and src.shape == (5, 7, 3) and tuple(src.reshape(-1)[:5]) == cr.SPECIAL_WORDS
    assert np.isnan(src.view(np.float32).reshape(-1)[1]) and cr.plane_case(np.random.default_rng(0), 5, 7, 4).shape == (5, 7)


def test_struct_symbol_and_headers():
    io, plane = _abi.PhxTrajCompactIO, _abi.PhxCompactPlane
    header = open(os.path.join(ROOT, "include", "phantom_amd_compact.h")).read()
    assert ctypes.sizeof(plane) == 24 and "} phx_compact_plane;      /* 24 bytes */" in header
    assert ctypes.sizeof(io) == 440 and "} phx_traj_compact_io;              /* 440 bytes */" in header
    assert "#define PHX_COMPACT_MAX_PLANES 16" in header and _abi.COMPACT_MAX_PLANES == 16
    offsets = dict(T=0, n_planes=4, N=8, capacity=16, keep=24, start=32, out_row=40, out_col=48, plane=56)
    assert {n: getattr(io, n).offset for n, _ in io._fields_} == offsets
    assert {n: getattr(plane, n).offset for n, _ in plane._fields_} == dict(src=0, dst=8, elem_bytes=16, reserved=20)
    for struct, name in ((io, "phx_traj_compact_io"), (plane, "phx_compact_plane")):
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
        names = re.findall(r"(\w+)(?:\[\w+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
        assert names == [n for n, _ in struct._fields_], names
    assert "int phx_traj_compact(const phx_traj_compact_io* io, void* stream);" in header
    lib = _abi.load_library()
    assert hasattr(lib, "phx_traj_compact") and hasattr(lib, "phx_traj_next") and hasattr(lib, "phx_gae_masked") and hasattr(lib, "phx_vtrace")
    assert "phx_traj_compact" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert _abi.COMPACT_KERNELS == "phx_compact_count_kernel+phx_compact_scan_kernel+phx_compact_scatter_kernel" and _abi.COMPACT_KERNELS in header
    assert (_abi.COMPACT_COUNT_KERNEL, _abi.COMPACT_SCAN_KERNEL, _abi.COMPACT_SCATTER_KERNEL) == tuple(_abi.COMPACT_KERNELS.split("+"))
    for h in ("phantom_amd.h", "phantom_amd_gae.h", "phantom_amd_vtrace.h", "phantom_amd_traj.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "phx_traj_compact" not in text and "phx_compact" not in text, h
    assert ctypes.sizeof(_abi.PhxGaeIO) == 80 and ctypes.sizeof(_abi.PhxGaeMaskedIO) == 104 and ctypes.sizeof(_abi.PhxVtraceIO) == 112
    assert ctypes.sizeof(_abi.PhxTrajNextIO) == 96
    assert "phx_traj_compact.hip" in build.SOURCES and any(h.endswith("phantom_amd_compact.h") for h in build.HEADERS)


def test_no_instantiation_of_the_kernels_uses_scratch(tmp_path):
    """every instantiation cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 (a spilled item buffer would put
    loads and stores into the scatter's store phase): one of the count, one of the scan, four of the scatter"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_traj_compact.hip"), "-o", str(tmp_path / "cp.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == 6
    assert [sum(k in n for n in names) for k in ("phx_compact_count_kernel", "phx_compact_scan_kernel", "phx_compact_scatter_kernel")] == [1, 1, 4]
    assert scratch == [0] * 6, dict(zip(names, scratch))


# ---- the two batch forms -----------------------------------------------------------------------------------------------------------
IDS = ["a", "b", "c", "d"]
MAPPINGS = {"default": None, "per agent": lambda aid: aid, "not contiguous": lambda aid: "x" if aid in "ac" else "y",
            "a subset and the rest": lambda aid: "first" if aid == "a" else "rest"}


def _time_major(B=3, S=4, T=7, D=3, critic=True, seed=0):
    rng = np.random.default_rng(seed)
    keep = (rng.random((T, B, S)) < 0.5).astype(np.uint8)
    keep[:, 1, 2] = 0                                          # a column that keeps nothing
    keep[:, 2, 0] = 1                                          # and one that keeps everything
    f = lambda *tail: rng.normal(size=(T, B, S) + tail).astype(np.float32)
    cols = {"obs": f(D), "new_obs": f(D), "actions": f(), "rewards": f(), "terminateds": (rng.random((T, B, S)) < 0.3).astype(np.uint8),
            "truncateds": (rng.random((T, B, S)) < 0.3).astype(np.uint8), "trajectory_next_row": rng.integers(-1, T, (T, B, S)).astype(np.int32)}
    if critic:
        cols.update(vf_preds=f(), advantages=f(), value_targets=f())
    cols["obs"].view(np.uint32)[0, 2, 0] = (0x80000000, 0x7fc00001, 0xff800001)       # (bytes are compared: NaN payloads and -0.0 count)
    t = np.broadcast_to(np.arange(T, dtype=np.int32) % 4, (B, T)).copy()
    eps_id = ((np.arange(T) // 4)[None, :] * B + np.arange(B)[:, None]).astype(np.int64)
    return keep, cols, t, eps_id


def _fragment_batch(keep, cols, t, eps_id):
    am = lambda a: np.ascontiguousarray(np.moveaxis(a, 0, 2))                        # [T, B, S, ..] -> [B, S, T, ..]
    step = lambda a: np.zeros_like(am(a))                                            # the step-aligned planes: not what the columns show
    return FragmentBatch(IDS, am(cols["obs"]), step(cols["new_obs"]), am(cols["actions"]), step(cols["rewards"]),
                         step(cols["terminateds"]).astype(bool), step(cols["truncateds"]).astype(bool), t, eps_id, obs_valid=am(keep),
                         new_obs_valid=am(keep), reward_valid=am(keep), trajectory_rewards=am(cols["rewards"]),
                         trajectory_next_row=am(cols["trajectory_next_row"]), trajectory_new_obs=am(cols["new_obs"]),
                         trajectory_terminateds=am(cols["terminateds"]).astype(bool), trajectory_truncateds=am(cols["truncateds"]).astype(bool),
                         **{k: am(cols[k]) for k in ("vf_preds", "advantages", "value_targets") if k in cols})


@pytest.mark.parametrize("critic", [False, True])
@pytest.mark.parametrize("mapping", list(MAPPINGS))
def test_compact_fragment_gives_the_fragment_batchs_sample_batches(mapping, critic):
    keep, cols, t, eps_id = _time_major(critic=critic)
    frag = CompactFragment.from_time_major(IDS, keep, cols, t, eps_id)
    B, S, T = 3, 4, 7
    assert (frag.B, frag.S, frag.T, frag.K) == (B, S, T, int(keep.sum())) and 0 < frag.K < T * B * S
    assert frag.col_start.dtype == np.int64 and frag.col_start.shape == (B * S + 1,) and frag.row.dtype == np.int32 and frag.row.shape == (frag.K,)
    assert frag.col_start[1 * S + 2] == frag.col_start[1 * S + 3] and frag.col_start[2 * S + 1] - frag.col_start[2 * S] == T
    np.testing.assert_array_equal(frag.col_start, cr.starts(keep.reshape(T, B * S)))
    got = frag.to_sample_batches(MAPPINGS[mapping])
    want = _fragment_batch(keep, cols, t, eps_id).to_sample_batches(MAPPINGS[mapping])
    cr.assert_same_batches(got, want, mapping)
    assert ("vf_preds" in got[next(iter(got))]) == critic
    if mapping == "default":                                   # every agent under one policy: the arrays themselves
        assert all(got["default_policy"][k] is v for k, v in frag.columns.items())
    assert not hasattr(frag, "rollouts") and not hasattr(frag, "step")


def test_compact_fragment_with_nothing_kept_and_with_everything_kept():
    keep, cols, t, eps_id = _time_major()
    for fill in (0, 1):
        k = np.full_like(keep, fill)
        frag = CompactFragment.from_time_major(IDS, k, cols, t, eps_id)
        assert frag.K == fill * keep.size
        for fn in MAPPINGS.values():
            cr.assert_same_batches(frag.to_sample_batches(fn), _fragment_batch(k, cols, t, eps_id).to_sample_batches(fn))
    with pytest.raises(ValueError, match="CompactFragment"):
        CompactFragment(IDS, 3, 4, 7, np.zeros(5, np.int64), np.zeros(0, np.int32), t, eps_id, {})


def test_a_plain_fragment_batchs_columns_are_what_they_were():
    B, S, T, D = 3, 2, 5, 3
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(B, S, T, D)).astype(np.float32)
    f = lambda: rng.normal(size=(B, S, T)).astype(np.float32)
    z = np.zeros((B, S, T), bool)
    tt = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    plain = FragmentBatch(["a", "b"], obs, obs + 1, f(), f(), z, z.copy(), tt, np.zeros((B, T), np.int64))
    today = plain.to_sample_batches()["default_policy"]
    assert list(today) == ["obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "eps_id", "agent_index", "t", "env_id"]
    np.testing.assert_array_equal(today["obs"], obs.reshape(-1, D))
    np.testing.assert_array_equal(today["new_obs"], (obs + 1).reshape(-1, D))
    np.testing.assert_array_equal(today["rewards"], plain.rewards.reshape(-1))
    assert today["actions"].shape == (B * S * T, 1) and len(today["obs"]) == B * S * T
    assert FragmentBatch.COLUMNS == ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")
