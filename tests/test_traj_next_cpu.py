"""CPU: the definition of phx_traj_next (include/phantom_amd_traj.h) as tests/traj_next_ref.py restates it -- the scan against the
segment-wise definition, the reduction without the two masks, what it does not read, independence of the columns; the struct, the
symbol and the headers; no scratch in any instantiation of the kernels; FragmentBatch's trajectory columns."""
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
import traj_next_ref as tn
from helpers import f32_bits
from phantom_amd import _abi, build
from phantom_amd.rollout import FragmentBatch

SHAPES = [(1, 1), (1, 5), (2, 9), (7, 16), (8, 63), (9, 64), (15, 65), (17, 70), (33, 130), (40, 257)]
FLAGS = ("truncated", "terminated", "acted", "new_obs_valid")


def _case(T, N, seed=0, D=None):
    return tn.random_case(np.random.default_rng([seed, T, N]), T, N, D=D)


@pytest.mark.parametrize("T,N", SHAPES)
def test_scan_equals_the_segment_wise_definition(T, N):
    case = _case(T, N)
    assert all(case[k].shape == (T, N) and case[k].dtype == np.uint8 for k in FLAGS)
    got = tn.scan(**case)
    assert got[0].dtype == np.int32 and got[1].dtype == got[2].dtype == np.uint8
    for g, w, name in zip(got, tn.by_segments(**case), ("next_row", "next_terminated", "next_truncated")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    hole = case["acted"] == 0
    assert (got[0][hole] == -1).all() and not got[1][hole].any() and not got[2][hole].any()
    assert not (got[1] & got[2]).any()                                # terminated wins: never both
    rows, held = np.nonzero(~hole)[0], got[0][~hole]
    assert (got[0] >= -1).all() and (got[0] < T).all() and (held[held >= 0] >= rows[held >= 0]).all()
    if N >= 63 and T >= 15:                                           # every class of row the scan can get wrong
        f = tn.features(case)
        assert all(f.values()), f
    for drop in (("terminated",), ("acted",), ("new_obs_valid",), ("terminated", "acted", "new_obs_valid")):      # a NULL plane
        c = {k: (None if k in drop else v) for k, v in case.items()}
        for g, w in zip(tn.scan(**c), tn.by_segments(**c)):
            np.testing.assert_array_equal(g, w, err_msg=str(drop))


def test_reduction_without_the_masks():
    T, N, D = 33, 130, 3
    case = _case(T, N, seed=8, D=D)
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2 ** 32, (T, N, D), dtype=np.uint64).astype(np.uint32)      # any bit pattern: NaN payloads, -0.0, denormals
    bits[0, 0] = (0x80000000, 0x7fc00001, 0xff800001)
    new_obs = bits.view(np.float32)
    for extra in ({}, dict(acted=np.ones((T, N), np.uint8), new_obs_valid=np.ones((T, N), np.uint8))):
        nr, te, tr, nob = tn.traj_next(case["truncated"], case["terminated"], obs=case["obs"], new_obs=new_obs, **extra)
        np.testing.assert_array_equal(nr, np.broadcast_to(np.arange(T, dtype=np.int32)[:, None], (T, N)))
        np.testing.assert_array_equal(te, (case["terminated"] != 0).astype(np.uint8))
        np.testing.assert_array_equal(tr, ((case["terminated"] == 0) & (case["truncated"] != 0)).astype(np.uint8))
        np.testing.assert_array_equal(f32_bits(nob), bits)
    assert (case["terminated"] & case["truncated"]).any()              # (rows with both flags are in the case)


def test_unread_elements_do_not_matter():
    T, N, D = 33, 130, 3
    case = _case(T, N, D=D)
    want = tn.traj_next(**case)
    rd = tn.reads(want[0], case["acted"])
    acted = case["acted"] != 0
    assert rd["obs"].any() and rd["new_obs"].any() and not rd["obs"][~acted].any()
    assert (rd["obs"].sum() + (acted & (want[0] >= 0)).sum()) == acted.sum()
    assert not rd["new_obs"][case["new_obs_valid"] == 0].any()        # only an observation the agent received is ever its next one
    for k in ("obs", "new_obs"):
        c = dict(case)
        c[k] = np.where(rd[k][..., None], case[k], np.float32(np.nan))
        np.testing.assert_array_equal(f32_bits(tn.traj_next(**c)[3]), f32_bits(want[3]), err_msg=f"next_obs with the unread {k} NaN")
        c[k] = np.where(rd[k][..., None], case[k] + np.float32(0.5), case[k])                  # and every read one does matter
        got = tn.traj_next(**c)[3]
        changed = (f32_bits(got) != f32_bits(want[3])).all(axis=-1)
        sel = (acted & (want[0] < 0)) if k == "obs" else (acted & (want[0] >= 0))
        np.testing.assert_array_equal(changed, sel, err_msg=k)


def test_a_column_is_unaffected_by_its_neighbours():
    rng = np.random.default_rng(5)
    T, N, D = 31, 70, 2
    case = _case(T, N, seed=5, D=D)
    want = tn.traj_next(**case)
    perm = rng.permutation(N)
    got = tn.traj_next(**{k: v[:, perm] for k, v in case.items()})
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w[:, perm])
    one = tn.traj_next(**{k: v[:, 13:14] for k, v in case.items()})
    for g, w in zip(one, want):
        np.testing.assert_array_equal(g, w[:, 13:14])


def test_struct_symbol_and_headers():
    io = _abi.PhxTrajNextIO
    header = open(os.path.join(ROOT, "include", "phantom_amd_traj.h")).read()
    assert ctypes.sizeof(io) == 96 and "} phx_traj_next_io;                     /* 96 bytes */" in header
    offsets = dict(T=0, D=4, N=8, truncated=16, terminated=24, acted=32, new_obs_valid=40, obs=48, new_obs=56, next_row=64,
                   next_terminated=72, next_truncated=80, next_obs=88)
    assert {n: getattr(io, n).offset for n, _ in io._fields_} == offsets
    body = header[header.index("typedef struct phx_traj_next_io {"):header.index("} phx_traj_next_io;")]
    names = re.findall(r"(\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert names == [n for n, _ in io._fields_] == list(offsets)
    assert "int phx_traj_next(const phx_traj_next_io* io, void* stream);" in header
    lib = _abi.load_library()
    assert hasattr(lib, "phx_traj_next") and hasattr(lib, "phx_gae_masked") and hasattr(lib, "phx_vtrace")
    assert "phx_traj_next" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert _abi.TRAJ_NEXT_KERNEL == "phx_traj_next_kernel" and _abi.TRAJ_GATHER_KERNEL == "phx_traj_gather_kernel"
    for h in ("phantom_amd.h", "phantom_amd_gae.h", "phantom_amd_vtrace.h"):
        assert "phx_traj" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert ctypes.sizeof(_abi.PhxGaeIO) == 80 and ctypes.sizeof(_abi.PhxGaeMaskedIO) == 104 and ctypes.sizeof(_abi.PhxVtraceIO) == 112
    assert "phx_traj_next.hip" in build.SOURCES and any(h.endswith("phantom_amd_traj.h") for h in build.HEADERS)


def test_no_instantiation_of_the_kernels_uses_scratch(tmp_path):
    """every instantiation cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 (a spilled chunk buffer would
    put loads and stores into the scan, against the one rule the kernel is built on): eight of the scan, four of the gather"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_traj_next.hip"), "-o", str(tmp_path / "tn.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == 12
    assert sum("phx_traj_next_kernel" in n for n in names) == 8 and sum("phx_traj_gather_kernel" in n for n in names) == 4
    assert scratch == [0] * 12, dict(zip(names, scratch))


def _fragment(B=3, S=2, T=5, D=3, **kw):
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(B, S, T, D)).astype(np.float32)
    f = lambda: rng.normal(size=(B, S, T)).astype(np.float32)
    z = np.zeros((B, S, T), bool)
    t = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    return FragmentBatch(["a", "b"], obs, obs + 1, f(), f(), z, z.copy(), t, np.zeros((B, T), np.int64), **kw)


def test_fragment_batch_trajectory_columns():
    B, S, T, D = 3, 2, 5, 3
    rng = np.random.default_rng(1)
    fields = dict(trajectory_next_row=rng.integers(-1, T, (B, S, T)).astype(np.int32),
                  trajectory_new_obs=(1000 + np.arange(B * S * T * D, dtype=np.float32)).reshape(B, S, T, D),
                  trajectory_terminateds=rng.random((B, S, T)) < 0.3, trajectory_truncateds=rng.random((B, S, T)) < 0.3)
    column = dict(trajectory_new_obs="new_obs", trajectory_terminateds="terminateds", trajectory_truncateds="truncateds",
                  trajectory_next_row="trajectory_next_row")
    frag = _fragment(**fields)
    cols = frag.to_sample_batches()["default_policy"]
    for k, c in column.items():                                # rows in (env, agent, step) order
        np.testing.assert_array_equal(cols[c], fields[k].reshape((B * S * T,) + fields[k].shape[3:]), err_msg=k)
    # the step-aligned planes stay what they were (rollouts() reads them)
    assert frag.new_obs is not fields["trajectory_new_obs"] and not frag.terminateds.any() and not frag.truncateds.any()
    plain = _fragment()
    assert all(getattr(plain, k) is None for k in fields)
    today = plain.to_sample_batches()["default_policy"]
    assert set(today) == {"obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "eps_id", "agent_index", "t", "env_id"}
    np.testing.assert_array_equal(today["new_obs"], plain.new_obs.reshape(-1, D))
    np.testing.assert_array_equal(today["terminateds"], plain.terminateds.reshape(-1))
    np.testing.assert_array_equal(today["truncateds"], plain.truncateds.reshape(-1))
    assert set(cols) == set(today) | {"trajectory_next_row"}
    for k in set(today) - set(column.values()):                # the other columns do not change with the fields
        np.testing.assert_array_equal(cols[k], today[k], err_msg=k)
    valid = np.ones((B, S, T), np.uint8)
    valid[1, 0, 2] = valid[2, 1, 4] = valid[0, 0, 0] = 0
    keep = valid.reshape(-1).astype(bool)
    masked = _fragment(obs_valid=valid, **fields).to_sample_batches()["default_policy"]
    for k, c in column.items():                                # masked by obs_valid: the rows where the agent acted
        np.testing.assert_array_equal(masked[c], fields[k].reshape((B * S * T,) + fields[k].shape[3:])[keep], err_msg=k)
    assert len(masked["obs"]) == len(masked["new_obs"]) == B * S * T - 3
    per_policy = _fragment(obs_valid=valid, **fields).to_sample_batches(lambda aid: aid)
    for s, pid in enumerate("ab"):
        k1 = valid[:, s].reshape(-1).astype(bool)
        np.testing.assert_array_equal(per_policy[pid]["new_obs"], fields["trajectory_new_obs"][:, s].reshape(-1, D)[k1])
        np.testing.assert_array_equal(per_policy[pid]["truncateds"], fields["trajectory_truncateds"][:, s].reshape(-1)[k1])
        np.testing.assert_array_equal(per_policy[pid]["terminateds"], fields["trajectory_terminateds"][:, s].reshape(-1)[k1])
    assert FragmentBatch.COLUMNS == ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")
