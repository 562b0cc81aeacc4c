"""CPU: the definition of phx_gae_masked (include/phantom_amd_gae.h) as tests/gae_masked_ref.py restates it -- its compaction
to gae_ref.gae per column, its reduction to gae_ref.gae without the two masks, what it does not read; the struct, the symbol
and the headers; FragmentBatch's trajectory_rewards; and the resource usage of every instantiation of the kernel."""
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
import gae_masked_ref as gm
import gae_ref
from helpers import f32_bits
from phantom_amd import _abi, build
from phantom_amd.rollout import FragmentBatch

SHAPES = [(1, 5), (2, 9), (17, 70), (33, 130)]
GL = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.5)]


def _case(T, N, seed=0):
    return gm.random_case(np.random.default_rng([seed, T, N]), T, N)


@pytest.mark.parametrize("T,N", SHAPES)
def test_the_generator_makes_the_cases_the_scan_can_get_wrong(T, N):
    case = _case(T, N)
    assert case["acted"].shape == case["reward_valid"].shape == (T, N) and case["acted"].dtype == case["reward_valid"].dtype == np.uint8
    if N >= 63 and T >= 15:
        f = gm.features(case)
        for k in ("no_trajectory_row", "last_row_not_acted", "first_row_not_acted", "two_cut_rows", "trunc_cut_on_hole", "term_cut_on_hole",
                  "no_present_reward"):
            assert f[k], k
        assert f["reward_valid_values"] == [0, 1, 2]
        assert f["densities"] == [0.1, 0.5, 1.0]


@pytest.mark.parametrize("gamma,lam", GL)
@pytest.mark.parametrize("T,N", SHAPES)
def test_compaction_per_column_against_gae(T, N, gamma, lam):
    """the outputs at a column's trajectory rows are gae_ref.gae's on the column compacted to those rows, bit for bit; zeros elsewhere"""
    case = _case(T, N)
    adv, vt, rs = gm.gae_masked(gamma=gamma, lam=lam, **case)
    hole = case["acted"] == 0
    for out in (adv, vt, rs):
        assert out.dtype == np.float32 and (f32_bits(out[hole]) == 0).all()
    for n in range(N):
        rows, planes, sums = gm.compact(case, n)
        assert rows == np.flatnonzero(case["acted"][:, n]).tolist()
        if not rows:
            continue
        a, v = gae_ref.gae(gamma=gamma, lam=lam, **planes)
        np.testing.assert_array_equal(f32_bits(adv[rows, n]), f32_bits(a[:, 0]), err_msg=f"advantage, column {n}")
        np.testing.assert_array_equal(f32_bits(vt[rows, n]), f32_bits(v[:, 0]), err_msg=f"value_target, column {n}")
        np.testing.assert_array_equal(f32_bits(rs[rows, n]), f32_bits(sums), err_msg=f"reward_sum, column {n}")


@pytest.mark.parametrize("gamma,lam", GL)
def test_reduction_without_the_masks_is_gae(gamma, lam):
    rng = np.random.default_rng(8)
    case = gae_ref.random_case(rng, 33, 130)
    for k in ("reward", "vf_next", "vf_pred"):                       # -0.0 sprinkled in: the first present reward is assigned, not added to +0.0
        case[k][rng.random(case[k].shape) < 0.1] = np.float32(-0.0)
    want = gae_ref.gae(gamma=gamma, lam=lam, **case)
    for extra in ({}, dict(acted=np.ones((33, 130), np.uint8), reward_valid=np.ones((33, 130), np.uint8))):
        adv, vt, rs = gm.gae_masked(gamma=gamma, lam=lam, **case, **extra)
        np.testing.assert_array_equal(f32_bits(adv), f32_bits(want[0]))
        np.testing.assert_array_equal(f32_bits(vt), f32_bits(want[1]))
        np.testing.assert_array_equal(f32_bits(rs), f32_bits(case["reward"]))
    for drop in ("vf_pred", "vf_next", "terminated"):
        c = dict(case); c[drop] = None
        got, want = gm.gae_masked(gamma=gamma, lam=lam, **c), gae_ref.gae(gamma=gamma, lam=lam, **c)
        np.testing.assert_array_equal(f32_bits(got[0]), f32_bits(want[0]))
        np.testing.assert_array_equal(f32_bits(got[1]), f32_bits(want[1]))


def test_unread_elements_do_not_matter():
    case = _case(33, 130)
    want = gm.gae_masked(gamma=0.99, lam=0.95, **case)
    rd = gm.reads(case["truncated"], case["terminated"], case["acted"], case["reward_valid"])
    assert not rd["reward"][case["reward_valid"] != 1].any() and (rd["reward"] != (case["reward_valid"] == 1)).any()
    assert (rd["vf_pred"] == (case["acted"] != 0)).all() and 0 < rd["vf_next"].sum() < (case["acted"] != 0).sum()
    for k in ("vf_next", "vf_pred", "reward"):
        c = dict(case)
        c[k] = np.where(rd[k], case[k], np.float32(np.nan))
        for got, w, name in zip(gm.gae_masked(gamma=0.99, lam=0.95, **c), want, ("advantage", "value_target", "reward_sum")):
            np.testing.assert_array_equal(f32_bits(got), f32_bits(w), err_msg=f"{name} with the unread {k} NaN")
    for k in ("vf_next", "vf_pred", "reward"):                       # and every element reads() names does matter to some output
        c = dict(case)
        c[k] = np.where(rd[k], case[k] + np.float32(1), case[k])
        got = gm.gae_masked(gamma=0.99, lam=0.95, **c)
        assert any((f32_bits(g) != f32_bits(w)).any() for g, w in zip(got, want)), k


def test_a_column_is_unaffected_by_its_neighbours():
    rng = np.random.default_rng(5)
    case = _case(31, 70)
    want = gm.gae_masked(gamma=0.99, lam=0.9, **case)
    perm = rng.permutation(70)
    got = gm.gae_masked(gamma=0.99, lam=0.9, **{k: v[:, perm] for k, v in case.items()})
    for g, w in zip(got, want):
        np.testing.assert_array_equal(f32_bits(g), f32_bits(w[:, perm]))
    one = gm.gae_masked(gamma=0.99, lam=0.9, **{k: v[:, 13:14] for k, v in case.items()})
    for g, w in zip(one, want):
        np.testing.assert_array_equal(f32_bits(g), f32_bits(w[:, 13:14]))


def test_struct_symbol_and_headers():
    io = _abi.PhxGaeMaskedIO
    assert ctypes.sizeof(io) == 104 and io.reward.offset == 24 and io.acted.offset == 64 and io.reward_valid.offset == 72
    assert io.advantage.offset == 80 and io.reward_sum.offset == 96
    assert ctypes.sizeof(_abi.PhxGaeIO) == 80
    lib = _abi.load_library()
    assert hasattr(lib, "phx_gae_masked") and hasattr(lib, "phx_gae")
    assert "phx_gae_masked" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert _abi.GAE_MASKED_KERNEL == "phx_gae_masked_kernel" and _abi.GAE_KERNEL == "phx_gae_kernel"
    new = open(os.path.join(ROOT, "include", "phantom_amd_gae.h")).read()
    old = open(os.path.join(ROOT, "include", "phantom_amd.h")).read()
    assert "int phx_gae_masked(const phx_gae_masked_io* io, void* stream);" in new
    assert "int phx_gae(const phx_gae_io* io, void* stream);" in new
    assert "phx_gae" not in old
    assert "phx_gae_masked.hip" in build.SOURCES


def _fragment(B=3, S=2, T=5, D=3, **kw):
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(B, S, T, D)).astype(np.float32)
    f = lambda: rng.normal(size=(B, S, T)).astype(np.float32)
    z = np.zeros((B, S, T), bool)
    t = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    return FragmentBatch(["a", "b"], obs, obs + 1, f(), f(), z, z.copy(), t, np.zeros((B, T), np.int64), **kw)


def test_fragment_batch_trajectory_rewards():
    B, S, T = 3, 2, 5
    tr = (1000 + np.arange(B * S * T, dtype=np.float32)).reshape(B, S, T)
    frag = _fragment(trajectory_rewards=tr)
    cols = frag.to_sample_batches()["default_policy"]
    np.testing.assert_array_equal(cols["rewards"], tr.reshape(-1))
    assert "trajectory_rewards" not in cols and frag.rewards is not tr          # the step-aligned plane stays what it was (rollouts() reads it)
    plain = _fragment()
    assert plain.trajectory_rewards is None
    np.testing.assert_array_equal(plain.to_sample_batches()["default_policy"]["rewards"], plain.rewards.reshape(-1))
    valid = np.ones((B, S, T), np.uint8)
    valid[1, 0, 2] = valid[2, 1, 4] = valid[0, 0, 0] = 0
    masked = _fragment(obs_valid=valid, trajectory_rewards=tr).to_sample_batches()["default_policy"]
    np.testing.assert_array_equal(masked["rewards"], tr.reshape(-1)[valid.reshape(-1).astype(bool)])
    assert len(masked["obs"]) == len(masked["rewards"]) == B * S * T - 3
    per_policy = _fragment(obs_valid=valid, trajectory_rewards=tr).to_sample_batches(lambda aid: aid)
    np.testing.assert_array_equal(per_policy["b"]["rewards"], tr[:, 1].reshape(-1)[valid[:, 1].reshape(-1).astype(bool)])
    np.testing.assert_array_equal(per_policy["a"]["rewards"], tr[:, 0].reshape(-1)[valid[:, 0].reshape(-1).astype(bool)])
    assert FragmentBatch.COLUMNS == ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")


def test_no_instantiation_of_the_kernel_uses_scratch(tmp_path):
    """every instantiation cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 (a spilled chunk buffer would
    put loads and stores into the chain, against the one rule the kernel is built on)"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_gae_masked.hip"), "-o", str(tmp_path / "gmk.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == len(vgprs) == 32 and all("phx_gae_masked_kernel" in n for n in names)
    assert scratch == [0] * 32, dict(zip(names, scratch))
