"""CPU: the definition of phx_vtrace (include/phantom_amd_vtrace.h) as tests/vtrace_ref.py restates it -- the cases its generator
makes, RLlib's formula in f64 within a computed forward error bound, the reduction to phx_gae, the no-flag case against a literal
transcription of from_importance_weights, independence; the struct, the symbol and the header; no scratch in any instantiation of
the kernel; FragmentBatch's V-trace columns."""
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
import gae_ref
import vtrace_ref as vr
from helpers import f32_bits
from phantom_amd import _abi, build
from phantom_amd.rollout import FragmentBatch

SRC = open(os.path.join(build.CSRC, "phx_vtrace.hip")).read()
K = int(re.search(r"constexpr int VT_K = (\d+);", SRC).group(1))
WG = int(re.search(r"constexpr int VT_LANES = (\d+);", SRC).group(1))
NS = (1, 3, 63, 64, 65, 549, WG - 2, WG + 2, 4 * WG + 2)          # tests/test_gpu_vtrace.py's shapes
TS = (1, 2, K - 1, K, K + 1, 2 * K + 1, 100)
PARAMS = [dict(gamma=0.99, lam=0.95), dict(gamma=1.0, lam=1.0, rho_bar=2.0, c_bar=1.0, pg_rho_bar=0.5),
          dict(gamma=0.9, lam=0.0, rho_bar=0.5, c_bar=2.0, pg_rho_bar=2.0), dict(gamma=0.99, lam=1.0, rho_bar=1e9, c_bar=1.0, pg_rho_bar=1e9)]


def _case(T, N, seed=0):
    return vr.random_case(np.random.default_rng([seed, T, N]), T, N)


def test_the_generator_makes_every_branch_at_the_shapes_the_gpu_tests_use():
    """rho on both sides of each threshold the GPU tests use (0.5, 1, 2), both ends of the clamp, columns with ratio exactly 0 (where
    rho == 1.0f exactly) and every flag combination at rows 0 and T - 1, at every shape with at least a wave of columns"""
    every = [(0, 1), (1, 0), (1, 1)]
    for T, N in [(T, N) for N in NS for T in TS] + [(4 * K + 3, 61 * 9 * 5 + 1)]:
        case = _case(T, N)
        assert all(case[k].shape == (T, N) for k in case)
        assert case["behaviour_logp"].dtype == case["target_logp"].dtype == np.float32
        if N < WG - 2:
            continue
        for thresholds in ((1.0, 1.0, 1.0), (0.5, 2.0, 2.0), (2.0, 0.5, 0.5)):
            f = vr.features(case, thresholds)
            assert f["below"] == [True] * 3 and f["above"] == [True] * 3, (T, N, thresholds, f)
        assert f["clamp_low"] and f["clamp_high"] and f["ratio_zero_columns"] >= N // 7 and f["rho_one"], (T, N, f)
        assert all(c in f["flags_first"] for c in every) and all(c in f["flags_last"] for c in every), (T, N, f)
        assert (0, 0) in f["flags_first"]


@pytest.mark.parametrize("kw", PARAMS)
def test_restatement_against_rllibs_formula_in_f64(kw):
    """|f32 definition - f64 formula| <= 2 E, E the first-order forward bound vtrace_f64 computes in f64 from the f64 values; the factor 2
    covers the second-order terms (the margin tests/test_gae_cpu.py uses)"""
    T, N = 57, 96
    case = _case(T, N, seed=7)
    vs, pg = vr.vtrace(**case, **kw)
    v64, p64, e_vs, e_pg = vr.vtrace_f64(**case, **kw)
    assert vs.dtype == pg.dtype == np.float32 and np.isfinite(vs).all() and np.isfinite(pg).all()
    assert (np.abs(vs.astype(np.float64) - v64) <= 2 * e_vs).all()
    assert (np.abs(pg.astype(np.float64) - p64) <= 2 * e_pg).all()
    # (the bound is no loose number: at most T rows times a dozen half-ulps of terms of a few units, 57 * 12 * 3 * 2^-24 = 1.2e-4; with
    #  a threshold above e^20 a column's terms span nine decades and there is no such scale to hold it against)
    if max(kw.get(k, 1.0) for k in ("rho_bar", "c_bar", "pg_rho_bar")) > 2.0:
        return
    assert (e_vs / np.maximum(1.0, np.abs(v64))).max() < 1.2e-4 and (e_pg / np.maximum(1.0, np.abs(p64))).max() < 1.2e-4


@pytest.mark.parametrize("gamma,lam", [(0.99, 1.0), (0.99, 0.95), (1.0, 0.3)])
@pytest.mark.parametrize("thresholds", [(1.0, 1.0, 1.0), (1.5, 2.0, 1.0)])
def test_reduction_identical_logp_planes_give_gaes_value_target(gamma, lam, thresholds):
    case = _case(33, 130, seed=8)
    case["target_logp"] = case["behaviour_logp"]
    rho = vr.weights(case["behaviour_logp"], case["target_logp"], gamma, lam, *thresholds)[0]
    assert (f32_bits(rho) == f32_bits(np.float32(1.0))).all()
    vs, pg = vr.vtrace(**case, gamma=gamma, lam=lam, rho_bar=thresholds[0], c_bar=thresholds[1], pg_rho_bar=thresholds[2])
    g = {k: case[k] for k in ("reward", "truncated", "vf_pred", "vf_next", "terminated")}
    adv, vt = gae_ref.gae(gamma=gamma, lam=lam, **g)
    np.testing.assert_array_equal(f32_bits(vs), f32_bits(vt))
    # and at cut rows, where vs[t + 1] does not enter, pg_advantage is GAE's one-step (lambda = 0) advantage
    one_step, _ = gae_ref.gae(gamma=gamma, lam=0.0, **g)
    cut = (case["truncated"] != 0) | (case["terminated"] != 0)
    cut[-1] = True
    np.testing.assert_array_equal(f32_bits(pg[cut]), f32_bits(one_step[cut]))


def _from_importance_weights(log_rhos, discounts, rewards, values, bootstrap_value, clip_rho_threshold, clip_pg_rho_threshold):
    """ray/rllib/algorithms/impala/vtrace_torch.py from_importance_weights, line by line, in f64 numpy ([T, N] planes)"""
    rhos = np.exp(log_rhos)
    clipped_rhos = np.minimum(clip_rho_threshold, rhos)
    cs = np.minimum(1.0, rhos)
    values_t_plus_1 = np.concatenate([values[1:], bootstrap_value[None]], axis=0)
    deltas = clipped_rhos * (rewards + discounts * values_t_plus_1 - values)
    acc = np.zeros_like(bootstrap_value)
    vs_minus_v_xs = np.empty_like(values)
    for i in range(values.shape[0] - 1, -1, -1):
        acc = deltas[i] + discounts[i] * cs[i] * acc
        vs_minus_v_xs[i] = acc
    vs = vs_minus_v_xs + values
    vs_t_plus_1 = np.concatenate([vs[1:], bootstrap_value[None]], axis=0)
    clipped_pg_rhos = np.minimum(clip_pg_rho_threshold, rhos)
    return vs, clipped_pg_rhos * (rewards + discounts * vs_t_plus_1 - values)


@pytest.mark.parametrize("rho_bar,pg_rho_bar", [(1.0, 1.0), (2.0, 0.5)])
def test_without_flags_it_is_from_importance_weights(rho_bar, pg_rho_bar):
    T, N = 41, 70
    case = _case(T, N, seed=9)
    case["truncated"] = np.zeros((T, N), np.uint8)
    case["terminated"] = None
    gamma = np.float32(0.99)
    vs, pg = vr.vtrace(**case, gamma=gamma, lam=1.0, rho_bar=rho_bar, c_bar=1.0, pg_rho_bar=pg_rho_bar)
    v64, p64, e_vs, e_pg = vr.vtrace_f64(**case, gamma=gamma, lam=1.0, rho_bar=rho_bar, c_bar=1.0, pg_rho_bar=pg_rho_bar)
    d = lambda k: case[k].astype(np.float64)
    log_rhos = vr.log_ratio(case["behaviour_logp"], case["target_logp"]).astype(np.float64)
    want_vs, want_pg = _from_importance_weights(log_rhos, np.full((T, N), np.float64(gamma)), d("reward"), d("vf_pred"), d("vf_next")[T - 1],
                                                np.float64(np.float32(rho_bar)), np.float64(np.float32(pg_rho_bar)))
    np.testing.assert_allclose(v64, want_vs, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(p64, want_pg, rtol=1e-12, atol=1e-12)
    assert (np.abs(vs.astype(np.float64) - want_vs) <= 2 * e_vs + 1e-12 * np.abs(want_vs)).all()
    assert (np.abs(pg.astype(np.float64) - want_pg) <= 2 * e_pg + 1e-12 * np.abs(want_pg)).all()


def test_a_terminated_row_is_rllibs_discount_zero():
    """one termination in the middle of an otherwise uncut column == from_importance_weights with discounts[t] = 0 there (the rows
    before and after the termination are coupled by nothing else)"""
    T, N = 19, 8
    case = _case(T, N, seed=10)
    case["truncated"] = np.zeros((T, N), np.uint8)
    term = np.zeros((T, N), np.uint8)
    term[7] = 1
    case["terminated"] = term
    v64, p64, _, _ = vr.vtrace_f64(**case, gamma=0.97, lam=1.0)
    d = lambda k: case[k].astype(np.float64)
    disc = np.full((T, N), np.float64(np.float32(0.97)))
    disc[7] = 0.0
    want_vs, want_pg = _from_importance_weights(vr.log_ratio(case["behaviour_logp"], case["target_logp"]).astype(np.float64), disc, d("reward"),
                                                d("vf_pred"), d("vf_next")[T - 1], 1.0, 1.0)
    np.testing.assert_allclose(v64, want_vs, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(p64, want_pg, rtol=1e-12, atol=1e-12)


def test_unread_vf_next_elements_do_not_matter():
    case = _case(20, 16, seed=6)
    want = vr.vtrace(**case, rho_bar=2.0)
    reads = vr.reads_vf_next(case["terminated"], case["truncated"])
    case["vf_next"] = np.where(reads, case["vf_next"], np.float32(np.nan))
    got = vr.vtrace(**case, rho_bar=2.0)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(f32_bits(g), f32_bits(w))
    case["vf_next"] = np.where(reads, case["vf_next"] + np.float32(1), case["vf_next"])       # (and the read ones do)
    assert (f32_bits(vr.vtrace(**case, rho_bar=2.0)[0]) != f32_bits(want[0])).any()


def test_a_column_is_unaffected_by_its_neighbours():
    rng = np.random.default_rng(5)
    case = _case(31, 40, seed=5)
    want = vr.vtrace(**case, gamma=0.99, lam=0.9, rho_bar=1.5)
    perm = rng.permutation(40)
    got = vr.vtrace(**{k: v[:, perm] for k, v in case.items()}, gamma=0.99, lam=0.9, rho_bar=1.5)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(f32_bits(g), f32_bits(w[:, perm]))
    one = vr.vtrace(**{k: v[:, 17:18] for k, v in case.items()}, gamma=0.99, lam=0.9, rho_bar=1.5)
    for g, w in zip(one, want):
        np.testing.assert_array_equal(f32_bits(g), f32_bits(w[:, 17:18]))


def test_struct_symbol_and_headers():
    io = _abi.PhxVtraceIO
    header = open(os.path.join(ROOT, "include", "phantom_amd_vtrace.h")).read()
    assert ctypes.sizeof(io) == 112 and "} phx_vtrace_io;                        /* 112 bytes */" in header
    offsets = dict(T=0, reserved0=4, N=8, gamma=16, lambda_=20, rho_bar=24, c_bar=28, pg_rho_bar=32, reserved1=36, reward=40, vf_pred=48,
                   vf_next=56, behaviour_logp=64, target_logp=72, terminated=80, truncated=88, vs=96, pg_advantage=104)
    assert {n: getattr(io, n).offset for n, _ in io._fields_} == offsets
    # the header declares the fields in this order (lambda_ is `lambda` in C)
    body = header[header.index("typedef struct phx_vtrace_io {"):header.index("} phx_vtrace_io;")]
    names = re.findall(r"(\w+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert names == [n.rstrip("_") for n, _ in io._fields_]
    assert "int phx_vtrace(const phx_vtrace_io* io, void* stream);" in header
    lib = _abi.load_library()
    assert hasattr(lib, "phx_vtrace") and hasattr(lib, "phx_gae") and hasattr(lib, "phx_gae_masked")
    assert "phx_vtrace" not in _abi.EXPORTS and _abi.ABI_VERSION == 10 and _abi.VTRACE_KERNEL == "phx_vtrace_kernel"
    assert "phx_vtrace" not in open(os.path.join(ROOT, "include", "phantom_amd.h")).read()
    assert "phx_vtrace" not in open(os.path.join(ROOT, "include", "phantom_amd_gae.h")).read()
    assert ctypes.sizeof(_abi.PhxGaeIO) == 80 and ctypes.sizeof(_abi.PhxGaeMaskedIO) == 104


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
                        os.path.join(build.CSRC, "phx_vtrace.hip"), "-o", str(tmp_path / "vt.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == len(vgprs) == 4 and all("phx_vtrace_kernel" in n for n in names)
    assert scratch == [0] * 4, dict(zip(names, scratch))
    assert "phx_vtrace.hip" in build.SOURCES and any(h.endswith("phantom_amd_vtrace.h") for h in build.HEADERS)


def _fragment(B=3, S=2, T=5, D=3, **kw):
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(B, S, T, D)).astype(np.float32)
    f = lambda: rng.normal(size=(B, S, T)).astype(np.float32)
    z = np.zeros((B, S, T), bool)
    t = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    return FragmentBatch(["a", "b"], obs, obs + 1, f(), f(), z, z.copy(), t, np.zeros((B, T), np.int64), **kw)


def test_fragment_batch_vtrace_columns():
    B, S, T = 3, 2, 5
    names = ("vf_preds", "target_logp", "vtrace_vs", "vtrace_pg_advantages")
    planes = {k: (100 * i + np.arange(B * S * T, dtype=np.float32)).reshape(B, S, T) for i, k in enumerate(names)}
    frag = _fragment(**planes)
    assert frag.advantages is None and frag.value_targets is None
    cols = frag.to_sample_batches()["default_policy"]
    for k, p in planes.items():                                # rows in (env, agent, step) order
        np.testing.assert_array_equal(cols[k], p.reshape(-1))
        assert cols[k].shape == cols["rewards"].shape
    assert "advantages" not in cols and "value_targets" not in cols
    plain = _fragment()
    assert plain.target_logp is None and plain.vtrace_vs is None and plain.vtrace_pg_advantages is None
    assert not set(names) & set(plain.to_sample_batches()["default_policy"])
    per_policy = frag.to_sample_batches(lambda aid: aid)
    np.testing.assert_array_equal(per_policy["b"]["vtrace_vs"], planes["vtrace_vs"][:, 1].reshape(-1))
    assert FragmentBatch.COLUMNS == ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")
