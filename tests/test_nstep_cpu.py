"""CPU: the definition of phx_nstep (include/phantom_amd_nstep.h) as tests/nstep_ref.py restates it -- against a plain double loop
written from the header, against adjust_nstep's formula in f64 on single plain episodes, the n = 1 identity, what it does not read,
the generator's coverage; the struct, the symbol, the headers and the build lists; no scratch in any instantiation of the kernels;
FragmentBatch's n-step columns."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import nstep_ref as ns
from helpers import f32_bits
from phantom_amd import _abi, build
from phantom_amd.rollout import NSTEP_COLUMNS, CompactFragment, FragmentBatch

SHAPES = [(1, 1), (1, 5), (2, 9), (7, 16), (16, 63), (17, 64), (33, 65), (40, 130)]
PLANES = ("reward", "truncated", "terminated", "acted", "next_row")
OPTIONAL = ("terminated", "acted", "next_row")
SIX = ns.OUTPUTS[:6]
OTHER_HEADERS = ("phantom_amd.h", "phantom_amd_gae.h", "phantom_amd_vtrace.h", "phantom_amd_traj.h", "phantom_amd_compact.h")


def _case(T, N, seed=0, D=None):
    return ns.random_case(np.random.default_rng([seed, T, N]), T, N, D=D)


def _bits(a):
    return f32_bits(a) if a.dtype == np.float32 else a


@pytest.mark.parametrize("T,N", SHAPES)
def test_restatement_equals_the_plain_loop_written_from_the_header(T, N):
    case = _case(T, N)
    for k, (n, gamma) in enumerate(((1, 0.99), (2, 0.5), (3, 0.99), (5, 1.0), (64, 0.0), (64, 0.97))):
        nulls = [c for r in range(4) for c in itertools.combinations(OPTIONAL, r)][(k + T) % 8]
        c = {p: (None if p in nulls else case[p]) for p in PLANES}
        got = ns.nstep(n=n, gamma=gamma, **c)
        want = ns.plain_loop(c["reward"], c["truncated"], c["terminated"], c["acted"], c["next_row"], n, gamma)
        if c["acted"] is not None:
            np.testing.assert_array_equal(got["succ_row"], want[0], err_msg=f"succ_row n={n} {nulls}")
        for name, w in zip(SIX, want[1:]):
            assert got[name].dtype == w.dtype and got[name].shape == (T, N)
            np.testing.assert_array_equal(_bits(got[name]), _bits(w), err_msg=f"{name} n={n} gamma={gamma} nulls={nulls}")
        hole = np.zeros((T, N), bool) if c["acted"] is None else c["acted"] == 0
        assert (f32_bits(got["nstep_reward"])[hole] == 0).all() and (f32_bits(got["nstep_discount"])[hole] == 0).all()
        assert (got["nstep_last"][hole] == -1).all() and (got["nstep_next_row"][hole] == -1).all()
        assert not got["nstep_terminated"][hole].any() and not got["nstep_truncated"][hole].any()
        assert not (got["nstep_terminated"] & got["nstep_truncated"]).any()
        rows = np.broadcast_to(np.arange(T)[:, None], (T, N))
        assert (got["nstep_last"][~hole] >= rows[~hole]).all() and (got["nstep_last"] < T).all()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 10, 64])
@pytest.mark.parametrize("gamma", [0.5, 0.99, 1.0])
def test_adjust_nstep_in_f64_on_single_plain_episodes(n, gamma):
    """one plain episode per column (no holes, the only flag in the last row): at row t, m = min(n, rows left),
    G = sum_{k < m} gamma^k r[t + k], new_obs and the flags of row t + m - 1, discount gamma^m.  The f32 chain rounds p at most n times
    and the sum at most n times, one half-ulp (2^-24 relative) each: |G32 - G64| <= 2 n 2^-24 sum_k |gamma^k r_k|"""
    T, N, D = 37, 12, 2
    rng = np.random.default_rng([n, int(gamma * 100)])
    r = (rng.normal(0, 1, (T, N)) * np.exp(rng.normal(0, 2, (T, N)))).astype(np.float32)
    trunc, term = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    trunc[T - 1, 0::2] = 1; term[T - 1, 1::2] = 1
    obs = rng.normal(size=(T, N, D)).astype(np.float32)
    got = ns.nstep(r, trunc, term, None, None, obs, n=n, gamma=gamma)
    g = np.float64(np.float32(gamma))
    r64 = r.astype(np.float64)
    for t in range(T):
        m = min(n, T - t)
        w = g ** np.arange(m)
        G64 = (w[:, None] * r64[t:t + m]).sum(axis=0)
        bound = 2 * n * 2.0 ** -24 * (w[:, None] * np.abs(r64[t:t + m])).sum(axis=0)
        assert (np.abs(got["nstep_reward"][t].astype(np.float64) - G64) <= bound).all(), (t, n, gamma)
        assert (np.abs(got["nstep_discount"][t].astype(np.float64) - g ** m) <= n * 2.0 ** -24 * g ** m).all()
        assert (got["nstep_last"][t] == t + m - 1).all() and (got["nstep_next_row"][t] == t + m - 1).all()
        np.testing.assert_array_equal(f32_bits(got["nstep_next_obs"][t]), f32_bits(obs[t + m - 1]))
        np.testing.assert_array_equal(got["nstep_terminated"][t], term[t + m - 1])
        np.testing.assert_array_equal(got["nstep_truncated"][t], trunc[t + m - 1])


def test_n_equals_one_is_the_identity_with_minus_zero_and_nan_in_the_unread():
    T, N, D = 33, 70, 3
    case = _case(T, N, seed=3, D=D)
    act = case["acted"] != 0
    bits = np.random.default_rng(3).integers(0, 2 ** 32, (T, N, D), dtype=np.uint64).astype(np.uint32)
    case["next_obs"] = bits.view(np.float32)
    case["reward"][0, :4] = np.float32(-0.0)
    case["acted"][0, :4] = 1
    act = case["acted"] != 0
    case["reward"] = np.where(act, case["reward"], np.float32(np.nan))             # unread: rewards at hole rows
    got = ns.nstep(n=1, gamma=0.37, **case)
    te = case["terminated"] != 0
    np.testing.assert_array_equal(f32_bits(got["nstep_reward"])[act], f32_bits(case["reward"])[act])
    assert (f32_bits(got["nstep_reward"][0, :4]) == 0x80000000).all()
    assert (f32_bits(got["nstep_discount"])[act] == f32_bits(np.float32(0.37))).all()
    rows = np.broadcast_to(np.arange(T)[:, None], (T, N))
    np.testing.assert_array_equal(got["nstep_last"][act], rows[act])
    np.testing.assert_array_equal(got["nstep_terminated"][act], te[act])
    np.testing.assert_array_equal(got["nstep_truncated"][act], (~te & (case["truncated"] != 0))[act])
    np.testing.assert_array_equal(got["nstep_next_row"][act], case["next_row"][act])
    np.testing.assert_array_equal(f32_bits(got["nstep_next_obs"])[act], bits[act])
    assert (f32_bits(got["nstep_next_obs"])[~act] == 0).all()
    plain = ns.nstep(case["reward"], case["truncated"], n=1, gamma=1.0)            # every plane NULL: rows are their own
    np.testing.assert_array_equal(f32_bits(plain["nstep_reward"]), f32_bits(case["reward"]))
    np.testing.assert_array_equal(plain["nstep_next_row"], rows)


@pytest.mark.parametrize("n", [2, 3, 64])
def test_unread_elements_do_not_matter_and_read_ones_do(n):
    T, N, D = 33, 70, 2
    case = _case(T, N, seed=9, D=D)
    want = ns.nstep(n=n, gamma=0.9, **case)
    planes = {p: case[p] for p in PLANES}
    rd = ns.reads(n=n, gamma=0.9, **planes)
    act = case["acted"] != 0
    assert rd["reward"].any() and not rd["reward"][~act].any() and rd["reward"][act].all()      # (a trajectory row reads its own reward)
    assert rd["next_obs"].any() and not rd["next_obs"][~act].any() and not rd["next_obs"].all()
    c = dict(case)
    c["reward"] = np.where(rd["reward"], case["reward"], np.float32(np.nan))
    c["next_obs"] = np.where(rd["next_obs"][..., None], case["next_obs"], np.float32(np.nan))
    got = ns.nstep(n=n, gamma=0.9, **c)
    for k in ns.OUTPUTS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
    c = dict(case)
    c["next_obs"] = np.where(rd["next_obs"][..., None], case["next_obs"] + np.float32(0.5), case["next_obs"])
    changed = (f32_bits(ns.nstep(n=n, gamma=0.9, **c)["nstep_next_obs"]) != f32_bits(want["nstep_next_obs"])).all(axis=-1)
    np.testing.assert_array_equal(changed, act)


def test_the_generator_leaves_no_chain_shape_out():
    """over the cases the GPU test runs (its shapes with T >= 15, its n): every stop reason occurs, and at least a quarter of the
    trajectory rows fold two or more transitions"""
    seen, rows, folded2 = set(), 0, 0
    for (T, N), n in itertools.product(((17, 65), (33, 64), (40, 257)), (1, 2, 3, 5, 64)):
        case = _case(T, N)
        planes = {p: case[p] for p in PLANES}
        m, stop = ns.stats(n=n, gamma=0.99, **planes)
        act = case["acted"] != 0
        assert (m[~act] == 0).all() and (stop[~act] == -1).all() and (m[act] >= 1).all() and (m <= n).all() and (stop[act] >= 0).all()
        seen |= {ns.STOPS[i] for i in np.unique(stop[act])}
        rows += int(act.sum()); folded2 += int((m >= 2).sum())
        if n >= 2:                                            # each case with n >= 2 on its own: every reason (n > T: no chain is n long)
            assert {ns.STOPS[i] for i in np.unique(stop[act])} == set(ns.STOPS) - ({"m_equals_n"} if n > T else set()), (T, N, n)
        assert not act[:, 10].any() and act[:, 11].all() and (m[:, 12] == np.minimum(n, T - np.arange(T))).all()
    assert seen == set(ns.STOPS)
    assert folded2 * 4 >= rows, (folded2, rows)


def test_a_column_is_unaffected_by_its_neighbours():
    T, N, D = 31, 70, 2
    case = _case(T, N, seed=5, D=D)
    want = ns.nstep(n=4, gamma=0.9, **case)
    perm = np.random.default_rng(5).permutation(N)
    got = ns.nstep(n=4, gamma=0.9, **{k: v[:, perm] for k, v in case.items()})
    for k in ns.OUTPUTS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k][:, perm]), err_msg=k)


def _declared(text):
    """the names a header declares: functions, struct / typedef names, macros (comments stripped)"""
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(phx_\w+)\s*\(", code)) | set(re.findall(r"}\s*(phx_\w+)\s*;", code))
    names |= set(re.findall(r"struct\s+(phx_\w+)", code)) | set(re.findall(r"#\s*define\s+(PHX_\w+|PHANTOM_\w+)", code))
    return names


def test_struct_symbol_headers_and_build_lists():
    io = _abi.PhxNstepIO
    header = open(os.path.join(ROOT, "include", "phantom_amd_nstep.h")).read()
    assert ctypes.sizeof(io) == 136 and re.search(r"} phx_nstep_io;\s*/\* 136 bytes \*/", header)
    offsets = dict(T=0, D=4, N=8, n=16, gamma=20, reward=24, truncated=32, terminated=40, acted=48, next_row=56, next_obs=64, succ_row=72,
                   nstep_reward=80, nstep_discount=88, nstep_last=96, nstep_terminated=104, nstep_truncated=112, nstep_next_row=120,
                   nstep_next_obs=128)
    assert {n: getattr(io, n).offset for n, _ in io._fields_} == offsets
    body = header[header.index("typedef struct phx_nstep_io {"):header.index("} phx_nstep_io;")]
    fields = re.findall(r"(int32_t|int64_t|float|const float\*|const uint8_t\*|const int32_t\*|int32_t\*|float\*|uint8_t\*)\s+(\w+);",
                        re.sub(r"/\*.*?\*/", "", body))
    assert [n for _, n in fields] == [n for n, _ in io._fields_] == list(offsets)
    size = lambda t: 8 if t.endswith("*") or t == "int64_t" else 4
    at = 0
    for t, n in fields:                                       # the C layout of the header's text: natural alignment, no padding needed
        at = -(-at // size(t)) * size(t)
        assert at == offsets[n], n
        at += size(t)
    assert at == 136
    assert "int phx_nstep(const phx_nstep_io* io, void* stream);" in header
    mine = _declared(header)
    assert mine == {"phx_nstep", "phx_nstep_io", "PHANTOM_AMD_NSTEP_H"}
    for h in OTHER_HEADERS:                                   # it declares nothing of the other five, and they nothing of it
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not (_declared(text) & mine), h
        assert "nstep" not in text, h
    assert "phx_nstep" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert (_abi.NSTEP_SUCC_KERNEL, _abi.NSTEP_FOLD_KERNEL, _abi.NSTEP_GATHER_KERNEL) == ("phx_nstep_succ_kernel", "phx_nstep_fold_kernel",
                                                                                         "phx_nstep_gather_kernel")
    src = open(os.path.join(build.CSRC, "phx_nstep.hip")).read()
    for name in (_abi.NSTEP_SUCC_KERNEL, _abi.NSTEP_FOLD_KERNEL, _abi.NSTEP_GATHER_KERNEL):
        assert re.search(rf'\.launched\("[^"\n]*", "{name}"\)', src)      # (FragCall::launched of phx_frag.h notes the name)
    assert "phx_note_kernel(kernel);" in open(os.path.join(build.CSRC, "phx_frag.h")).read()
    assert int(re.search(r"constexpr int NSTEP_MAX_N = (\d+);", src).group(1)) == _abi.NSTEP_MAX_N == 64
    assert "phx_nstep.hip" in build.SOURCES and any(h.endswith("phantom_amd_nstep.h") for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS)
    lib = _abi.load_library()
    assert hasattr(lib, "phx_nstep") and lib.phx_nstep.argtypes[0]._type_ is io


def test_no_instantiation_of_the_kernels_uses_scratch_and_denormals_are_kept(tmp_path):
    """every instantiation cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 -- one successor scan, eight
    folds, two gathers -- and no LDS; and the build's flags are what the header's (d) reads them as: nothing flushes f32 denormals"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    assert not any("denormal" in f or "fast-math" in f or f == "-Ofast" for f in build.FLAGS)
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_nstep.hip"), "-o", str(tmp_path / "ns.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == len(lds) == 11
    assert [sum(k in n for n in names) for k in ("phx_nstep_succ_kernel", "phx_nstep_fold_kernel", "phx_nstep_gather_kernel")] == [1, 8, 2]
    assert scratch == [0] * 11 and lds == [0] * 11, dict(zip(names, zip(scratch, lds)))


def _fragment(B=3, S=2, T=5, D=3, **kw):
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(B, S, T, D)).astype(np.float32)
    f = lambda: rng.normal(size=(B, S, T)).astype(np.float32)
    z = np.zeros((B, S, T), bool)
    t = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    return FragmentBatch(["a", "b"], obs, obs + 1, f(), f(), z, z.copy(), t, np.zeros((B, T), np.int64), **kw)


def test_fragment_batch_and_compact_fragment_nstep_columns():
    B, S, T, D = 3, 2, 5, 3
    rng = np.random.default_rng(1)
    fields = dict(nstep_rewards=rng.normal(size=(B, S, T)).astype(np.float32), nstep_discounts=rng.random((B, S, T)).astype(np.float32),
                  nstep_new_obs=(1000 + np.arange(B * S * T * D, dtype=np.float32)).reshape(B, S, T, D),
                  nstep_terminateds=rng.random((B, S, T)) < 0.3, nstep_truncateds=rng.random((B, S, T)) < 0.3)
    assert tuple(fields) == NSTEP_COLUMNS
    plain = _fragment()
    assert all(getattr(plain, k) is None for k in fields)
    today = plain.to_sample_batches()["default_policy"]
    assert set(today) == {"obs", "new_obs", "actions", "rewards", "terminateds", "truncateds", "eps_id", "agent_index", "t", "env_id"}
    cols = _fragment(**fields).to_sample_batches()["default_policy"]
    assert set(cols) == set(today) | set(fields)
    for k in today:                                           # the one-step columns stay as they are
        np.testing.assert_array_equal(cols[k], today[k], err_msg=k)
    for k, v in fields.items():
        assert cols[k].dtype == v.dtype
        np.testing.assert_array_equal(cols[k], v.reshape((B * S * T,) + v.shape[3:]), err_msg=k)
    one = _fragment(nstep_rewards=fields["nstep_rewards"]).to_sample_batches()["default_policy"]
    assert set(one) == set(today) | {"nstep_rewards"}         # a column per field that is present
    valid = np.ones((B, S, T), np.uint8)
    valid[1, 0, 2] = valid[2, 1, 4] = valid[0, 0, 0] = 0
    frag = _fragment(obs_valid=valid, **fields)
    masked = frag.to_sample_batches(lambda aid: aid)
    for s, pid in enumerate("ab"):
        keep = valid[:, s].reshape(-1).astype(bool)
        for k, v in fields.items():
            np.testing.assert_array_equal(masked[pid][k], v[:, s].reshape((B * T,) + v.shape[3:])[keep], err_msg=k)
    # the compact container carries them under the same names
    tm = lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0))          # [B, S, T, ..] -> [T, B, S, ..]
    columns = {k: tm(getattr(frag, k)) for k in FragmentBatch.COLUMNS}
    columns.update({k: tm(v) for k, v in fields.items()})
    for k in ("nstep_terminateds", "nstep_truncateds"):
        assert columns[k].dtype == bool
    comp = CompactFragment.from_time_major(frag.agent_ids, tm(valid), columns, frag.t, frag.eps_id)
    for policy_fn in (None, lambda aid: aid):
        got, want = comp.to_sample_batches(policy_fn), frag.to_sample_batches(policy_fn)
        assert set(got) == set(want)
        for pid in want:
            assert set(got[pid]) == set(want[pid])
            for k, w in want[pid].items():
                g = got[pid][k]
                assert g.dtype == w.dtype and g.shape == w.shape, (pid, k, g.dtype, w.dtype, g.shape, w.shape)
                assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (pid, k)
