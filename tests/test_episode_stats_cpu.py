"""CPU: the definition of phx_episode_stats (include/phantom_amd_episodes.h) as tests/episode_ref.py restates it -- against a plain
per-column double loop written from the header, split at any row with the carry handed over, the reduction to a sequential f32 sum,
early termination, NaN in what it does not read, the reduction's order against a literal transcription; the structs, the symbol, the
headers and the build lists; that the GPU test's cases are not vacuous; EpisodeStats.result()'s arithmetic."""
import ctypes
import itertools
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import episode_ref as er
from helpers import f32_bits
from phantom_amd import _abi, build
from phantom_amd.episodes import EpisodeStats

OPTIONAL = ("terminated", "acted", "reward_valid")
OTHER_HEADERS = ("phantom_amd.h", "phantom_amd_gae.h", "phantom_amd_vtrace.h", "phantom_amd_traj.h", "phantom_amd_compact.h",
                 "phantom_amd_nstep.h")
SRC = open(os.path.join(build.CSRC, "phx_episodes.hip")).read() if os.path.exists(os.path.join(build.CSRC, "phx_episodes.hip")) else ""
f32 = np.float32


def _planes(case, nulls=()):
    return {k: (None if k in nulls else v) for k, v in case.items()}


def _same(got, want, what=""):
    for k in ("episode_return", "carry_return"):
        np.testing.assert_array_equal(f32_bits(got[k]), f32_bits(want[k]), err_msg=what + k)
    for k in ("episode_len", "carry_len"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=what + k)
    er.assert_same_stats(got["col_stats"], want["col_stats"], what + "col_stats: ")
    er.assert_same_stats(got["summary"], want["summary"], what + "summary: ")


# ---- the header, a column and a scalar at a time ---------------------------------------------------------------------------------
def _f32_add(a, b):
    """the correctly rounded f32 sum of two f32 values, through f64 (exact there) and one rounding by struct"""
    s = float(a) + float(b)
    if math.isnan(s) or math.isinf(s):
        return f32(s)
    return f32(struct.unpack("<f", struct.pack("<f", s))[0])


def _plain_loop(reward, truncated, terminated, acted, reward_valid, G, K, carry):
    T, N = reward.shape
    C = N // G
    e_ret, e_len = np.zeros((T, C), f32), np.full((T, C), -1, np.int32)
    cols = []
    cr, cl = np.zeros(C, f32), np.full(C, -1, np.int32)
    for c in range(C):
        ret, ln = (f32(0.0), -1) if carry is None else (f32(carry[0][c]), int(carry[1][c]))
        st = dict(count=0, len_sum=0, ret_sum=0.0, ret_sumsq=0.0, ret_min=math.inf, ret_max=-math.inf, len_min=2 ** 31 - 1, len_max=-1)
        for t in range(T):
            any_act, all_flag = False, True
            for g in range(G):
                n = c * G + g
                present = reward_valid is None or reward_valid[t, n] == 1
                act = acted is None or acted[t, n] != 0
                if (present or act) and ln < 0:
                    ret, ln = f32(0.0), 0
                if present:
                    ret = _f32_add(ret, reward[t, n])
                any_act = any_act or act
                all_flag = all_flag and ((terminated is not None and terminated[t, n] != 0) or truncated[t, n] != 0)
            if any_act:
                ln += 1
            if all_flag and ln >= 0:
                e_ret[t, c], e_len[t, c] = ret, ln
                st["count"] += 1; st["len_sum"] += ln
                st["len_min"], st["len_max"] = min(st["len_min"], ln), max(st["len_max"], ln)
                st["ret_sum"] = st["ret_sum"] + float(ret)
                st["ret_sumsq"] = st["ret_sumsq"] + float(ret) * float(ret)
                st["ret_min"], st["ret_max"] = min(st["ret_min"], float(ret)), max(st["ret_max"], float(ret))
                ret, ln = f32(0.0), -1
        cr[c], cl[c] = ret, ln
        cols.append(st)
    col = er.empty(C)
    for c, st in enumerate(cols):
        for k, v in st.items():
            col[k][c] = v
    summary = er.empty(K)
    for k in range(K):
        members = [cols[c] for c in range(k, C, K)]
        summary["count"][k], summary["len_sum"][k] = sum(m["count"] for m in members), sum(m["len_sum"] for m in members)
        summary["len_min"][k], summary["len_max"][k] = min(m["len_min"] for m in members), max(m["len_max"] for m in members)
        summary["ret_min"][k], summary["ret_max"][k] = min(m["ret_min"] for m in members), max(m["ret_max"] for m in members)
        summary["ret_sum"][k] = _lane_tree([m["ret_sum"] for m in members])
        summary["ret_sumsq"][k] = _lane_tree([m["ret_sumsq"] for m in members])
    return dict(episode_return=e_ret, episode_len=e_len, col_stats=col, summary=summary, carry_return=cr, carry_len=cl)


def _lane_tree(x):
    """the header's reduction order, literally: lanes, then the tree"""
    a = [0.0] * 256
    for i in range(256):
        j = i
        while j < len(x):
            a[i] = a[i] + x[j]
            j += 256
    h = 128
    while h >= 1:
        for i in range(h):
            a[i] = a[i] + a[i + h]
        h //= 2
    return a[0]


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("K", [1, 3])
def test_restatement_equals_the_plain_loop_written_from_the_header(G, K):
    for T, C in ((1, 3), (5, 6), (17, 9), (40, 12)):
        case = er.case(T, C, G, seed=1)
        rng = np.random.default_rng([T, C, G])
        carry = (rng.normal(0, 3, C).astype(f32), rng.integers(-1, 4, C).astype(np.int32))
        for r in range(len(OPTIONAL) + 1):
            for nulls in itertools.combinations(OPTIONAL, r):
                for cy in (None, carry):
                    p = _planes(case, nulls)
                    got = er.episode_stats(G=G, K=K, carry=cy, **p)
                    _same(got, _plain_loop(G=G, K=K, carry=cy, **p), f"T={T} C={C} G={G} K={K} nulls={nulls} carry={cy is not None}: ")


@pytest.mark.parametrize("G", [1, 3])
def test_a_fragment_cut_at_any_row_with_the_carry_handed_over(G):
    T, C = 24, 9
    case = er.case(T, C, G, seed=2)
    whole = er.episode_stats(G=G, K=3, **case)
    assert (whole["col_stats"]["count"] >= 2).any() and (whole["carry_len"] >= 0).any()
    for cut in range(1, T):
        a = er.episode_stats(G=G, K=3, **{k: v[:cut] for k, v in case.items()})
        b = er.episode_stats(G=G, K=3, carry=(a["carry_return"], a["carry_len"]), **{k: v[cut:] for k, v in case.items()})
        for k in ("episode_return", "episode_len"):
            both = np.concatenate([a[k], b[k]])
            np.testing.assert_array_equal(f32_bits(both) if both.dtype == f32 else both, f32_bits(whole[k]) if both.dtype == f32 else whole[k],
                                          err_msg=f"cut {cut}: {k}")
        np.testing.assert_array_equal(f32_bits(b["carry_return"]), f32_bits(whole["carry_return"]))
        np.testing.assert_array_equal(b["carry_len"], whole["carry_len"])
        ca, cb, cw = a["col_stats"], b["col_stats"], whole["col_stats"]
        for f in ("count", "len_sum"):
            np.testing.assert_array_equal(ca[f] + cb[f], cw[f], err_msg=f"cut {cut}: {f}")
        for f in ("ret_min", "len_min"):
            np.testing.assert_array_equal(np.minimum(ca[f], cb[f]), cw[f], err_msg=f"cut {cut}: {f}")
        for f in ("ret_max", "len_max"):
            np.testing.assert_array_equal(np.maximum(ca[f], cb[f]), cw[f], err_msg=f"cut {cut}: {f}")


def test_reduction_one_plain_episode_is_the_sequential_f32_sum():
    T, N = 37, 11
    rng = np.random.default_rng(3)
    reward = (rng.normal(0, 1, (T, N)) * 10.0 ** rng.integers(-3, 3, (T, N))).astype(f32)
    truncated = np.zeros((T, N), np.uint8)
    truncated[T - 1] = 1
    got = er.episode_stats(reward, truncated)
    want = np.zeros(N, f32)
    for t in range(T):
        want = (want + reward[t]).astype(f32)
    np.testing.assert_array_equal(f32_bits(got["episode_return"][T - 1]), f32_bits(want))
    assert (got["episode_len"][T - 1] == T).all() and (got["episode_len"][:T - 1] == -1).all() and (got["col_stats"]["count"] == 1).all()
    assert (got["carry_len"] == -1).all() and (got["col_stats"]["len_sum"] == T).all()
    np.testing.assert_array_equal(got["col_stats"]["ret_sum"], want.astype(np.float64))
    np.testing.assert_array_equal(got["col_stats"]["ret_sumsq"], want.astype(np.float64) ** 2)


def test_an_agent_that_terminated_early_counts_one_episode_and_the_env_closes_where_all_are_flagged():
    T, S = 10, 3
    reward = np.ones((T, S), f32)
    acted = np.ones((T, S), np.uint8)
    valid = np.ones((T, S), np.uint8)
    term, trunc = np.zeros((T, S), np.uint8), np.zeros((T, S), np.uint8)
    term[3, 1] = 1                                      # agent 1 terminates in row 3 ..
    acted[4:, 1], valid[4:, 1] = 0, 0                   # .. neither acts nor is rewarded afterwards ..
    trunc[T - 1] = 1                                    # .. and sees the env's truncation with everybody else
    per_agent = er.episode_stats(reward, trunc, term, acted, valid, G=1, K=S)
    np.testing.assert_array_equal(per_agent["col_stats"]["count"], [1, 1, 1])
    np.testing.assert_array_equal(per_agent["col_stats"]["len_sum"], [T, 4, T])
    np.testing.assert_array_equal(per_agent["episode_len"][3], [-1, 4, -1])
    np.testing.assert_array_equal(per_agent["episode_len"][T - 1], [T, -1, T])
    np.testing.assert_array_equal(per_agent["summary"]["ret_sum"], [T, 4, T])
    env = er.episode_stats(reward, trunc, term, acted, valid, G=S, K=1)
    assert env["col_stats"]["count"][0] == 1 and env["episode_len"][T - 1, 0] == T and (env["episode_len"][:T - 1] == -1).all()
    assert env["episode_return"][T - 1, 0] == 2 * T + 4
    sticky = term.copy()
    sticky[3:, 1] = 1                                   # a sticky flag: the same
    _same(er.episode_stats(reward, trunc, sticky, acted, valid, G=1, K=S), per_agent)
    _same(er.episode_stats(reward, trunc, sticky, acted, valid, G=S, K=1), env)


def test_nan_in_the_unread_rewards_changes_nothing():
    for G in (1, 2):
        case = er.case(21, 8, G, seed=4)
        want = er.episode_stats(G=G, K=2, **case)
        poisoned = dict(case, reward=np.where(case["reward_valid"] == 1, case["reward"], f32(np.nan)))
        assert np.isnan(poisoned["reward"]).any()
        _same(er.episode_stats(G=G, K=2, **poisoned), want)
        assert not np.isnan(want["episode_return"]).any()


@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_the_reduction_order_against_a_literal_transcription(M):
    rng = np.random.default_rng(M)
    for K in (1, 3):
        col = er.empty(M * K)
        col["ret_sum"] = rng.normal(0, 1, M * K) * 10.0 ** rng.integers(-8, 8, M * K)
        col["ret_sumsq"] = col["ret_sum"] ** 2
        col["count"] = rng.integers(0, 5, M * K)
        col["len_sum"] = rng.integers(0, 50, M * K)
        col["ret_min"], col["ret_max"] = rng.normal(0, 1, M * K), rng.normal(0, 1, M * K)
        col["len_min"], col["len_max"] = rng.integers(0, 9, M * K), rng.integers(0, 9, M * K)
        got = er.reduce(col, K)
        for k in range(K):
            m = col[k::K]
            for f in er.SUM_FIELDS:
                want = _lane_tree([float(x) for x in m[f]])
                assert struct.pack("<d", got[f][k]) == struct.pack("<d", want), (M, K, k, f)
            assert got["count"][k] == sum(int(x) for x in m["count"]) and got["len_sum"][k] == sum(int(x) for x in m["len_sum"])
            assert got["ret_min"][k] == min(m["ret_min"]) and got["ret_max"][k] == max(m["ret_max"])
            assert got["len_min"][k] == min(m["len_min"]) and got["len_max"][k] == max(m["len_max"])
    if M >= 255:                                        # the order matters: a plain left-to-right sum rounds differently somewhere
        x = rng.normal(0, 1, (64, M)) * 10.0 ** rng.integers(-8, 8, (64, M))
        assert any(er.ordered_sum(row) != sum(float(v) for v in row) for row in x)


# ---- the structs, the symbol, the headers, the build lists --------------------------------------------------------------------------
def _declared(text):
    """the names a header declares: functions, struct / typedef names, macros (comments stripped)"""
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(phx_\w+)\s*\(", code)) | set(re.findall(r"}\s*(phx_\w+)\s*;", code))
    names |= set(re.findall(r"struct\s+(phx_\w+)", code)) | set(re.findall(r"#\s*define\s+(PHX_\w+|PHANTOM_\w+)", code))
    return names


def _c_layout(body, types):
    """(name, offset) of the fields in a struct body as C lays them out (natural alignment), and the size rounded to 8"""
    fields = re.findall(r"(" + "|".join(re.escape(t) for t in types) + r")\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    size = lambda t: 8 if t.endswith("*") or t in ("int64_t", "double") else 4
    at, out = 0, []
    for t, n in fields:
        at = -(-at // size(t)) * size(t)
        out.append((n, at))
        at += size(t)
    return out, -(-at // 8) * 8


def test_struct_symbol_headers_and_build_lists():
    header = open(os.path.join(ROOT, "include", "phantom_amd_episodes.h")).read()
    st, io = _abi.PhxEpisodeStats, _abi.PhxEpisodeIO
    st_off = dict(count=0, len_sum=8, ret_sum=16, ret_sumsq=24, ret_min=32, ret_max=36, len_min=40, len_max=44)
    io_off = dict(T=0, G=4, N=8, K=16, reserved0=20, reward=24, truncated=32, terminated=40, acted=48, reward_valid=56, carry_return=64,
                  carry_len=72, episode_return=80, episode_len=88, col_stats=96, summary=104)
    assert ctypes.sizeof(st) == 48 == np.dtype(_abi.EPISODE_STATS_DTYPE).itemsize == er.DTYPE.itemsize == _abi.EPISODE_STATS_BYTES
    assert ctypes.sizeof(io) == 112
    assert {n: getattr(st, n).offset for n, _ in st._fields_} == st_off and {n: getattr(io, n).offset for n, _ in io._fields_} == io_off
    assert np.dtype(_abi.EPISODE_STATS_DTYPE) == er.DTYPE and {n: er.DTYPE.fields[n][1] for n in er.DTYPE.names} == st_off
    body = header[header.index("struct phx_episode_stats {"):header.index("};", header.index("struct phx_episode_stats {"))]
    got, size = _c_layout(body, ("int64_t", "double", "float", "int32_t"))
    assert dict(got) == st_off and [n for n, _ in got] == list(st_off) and size == 48 and re.search(r"};\s*/\* 48 bytes \*/", header)
    body = header[header.index("typedef struct phx_episode_io {"):header.index("} phx_episode_io;")]
    got, size = _c_layout(body, ("int32_t*", "int32_t", "int64_t", "const float*", "const uint8_t*", "float*", "struct phx_episode_stats*"))
    assert dict(got) == io_off and [n for n, _ in got] == [n for n, _ in io._fields_] and size == 112
    assert re.search(r"} phx_episode_io;\s*/\* 112 bytes \*/", header)
    for n, at in {**st_off, **io_off}.items():          # the header states every offset next to its field
        line = next(l for l in header.splitlines() if re.search(rf"\b{n};", l) and "/*" in l)
        assert re.search(rf"/\*[\s\d,]*\b{at}\b", line), (n, at, line)
    assert "int phx_episode_stats(const phx_episode_io* io, void* stream);" in header
    mine = _declared(header)
    assert mine == {"phx_episode_stats", "phx_episode_io", "PHANTOM_AMD_EPISODES_H"}
    for h in OTHER_HEADERS:                             # it declares nothing of the other six, and they name nothing of it
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not (_declared(text) & mine), h
        assert "phx_episode" not in text and "phantom_amd_episodes" not in text, h
    assert "phx_episode_stats" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert (_abi.EPISODE_SCAN_KERNEL, _abi.EPISODE_REDUCE_KERNEL) == ("phx_episode_scan_kernel", "phx_episode_reduce_kernel")
    for name in (_abi.EPISODE_SCAN_KERNEL, _abi.EPISODE_REDUCE_KERNEL):
        assert re.search(rf'\.launched\("[^"\n]*", "{name}"\)', SRC)      # (FragCall::launched of phx_frag.h notes the name)
    assert "phx_note_kernel(kernel);" in open(os.path.join(build.CSRC, "phx_frag.h")).read()
    assert int(re.search(r"constexpr int EP_MAX_G = (\d+);", SRC).group(1)) == _abi.EPISODE_MAX_G == 256
    assert int(re.search(r"constexpr int EP_RED = (\d+);", SRC).group(1)) == er.LANES == 256
    assert re.search(r"constexpr int EP_K = (\d+);", SRC) and re.search(r"constexpr int EP_LANES = (\d+);", SRC)
    assert "phx_episodes.hip" in build.SOURCES and any(h.endswith("phantom_amd_episodes.h") for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS)
    lib = _abi.load_library()
    assert hasattr(lib, "phx_episode_stats") and lib.phx_episode_stats.argtypes[0]._type_ is io


def test_the_header_compiles_as_c_and_no_scan_kernel_uses_scratch(tmp_path):
    """the public header is C (the struct tag and the function share a name: no typedef); every instantiation cross-compiled for
    gfx950 with the build's own flags reports ScratchSize 0 -- sixteen scans and the reduction"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    src = tmp_path / "use.c"
    src.write_text('#include "phantom_amd_episodes.h"\nint use(const phx_episode_io* io) { struct phx_episode_stats s; s.count = 0; '
                   'return phx_episode_stats(io, 0) + (int)s.count + (int)sizeof(s); }\n')
    c_cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if c_cc:
        r = subprocess.run([c_cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_episodes.hip"), "-o", str(tmp_path / "ep.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == 17
    assert [sum(k in n for n in names) for k in ("phx_episode_scan_kernel", "phx_episode_reduce_kernel")] == [16, 1]
    assert scratch == [0] * 17, dict(zip(names, scratch))


# ---- the GPU test's cases ----------------------------------------------------------------------------------------------------------
def test_the_gpu_cases_are_not_vacuous():
    """for every (seed 0, shape) of tests/test_gpu_episode_stats.py with T >= 8: at least a quarter of the output columns close an
    episode, at least one ends with an episode open, at least one closes two"""
    ep_k = int(re.search(r"constexpr int EP_K = (\d+);", SRC).group(1))
    shapes = [s for s in er.gpu_shapes(ep_k) if s[0] >= 8]
    assert len(shapes) >= 20 and {s[2] for s in shapes} == {1, 2, 3}
    for T, C, G in shapes:
        want = er.episode_stats(G=G, **er.case(T, C, G))
        count = want["col_stats"]["count"]
        assert (count >= 1).sum() * 4 >= C, (T, C, G)
        assert (want["carry_len"] >= 0).any(), (T, C, G)
        assert (count >= 2).any(), (T, C, G)
        if C > 2:
            assert count[2] == 0 and want["carry_len"][2] == -1      # the column that never acts and never closes


# ---- EpisodeStats.result() ---------------------------------------------------------------------------------------------------------
class _Spec:
    agent_ids = ["a", "b", "c", "x"]
    strategic_idx = [0, 1, 2]
    n_strategic = 3


class _Env:
    spec, batch_size = _Spec, 4


def _records(rows):
    rec = er.empty(len(rows))
    for i, r in enumerate(rows):
        for k, v in r.items():
            rec[k][i] = v
    return rec


def test_episode_stats_result_arithmetic_without_a_gpu():
    st = EpisodeStats(_Env())
    empty = st.result()
    assert empty["episodes_this_iter"] == 0 and all(math.isnan(empty[k]) for k in ("episode_reward_mean", "episode_reward_min",
                                                                                     "episode_reward_max", "episode_len_mean"))
    assert set(empty["agent_reward_mean"]) == {"a", "b", "c"} and all(math.isnan(v) for v in empty["agent_reward_mean"].values())
    assert "policy_reward_mean" not in empty
    one = _records([dict(count=2, len_sum=7, ret_sum=3.0, ret_sumsq=5.0, ret_min=1.0, ret_max=2.0, len_min=3, len_max=4),
                    dict(),                             # agent b closed nothing
                    dict(count=1, len_sum=5, ret_sum=-4.5, ret_sumsq=20.25, ret_min=-4.5, ret_max=-4.5, len_min=5, len_max=5),
                    dict(count=1, len_sum=9, ret_sum=10.0, ret_sumsq=100.0, ret_min=10.0, ret_max=10.0, len_min=9, len_max=9)])
    two = _records([dict(count=1, len_sum=2, ret_sum=0.25, ret_sumsq=0.0625, ret_min=0.25, ret_max=0.25, len_min=2, len_max=2),
                    dict(), dict(),
                    dict(count=2, len_sum=11, ret_sum=-1.0, ret_sumsq=13.0, ret_min=-3.0, ret_max=2.0, len_min=5, len_max=6)])
    st.add_summaries(one)
    st.add_summaries(two)
    r = st.result(reset=False, policy_mapping_fn=lambda aid: "p0" if aid in ("a", "c") else "p1")
    assert r["episodes_this_iter"] == 3 and r["episode_reward_mean"] == 9.0 / 3 and r["episode_len_mean"] == 20 / 3
    assert (r["episode_reward_min"], r["episode_reward_max"]) == (-3.0, 10.0)
    assert r["agent_reward_mean"]["a"] == 3.25 / 3 and r["agent_reward_mean"]["c"] == -4.5 and math.isnan(r["agent_reward_mean"]["b"])
    assert r["agent_reward_min"]["a"] == 0.25 and r["agent_reward_max"]["a"] == 2.0 and math.isnan(r["agent_reward_min"]["b"])
    assert r["agent_episode_len_mean"]["a"] == 3.0 and r["agent_episode_len_mean"]["c"] == 5.0 and math.isnan(r["agent_episode_len_mean"]["b"])
    assert r["policy_reward_mean"] == {"p0": (3.25 - 4.5) / 4, "p1": pytest.approx(float("nan"), nan_ok=True)}
    assert r["policy_reward_min"]["p0"] == -4.5 and r["policy_reward_max"]["p0"] == 2.0 and math.isnan(r["policy_reward_max"]["p1"])
    again = st.result()                                 # reset=False kept the totals; this one clears them
    assert again["episodes_this_iter"] == 3 and "policy_reward_mean" not in again
    assert st.result()["episodes_this_iter"] == 0
    with_fn = EpisodeStats(_Env(), policy_mapping_fn=lambda aid: "shared")
    with_fn.add_summaries(one)
    assert with_fn.result()["policy_reward_mean"] == {"shared": (3.0 - 4.5) / 3}
    with pytest.raises(ValueError, match="records"):
        st.add_summaries(one[:2])
    st.drop_open()                                      # nothing on a device yet: nothing to do
