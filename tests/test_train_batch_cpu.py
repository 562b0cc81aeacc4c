"""CPU: the definition of phx_train_batch (include/phantom_amd_batch.h) as tests/batch_ref.py restates it -- the vectorised restatement
against the per-element loop, perm_K as a bijection and as a shuffle, the unshuffled columns against tests/compact_ref.py, the
standardized column against f64; the structs against the header as a C compiler lays them out, the symbol, no scratch in any kernel;
DeviceBatch's minibatches and TrainBatcher's epoch counter on hand-made buffers."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import batch_ref as br
import compact_ref as cr
from phantom_amd import _abi, build

SHAPES = [(1, 1), (1, 5), (2, 9), (7, 16), (9, 65), (17, 33), (3, 257)]
ELEM_BYTES = (1, 4, 12, 20, 4)                                   # (the last one holds f32: the standardized plane)
SEEDS = (0, 1, 0xDEADBEEF12345678)


def _sources(rng, T, N):
    src = [cr.plane_case(rng, T, N, eb) for eb in ELEM_BYTES[:-1]]
    return src + [(3.0 * rng.standard_normal((T, N)) + 1.0).astype(np.float32).view(np.uint32)]


@pytest.mark.parametrize("T,N", SHAPES)
def test_the_two_restatements_agree(T, N):
    offs, row_words = br.default_layout(ELEM_BYTES)
    assert offs == [0, 1, 2, 5, 10] and row_words == 16
    for i, density in enumerate(cr.DENSITIES):
        rng = np.random.default_rng([i, T, N])
        keep = cr.keep_case(rng, T, N, density)
        planes = list(zip(_sources(rng, T, N), offs))
        K = int((keep != 0).sum())
        for kw in (dict(shuffle=1, std_plane=4, seed=SEEDS[i % 3], epoch=i), dict(shuffle=0, std_plane=-1), dict(shuffle=1, std_plane=4, capacity=max(K - 1, 0)),
                   dict(shuffle=1, std_plane=4, keep=None), dict(shuffle=1, col_class=np.array([1, 0, 1], np.uint8)[:3 if N % 3 == 0 else 1],
                                                                 class_id=1, std_plane=4, seed=3)):
            kw = {"keep": keep, **kw}
            a = br.train_batch(T, N, planes, row_words, **kw)
            b = br.train_batch_loop(T, N, planes, row_words, **kw)
            br.same(a, b)
            if kw.get("capacity") is not None and K > 0:
                assert a["records"] is None and a["moments"]["count"] == K      # a permutation cannot be clipped
            elif a["records"] is not None:
                assert sorted(zip(a["out_col"].tolist(), a["out_row"].tolist())) == [tuple(x) for x in np.argwhere(br.kept_mask(
                    T, N, kw["keep"], kw.get("col_class"), kw.get("class_id", 0)).T).tolist()]
                assert (a["records"][:, 11:] == 0).all()          # the words no plane covers


@pytest.mark.parametrize("seed", SEEDS)
def test_perm_is_a_bijection(seed):
    for K in (0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4096, 4097, 65537):
        walks = []
        q = br.perm(K, seed, 0, walks=walks)
        assert q.dtype == np.int64 and q.shape == (K,)
        assert np.array_equal(np.sort(q), np.arange(K)), K
        keys = br.round_keys(seed, 0)
        for p in sorted({0, K // 3, K - 1} & set(range(K))):      # the loop restatement's walk ends at the same record
            assert br.perm_one(p, K, keys) == q[p]
        assert K <= 1 or walks[0] <= 64                           # (the expected trip count is below 4)
        assert np.array_equal(br.perm(K, seed, 0, shuffle=0), np.arange(K))
    assert all(0 <= k < 2 ** 32 for k in br.round_keys(seed, 5)) and br.round_keys(seed, 5) != br.round_keys(seed, 6)
    assert [br.half_bits(K) for K in (2, 4, 5, 16, 17, 64, 65, 4 ** 31)] == [1, 1, 2, 2, 3, 3, 4, 31]


def test_epochs_are_as_far_apart_as_seeds():
    """the positions two shuffles share: for two independent uniform permutations their number is Poisson(1) distributed, so the sum
    over 8 pairs is Poisson(8), which exceeds 24 with probability below 1e-5.  Epochs of one seed must do no worse than seeds"""
    K = 4096
    by_epoch = sum(int((br.perm(K, s, 0) == br.perm(K, s, 1)).sum()) for s in range(8))
    by_seed = sum(int((br.perm(K, s, 0) == br.perm(K, s + 8, 0)).sum()) for s in range(8))
    assert by_epoch <= 24 and by_seed <= 24, (by_epoch, by_seed)


def test_perm_shuffles():
    K = 4096
    p = np.arange(K)
    for seed in tuple(range(8)) + SEEDS:
        q = br.perm(K, seed, 0)
        fixed, disp = int((q == p).sum()), float(np.abs(q - p).mean()) / K
        assert fixed <= 16 and 0.30 <= disp <= 0.37, (seed, fixed, disp)


@pytest.mark.parametrize("T,N", SHAPES)
def test_unshuffled_columns_are_compact_refs_dense_arrays(T, N):
    offs, row_words = br.default_layout(ELEM_BYTES)
    for i, density in enumerate(cr.DENSITIES):
        rng = np.random.default_rng([i, T, N, 1])
        keep = cr.keep_case(rng, T, N, density)
        src = _sources(rng, T, N)
        got = br.train_batch(T, N, list(zip(src, offs)), row_words, keep=keep, shuffle=0)
        start, out_row, out_col, dense = cr.compact(keep, {str(k): s for k, s in enumerate(src)})
        assert (got["start"] == start).all() and (got["out_row"] == out_row).all() and (got["out_col"] == out_col).all()
        for k, s in enumerate(src):
            w = 1 if s.ndim == 2 else s.shape[2]
            col = got["records"][:, offs[k]:offs[k] + w]
            assert (col == dense[str(k)].astype(np.uint32).reshape(-1, w)).all(), (density, k)


@pytest.mark.parametrize("T,N", [(1, 1), (2, 3), (8, 64), (17, 257), (65, 1025)])
def test_the_standardized_column_against_f64(T, N):
    for i, density in enumerate((1.0, 0.5, 0.1)):
        rng = np.random.default_rng([i, T, N, 2])
        keep = (rng.random((T, N)) < density).astype(np.uint8)
        x = (3.0 * rng.standard_normal((T, N)) + 1.0).astype(np.float32)
        got = br.train_batch(T, N, [(x.view(np.uint32), 0)], 4, keep=keep, shuffle=1, seed=i, std_plane=0)
        K = got["K"]
        assert K == int(keep.sum()) and got["moments"]["count"] == K
        if K == 0:
            assert got["moments"].tobytes() == np.array((0, 0.0, 0.0, 0.0, 1e-4), br.MOMENTS_DTYPE).tobytes()
            continue
        kept = x[keep != 0].astype(np.float64)
        ref = (x.astype(np.float64) - kept.mean()) / max(1e-4, kept.std())
        val = got["records"][:, 0].view(np.float32).astype(np.float64)
        want = ref[got["out_row"], got["out_col"]]
        excess = np.abs(val - want) - 1e-6 * np.abs(want)
        print(f"T={T} N={N} density={density}: K={K}, worst excess over the relative term {excess.max():.3g}")
        assert (excess <= 1e-6).all(), (T, N, density, excess.max())
        assert (got["records"][:, 1:] == 0).all()


def test_struct_symbol_and_header(tmp_path):
    io, plane, mom = _abi.PhxTrainBatchIO, _abi.PhxBatchPlane, _abi.PhxBatchMoments
    header = open(os.path.join(ROOT, "include", "phantom_amd_batch.h")).read()
    assert "#define PHX_BATCH_MAX_PLANES 32" in header and _abi.BATCH_MAX_PLANES == 32
    assert "int phx_train_batch(const phx_train_batch_io* io, void* stream);" in header
    for struct, name in ((io, "phx_train_batch_io"), (plane, "phx_batch_plane"), (mom, "phx_batch_moments")):
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
        names = re.findall(r"(\w+)(?:\[\w+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
        assert names == [n for n, _ in struct._fields_], names
    # the sizes and offsets a C compiler gives the header's structs
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [("phx_train_batch_io", n) for n, _ in io._fields_] + [("phx_batch_plane", n) for n, _ in plane._fields_] + \
             [("phx_batch_moments", n) for n, _ in mom._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phantom_amd_batch.h"\nint main(void) {\n' +
                   '  printf("%zu %zu %zu\\n", sizeof(phx_train_batch_io), sizeof(phx_batch_plane), sizeof(phx_batch_moments));\n' +
                   "".join(f'  printf("%zu\\n", offsetof({s}, {f}));\n' for s, f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out[:3]] == [ctypes.sizeof(io), ctypes.sizeof(plane), ctypes.sizeof(mom)] == [656, 16, 32]
    want = [getattr(s, n).offset for s in (io, plane, mom) for n, _ in s._fields_]
    assert [int(x) for x in out[3:]] == want
    assert "} phx_train_batch_io;               /* 656 bytes */" in header and np.dtype(_abi.BATCH_MOMENTS_DTYPE).itemsize == 32
    assert np.dtype(_abi.BATCH_MOMENTS_DTYPE) == br.MOMENTS_DTYPE
    lib = _abi.load_library()
    assert hasattr(lib, "phx_train_batch") and "phx_train_batch" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert _abi.BATCH_KERNELS == "phx_batch_count_kernel+phx_batch_scan_kernel+phx_batch_moments_kernel+phx_batch_scatter_kernel"
    assert _abi.BATCH_KERNELS in header
    assert (_abi.BATCH_COUNT_KERNEL, _abi.BATCH_SCAN_KERNEL, _abi.BATCH_MOMENTS_KERNEL, _abi.BATCH_SCATTER_KERNEL) == tuple(_abi.BATCH_KERNELS.split("+"))
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "phantom_amd_batch.h":
            assert "phx_train_batch" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert "phx_train_batch.hip" in build.SOURCES and any(h.endswith("phantom_amd_batch.h") for h in build.HEADERS)
    assert lib.phx_train_batch(None, None) == -1 and b"phx_train_batch" in lib.phx_last_error()      # refused before any launch


def test_no_kernel_uses_scratch(tmp_path):
    """every kernel of the file cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 (a spilled stage buffer
    would put loads and stores into the scatter's store phase) and leaves room for at least 2 waves per SIMD"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_train_batch.hip"), "-o", str(tmp_path / "tb.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == len(occupancy) == 4
    assert [sum(k in n for n in names) for k in _abi.BATCH_KERNELS.split("+")] == [1, 1, 1, 1]
    assert scratch == [0] * 4, dict(zip(names, scratch))
    assert min(occupancy) >= 2, dict(zip(names, occupancy))


# ---- DeviceBatch and TrainBatcher on hand-made buffers ----------------------------------------------------------------------------
def _hand_made(T=5, N=6, seed=4):
    import torch
    rng = np.random.default_rng(seed)
    keep = cr.keep_case(rng, T, N, "random 0.5")
    obs = rng.standard_normal((T, N, 3)).astype(np.float32)
    rew = rng.standard_normal((T, N)).astype(np.float32)
    term = (rng.random((T, N)) < 0.3).astype(np.uint8) * 7           # (any non-zero byte is a set flag)
    nrow = rng.integers(-1, T, (T, N)).astype(np.int32)
    res = br.train_batch(T, N, [(obs.view(np.uint32), 0), (rew.view(np.uint32), 3), (term, 4), (nrow.view(np.uint32), 5)], 16, keep=keep, seed=seed)
    layout = {"obs": (0, 3, torch.float32, (3,)), "rewards": (3, 1, torch.float32, ()), "terminateds": (4, 1, torch.uint8, ()),
              "trajectory_next_row": (5, 1, torch.int32, ())}
    cap = T * N
    records = torch.full((cap, 16), -1515870811, dtype=torch.int32)
    records[:res["K"]] = torch.from_numpy(res["records"].view(np.int32))
    pad = lambda a: torch.from_numpy(np.concatenate([a, np.full(cap - len(a), -7, np.int32)]))
    return res, dict(obs=obs, rewards=rew, terminateds=term, trajectory_next_row=nrow), (records, layout, torch.from_numpy(res["start"]),
                                                                                          pad(res["out_row"]), pad(res["out_col"]))


def test_device_batch_columns_and_minibatches():
    import torch
    from phantom_amd.rollout import DeviceBatch
    res, src, args = _hand_made()
    db = DeviceBatch(*args)
    K = res["K"]
    assert db._count is None and db.count == K == len(db) and 0 < K < args[0].shape[0]        # one lazy read of start[N]
    t, n = res["out_row"], res["out_col"]
    assert (db.row.numpy() == t).all() and (db.col.numpy() == n).all()
    cols = db.columns
    assert list(cols) == ["obs", "rewards", "terminateds", "trajectory_next_row"]
    assert cols["obs"].dtype == torch.float32 and tuple(cols["obs"].shape) == (K, 3) and tuple(cols["rewards"].shape) == (K,)
    assert cols["terminateds"].dtype == torch.bool and cols["trajectory_next_row"].dtype == torch.int32
    for name in ("obs", "rewards", "trajectory_next_row"):
        assert cols[name].numpy().tobytes() == np.ascontiguousarray(src[name][t, n]).tobytes(), name
        assert cols[name].data_ptr() == args[0].data_ptr() + 4 * args[1][name][0]               # a strided view of the records
    assert (cols["terminateds"].numpy() == (src["terminateds"][t, n] != 0)).all()
    for size in (1, 4, K, K + 3):
        for drop_last in (False, True):
            mbs = list(db.minibatches(size, drop_last=drop_last))
            full, rest = divmod(K, size)
            assert [len(mb["rewards"]) for mb in mbs] == [size] * full + ([rest] if rest and not drop_last else [])
            assert all(set(mb) == set(cols) for mb in mbs)
            got = np.concatenate([mb["obs"].numpy() for mb in mbs]) if mbs else np.zeros((0, 3), np.float32)
            assert got.tobytes() == cols["obs"].numpy()[:len(got)].tobytes()                   # contiguous slices, in record order
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="size"):
            next(db.minibatches(bad))
    known = DeviceBatch(*args, count=3)
    assert known.count == 3 and tuple(known.columns["obs"].shape) == (3, 3)
    over = DeviceBatch(args[0][:K - 1], *args[1:])
    with pytest.raises(RuntimeError, match="fit"):
        over.count


class _Spec:
    agent_ids = ["exo", "a", "b", "c", "d", "e"]
    strategic_idx = [1, 2, 3, 4, 5]
    n_strategic = 5


class _Env:
    spec, batch_size = _Spec, 2


class _Dev:
    """stands in for DeviceEnv.train_batch: records what it was asked for"""
    device = "cpu"

    def __init__(self):
        self.asked = []

    def train_batch(self, planes, **kw):
        import torch
        self.asked.append(kw)
        lay, off = {}, 0
        for name, x in planes.items():
            w = x.shape[3] if x.dim() == 4 else 1
            lay[name] = (off, w, x.dtype)
            off += w
        cap = kw["capacity"]
        return torch.zeros(11, dtype=torch.int64), torch.zeros((cap, 16), dtype=torch.int32), torch.zeros(cap, dtype=torch.int32), \
            torch.zeros(cap, dtype=torch.int32), None, lay


def test_train_batcher_counts_epochs_and_maps_policies():
    import torch
    import phantom_amd as ph
    tb = ph.TrainBatcher(_Env, seed=9, policy_mapping_fn=lambda aid: "x" if aid in "ace" else "y")
    assert tb.agent_ids == ["a", "b", "c", "d", "e"] and (tb.B, tb.S) == (2, 5) and tb.calls == 0 and tb.standardize == "advantages"
    assert tb.policies == {"x": [0, 2, 4], "y": [1, 3]} and tb.col_class.tolist() == [0, 1, 0, 1, 0] and tb.col_class.dtype == np.uint8
    dev, T = _Dev(), 3
    planes = {"obs": torch.zeros(T, 2, 5, 3), "rewards": torch.zeros(T, 2, 5), "advantages": torch.zeros(T, 2, 5)}
    keep = torch.ones(T, 2, 5, dtype=torch.uint8)
    for call in range(3):
        out = tb.collect(dev, planes, keep if call else None)
        assert tb.calls == call + 1 and list(out) == ["x", "y"]
        asked = dev.asked[-2:]
        assert [a["class_id"] for a in asked] == [0, 1] and [a["epoch"] for a in asked] == [call, call] and all(a["seed"] == 9 for a in asked)
        assert [a["capacity"] for a in asked] == [T * 2 * 3, T * 2 * 2] and all(a["standardize"] == "advantages" and a["shuffle"] for a in asked)
        assert all(a["col_class"].tolist() == [0, 1, 0, 1, 0] for a in asked)
        assert [b._count for b in out.values()] == ([None, None] if call else [18, 12])      # known without a wait where nothing is masked
        assert out["x"].layout["obs"] == (0, 3, torch.float32, (3,)) and out["x"].layout["advantages"] == (4, 1, torch.float32, ())
    one = ph.TrainBatcher(_Env, standardize=None)
    assert one.policies == {"default_policy": [0, 1, 2, 3, 4]} and one.standardize is None
    one.collect(dev, {"rewards": planes["rewards"]})
    assert dev.asked[-1]["col_class"] is None and dev.asked[-1]["standardize"] is None and dev.asked[-1]["epoch"] == 0
    tb.collect(dev, {"rewards": planes["rewards"]})                                          # no such column in this fragment: nothing standardized
    assert dev.asked[-1]["standardize"] is None and dev.asked[-1]["epoch"] == 3
    with pytest.raises(ValueError, match="one column"):
        ph.TrainBatcher(_Env, standardize=("advantages", "value_targets"))
    with pytest.raises(ValueError, match="seed"):
        ph.TrainBatcher(_Env, seed=-1)
    with pytest.raises(ValueError, match="expected"):
        tb.collect(dev, {"rewards": torch.zeros(T, 2, 4)})
