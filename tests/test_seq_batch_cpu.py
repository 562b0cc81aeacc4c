"""CPU: the definition of phx_seq_batch (include/phantom_amd_seq.h) as tests/seq_ref.py restates it -- the vectorised restatement against
the per-element loop, the two reductions to phx_train_batch (L = 1; shuffle = 0), the slot and sequence properties; the struct against
the header as a C compiler lays it out, the symbol, no scratch in any kernel; DeviceSeqBatch and TrainBatcher(max_seq_len=) on hand-made
buffers."""
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
import seq_ref as sr
from phantom_amd import _abi, build

SHAPES = [(1, 1), (1, 5), (2, 9), (7, 16), (9, 65), (17, 33), (3, 257)]
ELEM_BYTES = (1, 4, 12, 20, 4)                                   # (the last one holds f32: the standardized plane)
SEEDS = (0, 1, 0xDEADBEEF12345678)


def _lens(T):
    return sorted({L for L in (1, 2, 3, T - 1, T, T + 5) if L >= 1})


def _sources(rng, T, N):
    src = [cr.plane_case(rng, T, N, eb) for eb in ELEM_BYTES[:-1]]
    return src + [(3.0 * rng.standard_normal((T, N)) + 1.0).astype(np.float32).view(np.uint32)]


def _flag_planes(rng, T, N, L, keep):
    """random flags, plus the placed ones: on the first row, the last row, two consecutive rows and the L-th kept row of a column; what
    is not kept holds garbage"""
    term = (rng.random((T, N)) < 0.15).astype(np.uint8) * rng.integers(1, 256, (T, N)).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.1).astype(np.uint8)
    term[0, 0] = 1
    trunc[T - 1, N - 1] = 3
    if T > 2:
        term[1, N // 2] = trunc[2, N // 2] = 1
    n = N // 3
    kept_rows = np.flatnonzero(keep[:, n])
    if len(kept_rows) >= L:
        term[:kept_rows[L - 1], n] = trunc[:kept_rows[L - 1], n] = 0
        term[kept_rows[L - 1], n] = 9                              # a flag on the L-th row: one sequence closes, not two
    holes = keep == 0
    term[holes] = rng.integers(0, 256, int(holes.sum())).astype(np.uint8)
    trunc[holes] = rng.integers(0, 256, int(holes.sum())).astype(np.uint8)
    return term, trunc


def check_properties(res, T, N, L, k, flags):
    """what the header promises of a complete result, from the outputs alone"""
    Q, K = res["Q"], res["K"]
    assert K == int(k.sum()) and res["seq_start"][N] == Q and (np.diff(res["seq_start"]) >= 0).all()
    if res["records"] is None:
        return
    lens, row, col = res["seq_lens"], res["out_row"].reshape(Q, L), res["out_col"].reshape(Q, L)
    assert int(lens.sum()) == K and ((lens >= 1) & (lens <= L)).all()            # no sequence is empty
    pad = np.arange(L)[None, :] >= lens[:, None]
    assert ((row == -1) == pad).all() and ((col == -1) == pad).all()            # a slot is a kept element's or padding, never both
    assert (res["records"].reshape(Q, L, res["records"].shape[1])[pad] == 0).all()
    assert sorted(zip(col[~pad].tolist(), row[~pad].tolist())) == [tuple(x) for x in np.argwhere(k.T).tolist()]      # each exactly once
    if Q:
        assert (res["seq_row"] == row[:, 0]).all() and (res["seq_col"] == col[:, 0]).all()
        assert ((col == col[:, :1]) | pad).all()                                  # one column per sequence
        assert (np.diff(row, axis=1)[~pad[:, 1:]] > 0).all()                      # rows in time order
    f = np.zeros((Q, L), bool)
    f[~pad] = flags[row[~pad], col[~pad]]
    last = np.arange(L)[None, :] == (lens - 1)[:, None]
    assert not (f & ~last).any()                                                 # a flagged row is its sequence's last
    # a sequence that is neither full nor flagged is its column's last
    short = (lens < L) & ~f[np.arange(Q), lens - 1] if Q else np.zeros(0, bool)
    for s in np.flatnonzero(short):
        n, t_last = res["seq_col"][s], row[s, lens[s] - 1]
        assert not k[t_last + 1:, n].any()


@pytest.mark.parametrize("T,N", SHAPES)
def test_the_two_restatements_agree(T, N):
    offs, row_words = br.default_layout(ELEM_BYTES)
    case = 0
    for L in _lens(T):
        for i, density in enumerate(cr.DENSITIES):
            rng = np.random.default_rng([i, T, N, L])
            keep = cr.keep_case(rng, T, N, density)
            if i == 1 and N > 2:
                keep[:, 1] = 0                                     # a column that keeps nothing
            term, trunc = _flag_planes(rng, T, N, L, keep)
            planes = list(zip(_sources(rng, T, N), offs))
            variants = (dict(shuffle=1, std_plane=4, seed=SEEDS[i % 3], epoch=i, terminated=term, truncated=trunc),
                        dict(shuffle=0, std_plane=-1, terminated=term), dict(shuffle=1, std_plane=4, truncated=trunc, keep=None),
                        dict(shuffle=1, std_plane=4, seed=3, terminated=term, truncated=trunc,
                             col_class=np.array([1, 0, 1], np.uint8)[:3 if N % 3 == 0 else 1], class_id=1),
                        dict(shuffle=1, seed=5))
            kw = {"keep": keep, **variants[case % len(variants)]}
            case += 1
            a = sr.seq_batch(T, N, planes, row_words, L, **kw)
            b = sr.seq_batch_loop(T, N, planes, row_words, L, **kw)
            sr.same(a, b)
            k = br.kept_mask(T, N, kw["keep"], kw.get("col_class"), kw.get("class_id", 0))
            check_properties(a, T, N, L, k, sr._flags(T, N, kw.get("terminated"), kw.get("truncated")))
            assert (a["records"][:, 11:] == 0).all()
            if a["Q"] > 0:                                         # the capacity rule: one sequence too few writes nothing
                c = sr.seq_batch(T, N, planes, row_words, L, capacity=a["Q"] - 1, **kw)
                sr.same(c, sr.seq_batch_loop(T, N, planes, row_words, L, capacity=a["Q"] - 1, **kw))
                assert c["records"] is None and c["seq_lens"] is None and c["seq_start"].tobytes() == a["seq_start"].tobytes()
                assert (c["moments"] is None) == (a["moments"] is None) and (c["moments"] is None or c["moments"].tobytes() == a["moments"].tobytes())
                sr.same(a, sr.seq_batch(T, N, planes, row_words, L, capacity=a["Q"], **kw))


def test_nothing_kept_gives_no_sequence():
    T, N = 5, 7
    planes = [(np.arange(T * N, dtype=np.uint32).reshape(T, N), 0)]
    for fn in (sr.seq_batch, sr.seq_batch_loop):
        res = fn(T, N, planes, 4, 3, keep=np.zeros((T, N), np.uint8), terminated=np.ones((T, N), np.uint8), std_plane=0)
        assert res["Q"] == 0 == res["K"] and res["records"].shape == (0, 4) and res["seq_lens"].shape == (0,) and not res["seq_start"].any()
        assert res["moments"].tobytes() == np.array((0, 0.0, 0.0, 0.0, 1e-4), br.MOMENTS_DTYPE).tobytes()


def test_a_flag_on_the_lth_row_closes_one_sequence():
    T, N, L = 6, 1, 3
    x = np.arange(T, dtype=np.uint32).reshape(T, 1)
    term = np.zeros((T, 1), np.uint8)
    term[2, 0] = 1
    res = sr.seq_batch(T, N, [(x, 0)], 4, L, terminated=term, shuffle=0)
    assert res["Q"] == 2 and res["seq_lens"].tolist() == [3, 3] and res["seq_row"].tolist() == [0, 3]
    term[1, 0] = 1                                               # flags on consecutive rows: a sequence of one row
    res = sr.seq_batch(T, N, [(x, 0)], 4, L, terminated=term, shuffle=0)
    assert res["seq_lens"].tolist() == [2, 1, 3] and res["out_row"].tolist() == [0, 1, -1, 2, -1, -1, 3, 4, 5]
    assert res["records"][:, 0].tolist() == [0, 1, 0, 2, 0, 0, 3, 4, 5]


@pytest.mark.parametrize("T,N", SHAPES)
def test_with_sequences_of_one_row_it_is_train_batch(T, N):
    offs, row_words = br.default_layout(ELEM_BYTES)
    for i, density in enumerate(cr.DENSITIES):
        rng = np.random.default_rng([i, T, N, 7])
        keep = cr.keep_case(rng, T, N, density)
        term, trunc = _flag_planes(rng, T, N, 1, keep)
        planes = list(zip(_sources(rng, T, N), offs))
        for std in (-1, 4):
            kw = dict(keep=keep, shuffle=1, seed=SEEDS[i % 3], epoch=i, std_plane=std)
            got = sr.seq_batch(T, N, planes, row_words, 1, terminated=term, truncated=trunc, **kw)
            want = br.train_batch(T, N, planes, row_words, **kw)
            assert got["Q"] == got["K"] == want["K"] and (got["seq_lens"] == 1).all()
            for a, b in (("seq_start", "start"), ("records", "records"), ("out_row", "out_row"), ("out_col", "out_col")):
                assert got[a].tobytes() == want[b].tobytes(), (a, density)
            assert (got["seq_row"] == want["out_row"]).all() and (got["seq_col"] == want["out_col"]).all()
            assert std < 0 or got["moments"].tobytes() == want["moments"].tobytes()


@pytest.mark.parametrize("T,N", SHAPES)
def test_unshuffled_sequences_concatenate_to_the_unshuffled_train_batch(T, N):
    offs, row_words = br.default_layout(ELEM_BYTES)
    for L in _lens(T):
        for i, density in enumerate(cr.DENSITIES):
            rng = np.random.default_rng([i, T, N, L, 9])
            keep = cr.keep_case(rng, T, N, density)
            term, trunc = _flag_planes(rng, T, N, L, keep)
            planes = list(zip(_sources(rng, T, N), offs))
            for std in (-1, 4):
                got = sr.seq_batch(T, N, planes, row_words, L, keep=keep, terminated=term, truncated=trunc, shuffle=0, std_plane=std)
                want = br.train_batch(T, N, planes, row_words, keep=keep, shuffle=0, std_plane=std)
                real = (np.arange(L)[None, :] < got["seq_lens"][:, None]).reshape(-1)
                assert got["records"][real].tobytes() == want["records"].tobytes()
                assert got["out_row"][real].tobytes() == want["out_row"].tobytes() and got["out_col"][real].tobytes() == want["out_col"].tobytes()
                assert std < 0 or got["moments"].tobytes() == want["moments"].tobytes()


def test_struct_symbol_and_header(tmp_path):
    io = _abi.PhxSeqBatchIO
    header = open(os.path.join(ROOT, "include", "phantom_amd_seq.h")).read()
    assert '#include "phantom_amd_batch.h"' in header and "#define PHX_SEQ_MAX_LEN 65536" in header and _abi.SEQ_MAX_LEN == 65536
    assert "int phx_seq_batch(const phx_seq_batch_io* io, void* stream);" in header
    body = header[header.index("typedef struct phx_seq_batch_io {"):header.index("} phx_seq_batch_io;")]
    names = re.findall(r"(\w+)(?:\[\w+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert names == [n for n, _ in io._fields_], names
    stated = [int(x) for x in re.findall(r"/\* (\d+) ", body)]
    assert stated == [getattr(io, n).offset for n, _ in io._fields_]             # every offset is stated in the header
    assert "} phx_seq_batch_io;                 /* 704 bytes */" in header and ctypes.sizeof(io) == 704
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phantom_amd_seq.h"\nint main(void) {\n' +
                   '  printf("%zu\\n", sizeof(phx_seq_batch_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(phx_seq_batch_io, {f}));\n' for f, _ in io._fields_) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(io) == 704
    assert out[1:] == [getattr(io, n).offset for n, _ in io._fields_]
    lib = _abi.load_library()
    assert hasattr(lib, "phx_seq_batch") and "phx_seq_batch" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    assert _abi.SEQ_KERNELS == "phx_seq_count_kernel+phx_seq_scan_kernel+phx_seq_moments_kernel+phx_seq_scatter_kernel"
    assert _abi.SEQ_KERNELS in header and all(k.startswith("phx_seq_") for k in _abi.SEQ_KERNELS.split("+"))
    assert (_abi.SEQ_COUNT_KERNEL, _abi.SEQ_SCAN_KERNEL, _abi.SEQ_MOMENTS_KERNEL, _abi.SEQ_SCATTER_KERNEL) == tuple(_abi.SEQ_KERNELS.split("+"))
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "phantom_amd_seq.h":
            assert "phx_seq_batch" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert "phx_seq_batch.hip" in build.SOURCES and any(h.endswith("phantom_amd_seq.h") for h in build.HEADERS)
    assert lib.phx_seq_batch(None, None) == -1 and b"phx_seq_batch" in lib.phx_last_error()          # refused before any launch


def test_no_kernel_uses_scratch(tmp_path):
    """every kernel of the file cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 and leaves room for at least
    2 waves per SIMD"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_seq_batch.hip"), "-o", str(tmp_path / "sq.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == len(set(names)) == len(scratch) == len(occupancy) == 4
    assert all("phx_seq_" in n for n in names)
    assert [sum(k in n for n in names) for k in _abi.SEQ_KERNELS.split("+")] == [1, 1, 1, 1]
    assert scratch == [0] * 4, dict(zip(names, scratch))
    assert min(occupancy) >= 2, dict(zip(names, occupancy))


# ---- DeviceSeqBatch and TrainBatcher(max_seq_len=) on hand-made buffers -----------------------------------------------------------
def _hand_made(T=7, N=6, L=3, seed=4, spare=2):
    import torch
    rng = np.random.default_rng(seed)
    keep = cr.keep_case(rng, T, N, "random 0.5")
    obs = rng.standard_normal((T, N, 3)).astype(np.float32)
    rew = rng.standard_normal((T, N)).astype(np.float32)
    term = (rng.random((T, N)) < 0.3).astype(np.uint8) * 7           # (any non-zero byte is a set flag)
    res = sr.seq_batch(T, N, [(obs.view(np.uint32), 0), (rew.view(np.uint32), 3), (term, 4)], 16, L, keep=keep, terminated=term, seed=seed)
    layout = {"obs": (0, 3, torch.float32, (3,)), "rewards": (3, 1, torch.float32, ()), "terminateds": (4, 1, torch.uint8, ())}
    Q, cap = res["Q"], res["Q"] + spare
    records = torch.full((cap, L, 16), -1515870811, dtype=torch.int32)
    records[:Q] = torch.from_numpy(res["records"].view(np.int32).reshape(Q, L, 16))
    pad = lambda a, shape: torch.from_numpy(np.concatenate([a.reshape((Q,) + shape), np.full((spare,) + shape, -7, np.int32)]))
    args = (records, layout, torch.from_numpy(res["seq_start"]), pad(res["seq_lens"], ()), pad(res["seq_row"], ()), pad(res["seq_col"], ()),
            pad(res["out_row"], (L,)), pad(res["out_col"], (L,)))
    return res, dict(obs=obs, rewards=rew, terminateds=term), args


def test_device_seq_batch_columns_mask_and_minibatches():
    import torch
    from phantom_amd.rollout import DeviceSeqBatch
    res, src, args = _hand_made()
    sb = DeviceSeqBatch(*args)
    Q, K, L = res["Q"], res["K"], 3
    assert sb._q is None and sb.num_sequences == Q == len(sb) and 1 < Q < args[0].shape[0] and sb.count == K and sb.max_seq_len == L
    assert (sb.seq_lens.numpy() == res["seq_lens"]).all() and (sb.seq_row.numpy() == res["seq_row"]).all() and (sb.seq_col.numpy() == res["seq_col"]).all()
    mask = sb.mask
    assert mask.dtype == torch.bool and tuple(mask.shape) == (Q, L) and (mask.numpy() == (np.arange(L)[None] < res["seq_lens"][:, None])).all()
    assert int(mask.sum()) == K and tuple(sb.row.shape) == tuple(sb.col.shape) == (Q, L)
    assert ((sb.row.numpy() == -1) == ~mask.numpy()).all() and ((sb.col.numpy() == -1) == ~mask.numpy()).all()
    t, n = sb.row.numpy()[mask.numpy()], sb.col.numpy()[mask.numpy()]
    cols = sb.columns
    assert list(cols) == ["obs", "rewards", "terminateds"]
    assert cols["obs"].dtype == torch.float32 and tuple(cols["obs"].shape) == (Q, L, 3) and tuple(cols["rewards"].shape) == (Q, L)
    assert cols["terminateds"].dtype == torch.bool and tuple(cols["terminateds"].shape) == (Q, L)
    for name in ("obs", "rewards"):
        assert cols[name].numpy()[mask.numpy()].tobytes() == np.ascontiguousarray(src[name][t, n]).tobytes(), name
        assert (cols[name].numpy()[~mask.numpy()] == 0).all()
        assert cols[name].data_ptr() == args[0].data_ptr() + 4 * args[1][name][0]               # a strided view of the records
    assert (cols["terminateds"].numpy()[mask.numpy()] == (src["terminateds"][t, n] != 0)).all()
    for size in (1, 2, Q, Q + 3):
        for drop_last in (False, True):
            mbs = list(sb.minibatches(size, drop_last=drop_last))
            full, rest = divmod(Q, size)
            assert [len(mb["seq_lens"]) for mb in mbs] == [size] * full + ([rest] if rest and not drop_last else [])
            assert all(set(mb) == set(cols) | {"seq_lens", "mask"} for mb in mbs)
            assert all(tuple(mb["obs"].shape[1:]) == (L, 3) and tuple(mb["mask"].shape[1:]) == (L,) for mb in mbs)
            got = np.concatenate([mb["obs"].numpy() for mb in mbs]) if mbs else np.zeros((0, L, 3), np.float32)
            assert got.tobytes() == cols["obs"].numpy()[:len(got)].tobytes()                   # whole sequences, in record order
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_sequences"):
            next(sb.minibatches(bad))
    over = DeviceSeqBatch(args[0][:Q - 1], *args[1:])
    with pytest.raises(RuntimeError, match="fit"):
        over.num_sequences
    with pytest.raises(RuntimeError, match="fit"):
        DeviceSeqBatch(args[0][:Q - 1], *args[1:]).count


class _Spec:
    agent_ids = ["exo", "a", "b", "c", "d", "e"]
    strategic_idx = [1, 2, 3, 4, 5]
    n_strategic = 5


class _Env:
    spec, batch_size, num_steps = _Spec, 2, 4


class _Dev:
    """stands in for DeviceEnv.seq_batch: records what it was asked for; train_batch must not be called"""
    device = "cpu"

    def __init__(self):
        self.asked = []

    def seq_batch(self, planes, max_seq_len, **kw):
        import torch
        self.asked.append(dict(kw, max_seq_len=max_seq_len))
        lay, off = {}, 0
        for name, x in planes.items():
            w = x.shape[3] if x.dim() == 4 else 1
            lay[name] = (off, w, x.dtype)
            off += w
        cap, L = kw["capacity"], max_seq_len
        z = lambda *s: torch.zeros(s, dtype=torch.int32)
        return torch.zeros(11, dtype=torch.int64), z(cap, L, 16), z(cap), z(cap), z(cap), z(cap, L), z(cap, L), None, lay


def test_train_batcher_with_max_seq_len():
    import torch
    import phantom_amd as ph
    from phantom_amd.rollout import DeviceBatch, DeviceSeqBatch
    tb = ph.TrainBatcher(_Env, seed=9, policy_mapping_fn=lambda aid: "x" if aid in "ace" else "y", max_seq_len=3)
    assert tb.max_seq_len == 3 and tb.calls == 0 and ph.TrainBatcher(_Env).max_seq_len is None
    dev = _Dev()
    for T in (3, 4, 5, 9):
        planes = {"obs": torch.zeros(T, 2, 5, 3), "advantages": torch.zeros(T, 2, 5), "terminateds": torch.ones(T, 2, 5, dtype=torch.uint8),
                  "truncateds": torch.zeros(T, 2, 5, dtype=torch.uint8)}
        before = tb.calls
        out = tb.collect(dev, planes, None)
        assert tb.calls == before + 1 and list(out) == ["x", "y"] and all(isinstance(b, DeviceSeqBatch) for b in out.values())
        asked = dev.asked[-2:]
        per_column = -(-T // 3) + (T - 1) // 4 + 1                # the length cuts, plus one per episode end inside the fragment
        assert [a["capacity"] for a in asked] == [2 * 3 * per_column, 2 * 2 * per_column]
        assert [a["class_id"] for a in asked] == [0, 1] and [a["epoch"] for a in asked] == [before, before] and all(a["seed"] == 9 for a in asked)
        assert all(a["max_seq_len"] == 3 and a["standardize"] == "advantages" and a["shuffle"] and a["lead_dims"] == 3 for a in asked)
        assert all(a["terminated"] is planes["terminateds"] and a["truncated"] is planes["truncateds"] and a["keep"] is None for a in asked)
        assert out["x"].epoch == before and out["x"].standardized == "advantages" and out["x"].layout["obs"] == (0, 3, torch.float32, (3,))
        assert tuple(out["y"].records.shape) == (2 * 2 * per_column, 3, 16)
    tb.collect(dev, {"rewards": torch.zeros(2, 2, 5)})                 # a fragment without flag planes: only the length cuts
    assert dev.asked[-1]["terminated"] is None and dev.asked[-1]["truncated"] is None and dev.asked[-1]["standardize"] is None
    with pytest.raises(ValueError, match="out of scope"):
        tb.reshuffle(out["x"])
    assert tb.calls == 5                                               # (a refused reshuffle draws no epoch)
    for bad in (0, -1, 65537, 2.5, True):
        with pytest.raises(ValueError, match="max_seq_len"):
            ph.TrainBatcher(_Env, max_seq_len=bad)
    assert DeviceBatch is ph.rollout.DeviceBatch and DeviceSeqBatch is ph.rollout.DeviceSeqBatch
