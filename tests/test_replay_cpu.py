"""CPU: the definition of phx_replay_add / phx_replay_sample (include/phantom_amd_replay.h) as tests/replay_ref.py restates it -- the
header's known answers, the draws' bounds and coverage, the ring against a record-by-record loop over add sequences that wrap; the
structs against the header as a C compiler lays them out, the symbols, no scratch in any kernel; ReplayBuffer's and sample()'s
argument errors that need no device."""
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
import replay_ref as rr
from helpers import supply_chain_env
from phantom_amd import _abi, build

KNOWN = {(0, 0): [338, 269, 271, 480, 597, 433, 92, 207], (0, 1): [522, 286, 949, 176, 367, 247, 151, 218],
         (1, 0): [432, 425, 539, 817, 168, 145, 763, 378], (2 ** 64 - 1, 2 ** 64 - 1): [730, 14, 3, 914, 472, 481, 675, 830]}


def test_known_answers():
    for (seed, draw), want in KNOWN.items():
        assert rr.draws(seed, draw, 1000, 8) == want, (seed, draw)
    assert rr.draws(7, 3, 2 ** 40 + 5, 4) == [643853115474, 346710636050, 830867739405, 867501151371]
    assert rr.draws(0, 0, 1000, 3, first=5) == KNOWN[0, 0][5:]
    assert rr.draws(5, 9, 0, 4) == [-1] * 4


@pytest.mark.parametrize("size", [1, 2, 7, 257, 2 ** 40 + 5])
def test_draws_stay_inside_the_ring(size):
    for seed, draw in ((0, 0), (1, 2), (2 ** 64 - 1, 2 ** 64 - 1), (0xDEADBEEF12345678, 41)):
        s = rr.draws(seed, draw, size, 1000)
        assert all(isinstance(x, int) and 0 <= x < size for x in s), (size, seed, draw)
        assert size == 1 or len(set(s)) > 1


def test_every_slot_is_drawn():
    counts = np.bincount(rr.draws(0, 0, 7, 1000), minlength=7)
    assert counts.sum() == 1000 and counts.min() == 125, counts     # (the definition's own figure: the rarest of 7 slots)
    for seed, draw in ((1, 0), (0, 1), (3, 99)):
        assert np.bincount(rr.draws(seed, draw, 7, 1000), minlength=7).min() > 0


def test_draw_numbers_give_different_streams():
    a = [tuple(rr.draws(9, d, 2 ** 40, 16)) for d in range(32)]
    assert len(set(a)) == 32
    same = sum(x == y for d in range(31) for x, y in zip(a[d], a[d + 1]))
    assert same == 0                                                # (a shared slot of 2^40 would be a collision of the hash)
    assert rr.draws(9, 0, 2 ** 40, 16) != rr.draws(10, 0, 2 ** 40, 16)


@pytest.mark.parametrize("C", [1, 2, 5, 257])
@pytest.mark.parametrize("row_words", [4, 12])
def test_the_ring_against_a_record_by_record_loop(C, row_words):
    rng = np.random.default_rng([C, row_words])
    cap = 3 * C + 2
    a, b = rr.Ring(C, row_words, fill=0xA5A5A5A5), rr.NaiveRing(C, row_words, fill=0xA5A5A5A5)
    counts = [0, 1, C - 1, C, C + 1, 3 * C + 2, cap + 1, -1, 1, C - 1, 2, C + 1, 0, 3 * C + 2, 1]      # (two refused: cap + 1 and -1)
    refused = 0
    for step, K in enumerate(counts):
        src = rng.integers(0, 2 ** 32, (cap, row_words), dtype=np.uint64).astype(np.uint32)
        before = a.ring.copy()
        a.add(src, K)
        b.add(src, K)
        refused += K < 0 or K > cap
        assert (a.cursor, a.size, a.total, a.refused) == (b.cursor, b.size, b.total, b.refused), (step, K)
        assert a.refused == refused and a.total == sum(k for k in counts[:step + 1] if 0 <= k <= cap)
        assert a.ring.tolist() == b.ring, (step, K)
        assert 0 <= a.cursor < C and a.size <= C and (a.size == C or a.cursor == a.size)      # the invariant: valid slots are [0, size)
        if K < 0 or K > cap:
            assert (a.ring == before).all()
        elif 0 < K:                                               # the ring holds the LAST min(K, C) records, in order, ending before the cursor
            m = min(K, C)
            assert (a.ring[(a.cursor - m + np.arange(m)) % C] == src[K - m:K]).all()
    assert a.state().tobytes() == np.array((a.cursor, a.size, a.total, a.refused), "<i8").tobytes()


def test_the_reference_sample_selects_before_it_reads():
    r = rr.Ring(5, 4)
    out, s = r.sample(3, seed=1)
    assert (s == -1).all() and (out == 0).all()                    # an empty ring
    r.add(np.arange(12, dtype=np.uint32).reshape(3, 4) + 1, 3)
    out, s = r.sample(6, slot_in=[0, 2, 3, -1, np.iinfo(np.int64).min, np.iinfo(np.int64).max])
    assert s.tolist() == [0, 2, -1, -1, -1, -1] and (out[:2] == r.ring[[0, 2]]).all() and (out[2:] == 0).all()
    out, s = r.sample(64, seed=3, draw=4)
    assert s.tolist() == rr.draws(3, 4, 3, 64) and (out == r.ring[s]).all()


def test_struct_symbols_and_header(tmp_path):
    structs = ((_abi.PhxReplayState, "phx_replay_state"), (_abi.PhxReplayAddIO, "phx_replay_add_io"), (_abi.PhxReplaySampleIO, "phx_replay_sample_io"))
    header = open(os.path.join(ROOT, "include", "phantom_amd_replay.h")).read()
    assert "int phx_replay_add(const phx_replay_add_io* io, void* stream);" in header
    assert "int phx_replay_sample(const phx_replay_sample_io* io, void* stream);" in header
    for struct, name in structs:
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
        names = re.findall(r"(\w+)(?:\[\w+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
        assert names == [n for n, _ in struct._fields_], names
    assert [ctypes.sizeof(s) for s, _ in structs] == [32, 80, 96]
    for text in ("} phx_replay_state;                 /* 32 bytes */", "} phx_replay_add_io;                /* 80 bytes */",
                 "} phx_replay_sample_io;             /* 96 bytes */"):
        assert text in header
    assert np.dtype(_abi.REPLAY_STATE_DTYPE) == rr.STATE_DTYPE and rr.STATE_DTYPE.itemsize == _abi.REPLAY_STATE_BYTES == 32
    for banned in ("phx_train_batch", "phx_seq_batch", "phx_traj"):  # the other headers' tests scan every header for their names
        assert banned not in header
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "phantom_amd_replay.h":
            assert "phx_replay" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert _abi.REPLAY_ADD_KERNELS == "phx_replay_add_kernel+phx_replay_commit_kernel" and _abi.REPLAY_ADD_KERNELS in header
    assert _abi.REPLAY_SAMPLE_KERNEL == "phx_replay_sample_kernel" and _abi.REPLAY_SAMPLE_KERNEL in header
    assert (_abi.REPLAY_ADD_KERNEL, _abi.REPLAY_COMMIT_KERNEL) == tuple(_abi.REPLAY_ADD_KERNELS.split("+"))
    assert "phx_replay.hip" in build.SOURCES and any(h.endswith("phantom_amd_replay.h") for h in build.HEADERS)
    lib = _abi.load_library()
    for fn in ("phx_replay_add", "phx_replay_sample"):
        assert hasattr(lib, fn) and fn not in _abi.EXPORTS
        assert getattr(lib, fn)(None, None) == -1 and fn.encode() in lib.phx_last_error()      # refused before any launch
    assert _abi.ABI_VERSION == 10
    # the sizes and offsets a C compiler gives the header's structs
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [(name, n) for s, name in structs for n, _ in s._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phantom_amd_replay.h"\nint main(void) {\n' +
                   '  printf("%zu %zu %zu\\n", sizeof(phx_replay_state), sizeof(phx_replay_add_io), sizeof(phx_replay_sample_io));\n' +
                   "".join(f'  printf("%zu\\n", offsetof({s}, {f}));\n' for s, f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out[:3]] == [32, 80, 96]
    assert [int(x) for x in out[3:]] == [getattr(s, n).offset for s, _ in structs for n, _ in s._fields_]


def test_no_kernel_uses_scratch(tmp_path):
    """every kernel of the file cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 (a spilled load buffer would
    put scratch traffic between the loads in flight and their stores) and leaves room for at least 2 waves per SIMD"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_replay.hip"), "-o", str(tmp_path / "rp.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    kernels = (_abi.REPLAY_ADD_KERNEL, _abi.REPLAY_COMMIT_KERNEL, _abi.REPLAY_SAMPLE_KERNEL)
    assert len(names) == len(set(names)) == len(scratch) == len(occupancy) == 3
    assert [sum(k in n for n in names) for k in kernels] == [1, 1, 1]
    assert scratch == [0] * 3, dict(zip(names, scratch))
    assert min(occupancy) >= 2, dict(zip(names, occupancy))
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert lds == [0] * 3, dict(zip(names, lds))                    # no LDS, as the header's issue asks


# ---- ReplayBuffer and sample(replay=...) on hand-made batches ---------------------------------------------------------------------
class _Dev:
    """stands in for DeviceEnv.replay_add / replay_sample: the restatement on host tensors, and a record of what it was asked for"""

    def __init__(self):
        self.asked, self.ref = [], None

    def replay_add(self, ring, state, records, count=None):
        import torch
        self.asked.append(("add", count))
        if self.ref is None:
            self.ref = rr.Ring(*ring.shape)
        K = records.shape[0] if count is None else int(count.item()) if hasattr(count, "item") else count
        self.ref.add(records.numpy().view(np.uint32), K)
        ring.copy_(torch.from_numpy(self.ref.ring.view(np.int32)))
        state.copy_(torch.from_numpy(np.frombuffer(self.ref.state().tobytes(), "<i8").copy()))

    def replay_sample(self, ring, state, n, seed=0, draw=0, slots=None, out=None):
        import torch
        self.asked.append(("sample", n, seed, draw, slots is not None))
        out, s = self.ref.sample(n, seed, draw, None if slots is None else slots.numpy())
        return torch.from_numpy(out.view(np.int32)), torch.from_numpy(s)


def _batch(dev, K, cap, seed, known=True, words=8):
    import torch
    from phantom_amd.rollout import DeviceBatch
    rng = np.random.default_rng(seed)
    layout = {"obs": (0, 3, torch.float32, (3,)), "rewards": (3, 1, torch.float32, ()), "terminateds": (4, 1, torch.uint8, ())}
    rec = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (cap, words)).astype(np.int32))
    rec[:, 4] = torch.from_numpy(rng.integers(0, 2, cap).astype(np.int32))
    start = torch.tensor([0, K], dtype=torch.int64)
    return DeviceBatch(rec, layout, start, count=K if known else None, dev=dev)


def test_replay_buffer_on_hand_made_batches():
    import torch
    import phantom_amd as ph
    from phantom_amd.rollout import DeviceBatch, DeviceSeqBatch
    dev = _Dev()
    rb = ph.ReplayBuffer(None, 10, seed=6)
    assert len(rb) == 0 and rb.total == 0 and rb.refused == 0 and rb.ring is None and rb.draws == 0
    with pytest.raises(ValueError, match="nothing was ever added"):
        rb.sample(4)
    with pytest.raises(ValueError, match="nothing was ever added"):
        rb.gather(torch.zeros(2, dtype=torch.int64))
    b1 = _batch(dev, 7, 7, 1)
    rb.add(b1)
    assert dev.asked[-1] == ("add", 7) and tuple(rb.ring.shape) == (10, 8) and rb.ring.dtype == torch.int32 and rb.layout == b1.layout
    assert tuple(rb.state.shape) == (4,) and rb.state.dtype == torch.int64
    assert (len(rb), rb.total, rb.refused) == (7, 7, 0)
    b2 = _batch(dev, 5, 9, 2, known=False)                          # the host does not know the count: it goes as a device tensor
    rb.add(b2)
    kind, count = dev.asked[-1]
    assert kind == "add" and count.data_ptr() == b2.start.data_ptr() + 8 and tuple(count.shape) == (1,) and b2._count is None
    assert (len(rb), rb.total, rb.refused) == (10, 12, 0)
    want = np.concatenate([b1.records.numpy(), b2.records.numpy()[:5]])[2:]
    assert (rb.ring.numpy()[(2 + np.arange(10)) % 10] == want).all()
    over = _batch(dev, 12, 9, 3, known=False)                       # a batch whose count exceeded its buffer holds no records
    rb.add(over)
    assert (len(rb), rb.total, rb.refused) == (10, 12, 1)
    for d in range(3):
        mb = rb.sample(64)
        assert dev.asked[-1] == ("sample", 64, 6, d, False) and rb.draws == d + 1
        assert isinstance(mb, DeviceBatch) and mb.count == 64 == len(mb) and mb.epoch == d and mb.row is None and mb.col is None
        assert mb.layout == rb.layout and mb.slots.tolist() == rr.draws(6, d, 10, 64)
        cols = mb.columns
        assert cols["obs"].dtype == torch.float32 and tuple(cols["obs"].shape) == (64, 3) and cols["terminateds"].dtype == torch.bool
        assert (mb.records.numpy() == rb.ring.numpy()[mb.slots.numpy()]).all()
    g = rb.gather(torch.tensor([9, 0, 10, -1, 3], dtype=torch.int64))
    assert g.slots.tolist() == [9, 0, -1, -1, 3] and g.epoch == 3 and rb.draws == 4 and g.count == 5
    assert (g.records.numpy()[[0, 1, 4]] == rb.ring.numpy()[[9, 0, 3]]).all() and (g.records.numpy()[[2, 3]] == 0).all()
    with pytest.raises(ValueError, match="layout"):
        rb.add(_batch(dev, 3, 3, 4, words=12))
    other = _batch(dev, 3, 3, 4)
    other.layout["rewards"] = (5, 1, torch.float32, ())
    with pytest.raises(ValueError, match="layout"):
        rb.add(other)
    seq = DeviceSeqBatch(torch.zeros((2, 3, 8), dtype=torch.int32), b1.layout, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    for bad, match in ((seq, "DeviceSeqBatch"), ({"obs": 1}, "DeviceBatch"), (None, "DeviceBatch")):
        with pytest.raises(ValueError, match=match):
            rb.add(bad)
    with pytest.raises(ValueError, match="slots"):
        rb.gather([1, 2])
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="capacity"):
            ph.ReplayBuffer(None, bad)
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            ph.ReplayBuffer(None, 4, seed=bad)
    assert (len(rb), rb.total, rb.refused) == (10, 12, 1)           # the refusals above changed nothing


def test_sample_checks_replay_before_anything_runs():
    import phantom_amd as ph
    env = supply_chain_env(3, [2] * 3, 6, 4, seed=1, exogenous="device")
    ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
    one, two = ph.TrainBatcher(env), ph.TrainBatcher(env, policy_mapping_fn=lambda aid: "a" if aid == ids[0] else "b")
    seq = ph.TrainBatcher(env, max_seq_len=4)
    rb = ph.ReplayBuffer(env, 16)
    for kw, match in ((dict(replay=rb), "needs `batcher`"), (dict(replay=rb, batcher=seq), "max_seq_len"), (dict(replay=rb, batcher=two), "policy ids"),
                      (dict(replay={"a": rb}, batcher=two), "policy ids"), (dict(replay={"a": rb, "b": rb, "c": rb}, batcher=two), "policy ids"),
                      (dict(replay={"a": rb, "b": 3}, batcher=two), "policy ids"), (dict(replay=[rb], batcher=one), "policy ids"),
                      (dict(replay={"other": rb}, batcher=one), "policy ids")):
        with pytest.raises(ValueError, match=match):
            env.sample(4, n_step=3, **kw)
        with pytest.raises(ValueError, match=match):
            ph.rllib.BatchedBaseEnv(env).sample(4, n_step=3, **kw)
    assert one.calls == two.calls == seq.calls == 0 and rb.ring is None
