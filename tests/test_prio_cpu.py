"""CPU: the definition of phx_prio_add / phx_prio_update / phx_prio_sample (include/phantom_amd_prio.h) as tests/prio_ref.py restates it
-- the header's known answers, the array restatement against the node-by-node one over add sequences that wrap and updates with
duplicates, unusable priorities and slots outside the ring, the draws' guarantees (the "no k" fallback included) and their
proportionality; the structs against the header as a C compiler lays them out, the symbols, the naming rule between the headers, no
scratch in any kernel; FragmentOps.prio_*'s refusals in front of a stand-in library and PrioritizedReplayBuffer on a stand-in device."""
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
import prio_ref as pr
import replay_ref as rr
from phantom_amd import _abi, build

RINGS = (1, 15, 16, 17, 255, 257)
I64_MIN, I64_MAX = pr.I64_MIN, pr.I64_MAX
BAD_PRIORITIES, KNOWN, FALLBACK_DRAWS = pr.BAD_PRIORITIES, pr.KNOWN, pr.FALLBACK_DRAWS      # (shared with the GPU tests)
ADD_COUNTS = lambda C: [0, 1, C - 1, C, C + 1, 3 * C + 2, 3 * C + 3, -1, 1, C - 1, 2, C + 1, 0, 3 * C + 2, 1]      # (two refused: beyond src, -1)


def known_tree(cls=pr.Tree):
    t = cls(37)
    t.add(37, 37, 0)
    t.update(list(range(37)), [1 + s % 7 for s in range(37)], 37)
    return t


def fallback_tree(cls=pr.Tree):
    t = cls(32)
    t.add(32, 32, 0)
    t.update(list(range(32)), [3.0] + [0.0] * 15 + [2.0 ** 24 + 4] + [0.0] * 15, 32)      # (0 is sanitized to 2^-40)
    return t


def same(a, b, what):
    assert a.buf.tobytes() == b.buf.tobytes(), what
    assert a.state().tobytes() == b.state().tobytes(), what


def check_invariant(t):
    """the header's invariant, read straight off the buffer (and the padding is zero)"""
    b = t.buf
    for l in range(0, t.L + 1):
        w = 16 if l == t.L else t.off[l + 1] - t.off[l]
        assert (b[t.off[l] + t.n[l]:t.off[l] + w] == 0).all()
        if l >= 1:
            assert (b[t.moff(l) + t.n[l]:t.moff(l) + w] == 0).all()
            for j in range(t.n[l]):
                c = b[t.off[l - 1] + 16 * j:t.off[l - 1] + 16 * j + 16]
                s = c[0]
                for k in range(1, 16):
                    s = np.float32(s + c[k])
                assert b[t.off[l] + j] == s
                m = c if l == 1 else b[t.moff(l - 1) + 16 * j:t.moff(l - 1) + 16 * j + 16]
                assert b[t.moff(l) + j] == (m[m != 0].min() if (m != 0).any() else 0)


def test_known_answers():
    a, b = known_tree(), known_tree(pr.NaiveTree)
    same(a, b, "the known tree")
    assert a.total() == 143 and a.pmin() == 1 and a.maxp() == 7
    for (seed, draw), (slots, prios) in KNOWN.items():
        for t in (a, b):
            s, p = t.sample(8, seed, draw, 37)
            assert s.tolist() == slots and p.tolist() == prios and p.dtype == np.float32 and s.dtype == np.int64, (seed, draw)
    assert a.sample(4, 5, 9, 0)[0].tolist() == [-1] * 4 and pr.Tree(37).sample(4, 5, 9, 37)[1].tobytes() == bytes(16)
    s0 = rr.mix(rr.mix((3 + rr.G) & rr.M64) ^ 4)
    assert pr.uniforms(3, 4, 5).tolist() == [(rr.mix((s0 + (i + 1) * rr.G) & rr.M64) >> 40) / 2 ** 24 for i in range(5)]
    assert pr.san(float("nan")) == pr.san(0) == pr.san(-1) == pr.san(2.0 ** -50) == pr.PRIO_MIN == 2.0 ** -40
    assert pr.san(float("inf")) == pr.san(2.0 ** 50) == pr.PRIO_MAX == 2.0 ** 40 and pr.san(0.5) == 0.5


@pytest.mark.parametrize("C", RINGS)
def test_the_array_restatement_against_node_by_node(C):
    rng = np.random.default_rng(C)
    a, b, ring = pr.Tree(C), pr.NaiveTree(C), rr.Ring(C, 4)
    cap, refused, ignored = 3 * C + 2, 0, 0
    src = np.zeros((cap, 4), np.uint32)
    for step, K in enumerate(ADD_COUNTS(C)):
        for t in (a, b):
            t.add(K, cap, ring.cursor)
        before = ring.size
        ring.add(src, K)                                           # the ring's own add comes second
        refused += K < 0 or K > cap
        same(a, b, f"C={C} add {step} (K={K})")
        assert a.refused == refused == ring.refused
        check_invariant(a)
        held = a.buf[:C] > 0
        assert held[:ring.size].all() and not held[ring.size:].any()      # exactly the slots the ring holds have a priority
        if 0 <= K <= cap:
            assert ring.size == min(C, before + K)
        # an update: duplicates, unusable priorities, slots outside [0, size)
        n = int(rng.integers(1, 2 * C + 8))
        slots = rng.integers(-2, C + 2, n).tolist() + [-1, ring.size, I64_MIN, I64_MAX] + [0] * 3
        prios = (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32).tolist() + [1.0] * 4 + [0.25, 9.0, 0.5]
        for i, bad in enumerate(BAD_PRIORITIES):
            if i < n:
                prios[i] = bad
        for t in (a, b):
            t.update(slots, prios, ring.size)
        ignored += sum(not 0 <= s < ring.size for s in slots)
        same(a, b, f"C={C} update {step}")
        assert a.ignored == ignored
        check_invariant(a)
        if ring.size:
            assert a.buf[0] == max(pr.san(p) for s, p in zip(slots, prios) if s == 0) >= 9.0      # the duplicates' maximum, not the last
            assert (a.buf[:ring.size] >= pr.PRIO_MIN).all() and (a.buf[:ring.size] <= pr.PRIO_MAX).all()
            assert a.maxp() >= max(9.0, a.buf[:C].max()) and np.isfinite(a.total()) and a.pmin() == a.buf[:ring.size].min()
        s1, p1 = a.sample(33, C, step, ring.size)
        s2, p2 = b.sample(33, C, step, ring.size)
        assert (s1 == s2).all() and p1.tobytes() == p2.tobytes()
        if ring.size:
            assert ((s1 >= 0) & (s1 < ring.size)).all() and (p1 > 0).all() and (p1 == a.buf[s1]).all()
        else:
            assert (s1 == -1).all() and (p1 == 0).all()
    # slot lists that name nothing, and one slot many times
    for t in (a, b):
        t.update([-1, C, I64_MIN, I64_MAX], [1.0] * 4, C)
        t.update([C - 1] * 70, list(np.linspace(0.5, 4.0, 70, dtype=np.float32)), C)
    same(a, b, f"C={C} all-invalid and all-duplicate updates")
    assert a.buf[C - 1] == 4.0


def test_every_draw_lands_on_a_held_slot_with_a_priority():
    for C, size, leaves in ((300, 300, {299: 0.5}), (300, 7, {6: 2.0 ** -40}), (17, 17, {16: 2.0 ** 40}), (1, 1, {0: 3.0})):
        for cls in (pr.Tree, pr.NaiveTree):
            t = cls(C)
            for s, p in leaves.items():                            # one non-zero leaf, in the last slot: written directly, then rebuilt
                t.buf[s] = np.float32(p)
            t.rebuild()
            s, p = t.sample(200, 1, 2, size)
            assert (s == max(leaves)).all() and (p == np.float32(leaves[max(leaves)])).all(), (C, size)
    t = pr.Tree(300)
    t.buf[299] = 1
    t.rebuild()
    assert (t.sample(8, 0, 0, 299)[0] == -1).all()                  # a leaf outside [0, size): a state the calls do not produce


def test_the_no_k_fallback_is_taken_and_still_lands_on_a_priority():
    a, b = fallback_tree(), fallback_tree(pr.NaiveTree)
    same(a, b, "the fallback tree")
    assert a.buf[a.off[1]] == 3 and a.buf[a.off[1] + 1] == 2.0 ** 24 + 4 and a.total() == 2.0 ** 24 + 8
    for seed, draw in FALLBACK_DRAWS:
        fb = []
        s, p = b.sample(4, seed, draw, 32, fallbacks=fb)
        assert (0, 1) in fb, (seed, draw)                          # draw 0 found no k at level 1
        assert s[0] == 31 and p[0] == pr.PRIO_MIN
        s2, p2 = a.sample(4, seed, draw, 32)
        assert (s == s2).all() and p.tobytes() == p2.tobytes() and ((s >= 0) & (s < 32)).all() and (p > 0).all()


def test_draws_are_proportional_to_priority():
    """7 000 draws of the stream (0, 0) over priorities 1 .. 7: the restatement's counts, pinned, each within 4 binomial standard
    deviations of 7 000 p / 28"""
    t = pr.Tree(7)
    t.add(7, 7, 0)
    t.update(list(range(7)), [1, 2, 3, 4, 5, 6, 7], 7)
    s, p = t.sample(7000, 0, 0, 7)
    counts = np.bincount(s, minlength=7)
    assert counts.tolist() == [247, 501, 745, 1002, 1294, 1481, 1730]
    q = np.arange(1, 8) / 28
    assert (np.abs(counts - 7000 * q) <= 4 * np.sqrt(7000 * q * (1 - q))).all()
    assert (p == s + 1).all()


def test_layout():
    for C, want in ((1, (0, (0,), 16, 16)), (2, (1, (0, 16), 32, 48)), (16, (1, (0, 16), 32, 48)), (17, (2, (0, 32, 48), 64, 96)),
                    (256, (2, (0, 256, 272), 288, 320)), (257, (3, (0, 272, 304, 320), 336, 400)), (4096, (3, (0, 4096, 4352, 4368), 4384, 4672)),
                    (4097, (4, (0, 4112, 4384, 4416, 4432), 4448, 4784))):
        assert _abi.prio_layout(C) == want, C
        L, n, off, W, words = pr.layout(C)
        assert (L, tuple(off), W, words) == want
        assert _abi.prio_min_root(C) == pr.Tree(C).pmin_index()
    assert _abi.prio_layout(2 ** 30)[0] == 8 and _abi.prio_layout(2 ** 24)[0] == 6 and _abi.prio_layout(2 ** 20 + 1)[0] == 6
    for bad in (0, -1, 2 ** 30 + 1, 2.0, True, None):
        with pytest.raises(ValueError, match="capacity"):
            _abi.prio_layout(bad)
    assert _abi.prio_kernels(_abi.PRIO_ADD_KERNELS, 4096) == "phx_prio_fill_kernel+phx_prio_top_kernel"
    assert _abi.prio_kernels(_abi.PRIO_ADD_KERNELS, 4097) == _abi.PRIO_ADD_KERNELS
    assert _abi.prio_kernels(_abi.PRIO_UPDATE_KERNELS, 1) == "phx_prio_zero_kernel+phx_prio_raise_kernel+phx_prio_top_kernel"


STRUCTS = ((_abi.PhxPrioState, "phx_prio_state", 32), (_abi.PhxPrioAddIO, "phx_prio_add_io", 72), (_abi.PhxPrioUpdateIO, "phx_prio_update_io", 72),
           (_abi.PhxPrioSampleIO, "phx_prio_sample_io", 80))
OTHERS = ("phx_replay", "phx_train_batch", "phx_seq_batch", "phx_traj", "phx_nstep", "phx_episode", "phx_vtrace", "phx_gae")


def test_struct_symbols_and_header(tmp_path):
    header = open(os.path.join(ROOT, "include", "phantom_amd_prio.h")).read()
    for fn in ("add", "update", "sample"):
        assert f"int phx_prio_{fn}(const phx_prio_{fn}_io* io, void* stream);" in header
    for struct, name, size in STRUCTS:
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
        names = re.findall(r"(\w+)(?:\[\w+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
        assert names == [n for n, _ in struct._fields_], names
        assert ctypes.sizeof(struct) == size and re.search(rf"\}} {name};\s+/\* {size} bytes \*/", header)
    assert np.dtype(_abi.PRIO_STATE_DTYPE) == pr.STATE_DTYPE and pr.STATE_DTYPE.itemsize == _abi.PRIO_STATE_BYTES == 32
    assert _abi.PRIO_FANOUT == pr.FANOUT == 16 and "#define PHX_PRIO_FANOUT 16" in header
    assert "#define PHX_PRIO_MIN 0x1p-40f" in header and "#define PHX_PRIO_MAX 0x1p+40f" in header
    # the naming rule, in both directions: every header's test scans all of include/ for its own identifiers
    for banned in OTHERS:
        assert banned not in header, banned
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "phantom_amd_prio.h":
            assert "phx_prio" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert "phantom_amd_prio.h" in open(os.path.join(ROOT, "include", "phantom_amd_replay.h")).read()
    # the kernels' names, the known answers and the draw's constants as the header states them
    assert _abi.PRIO_ADD_KERNELS == "phx_prio_fill_kernel+phx_prio_span_kernel+phx_prio_top_kernel" and f'"{_abi.PRIO_ADD_KERNELS}"' in header
    assert _abi.PRIO_UPDATE_KERNELS == "phx_prio_zero_kernel+phx_prio_raise_kernel+phx_prio_path_kernel+phx_prio_top_kernel"
    assert f'"{_abi.PRIO_UPDATE_KERNELS}"' in header and f'"{_abi.PRIO_SAMPLE_KERNEL}"' in header
    assert (_abi.PRIO_FILL_KERNEL, _abi.PRIO_SPAN_KERNEL, _abi.PRIO_TOP_KERNEL) == tuple(_abi.PRIO_ADD_KERNELS.split("+"))
    assert (_abi.PRIO_ZERO_KERNEL, _abi.PRIO_RAISE_KERNEL, _abi.PRIO_PATH_KERNEL, _abi.PRIO_TOP_KERNEL) == tuple(_abi.PRIO_UPDATE_KERNELS.split("+"))
    for slots, prios in KNOWN.values():
        assert re.search(r"slots\s+" + r"\s+".join(map(str, slots)) + r",\s+priorities\s+" + r"\s+".join(map(str, prios)) + r"\n", header)
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert const in header
    assert "phx_prio.hip" in build.SOURCES and any(h.endswith("phantom_amd_prio.h") for h in build.HEADERS)
    assert set(_abi.PRIORITY_OPS) == {"phx_prio_add", "phx_prio_update", "phx_prio_sample"} and not set(_abi.PRIORITY_OPS) & set(_abi.FRAGMENT_OPS)
    assert [io for io in _abi.PRIORITY_OPS.values()] == [_abi.PhxPrioAddIO, _abi.PhxPrioUpdateIO, _abi.PhxPrioSampleIO]
    lib = _abi.load_library()
    for fn in _abi.PRIORITY_OPS:
        assert hasattr(lib, fn) and fn not in _abi.EXPORTS
        assert getattr(lib, fn)(None, None) == -1 and fn.encode() in lib.phx_last_error()      # refused before any launch
        assert getattr(lib, fn).restype is ctypes.c_int32 and getattr(lib, fn).argtypes[0] is ctypes.POINTER(_abi.PRIORITY_OPS[fn])
    assert _abi.ABI_VERSION == 10 and lib.phx_abi_version() == 10
    # the sizes and offsets a C compiler gives the header's structs
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [(name, n) for s, name, _ in STRUCTS for n, _ in s._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phantom_amd_prio.h"\nint main(void) {\n' +
                   "".join(f'  printf("%zu\\n", sizeof({name}));\n' for _, name, _ in STRUCTS) +
                   "".join(f'  printf("%zu\\n", offsetof({s}, {f}));\n' for s, f in fields) +
                   '  printf("%d %a %a\\n", PHX_PRIO_FANOUT, (double)PHX_PRIO_MIN, (double)PHX_PRIO_MAX);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out[:4]] == [32, 72, 72, 80]
    assert [int(x) for x in out[4:-3]] == [getattr(s, n).offset for s, _, _ in STRUCTS for n, _ in s._fields_]
    assert int(out[-3]) == 16 and float.fromhex(out[-2]) == 2.0 ** -40 and float.fromhex(out[-1]) == 2.0 ** 40


def test_no_kernel_uses_scratch(tmp_path):
    """every kernel of the file cross-compiled for gfx950 with the build's own flags reports ScratchSize 0 (a node's 16 children and
    their chain stay in registers) and leaves room for at least 2 waves per SIMD; none uses LDS"""
    try:
        cc = build.hipcc()
        subprocess.run([cc, "--version"], check=True, capture_output=True)
    except (RuntimeError, OSError, subprocess.CalledProcessError):
        pytest.skip("no hipcc")
    flags = [f for f in build.FLAGS if f != "-shared" and not f.startswith("--offload-arch")]
    r = subprocess.run([cc, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, "phx_prio.hip"), "-o", str(tmp_path / "pr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    kernels = sorted(set((_abi.PRIO_ADD_KERNELS + "+" + _abi.PRIO_UPDATE_KERNELS + "+" + _abi.PRIO_SAMPLE_KERNEL).split("+")))
    assert len(kernels) == 7 and len(names) == len(set(names)) == len(scratch) == len(occupancy) == len(lds) == 7
    assert [sum(k in n for n in names) for k in kernels] == [1] * 7
    assert scratch == [0] * 7, dict(zip(names, scratch))
    assert min(occupancy) >= 2, dict(zip(names, occupancy))
    assert lds == [0] * 7, dict(zip(names, lds))


# ---- FragmentOps.prio_*: every refusal comes before any call into the library ------------------------------------------------------
class RecordingLib:
    """every entry point records ``(name, a copy of the io struct)`` and returns 0"""

    def __init__(self):
        self.calls = []

    def phx_last_error(self):
        return b"stand-in"

    def __getattr__(self, entry):
        def call(io_ref, stream):
            io = io_ref._obj
            self.calls.append((entry, type(io).from_buffer_copy(io)))
            return 0
        return call


def make_ops():
    import torch
    from phantom_amd.fragment_ops import FragmentOps

    class Ops(FragmentOps):
        def _launch(self, entry, io):      # the seam: no torch.cuda.device guard, no stream
            self._check(getattr(self.lib, entry)(ctypes.byref(io), None), entry)
    return Ops(RecordingLib(), torch.device("cpu"))


def misaligned(x):
    """``x``'s shape and dtype in a view that starts 4 bytes (8 for 8-byte elements) behind a 16-byte boundary"""
    import torch
    nbytes, off = x.numel() * x.element_size(), max(4, x.element_size())
    raw = torch.zeros(nbytes + 32, dtype=torch.uint8)
    off += -raw.data_ptr() % 16
    return raw[off:off + nbytes].view(x.dtype).view(x.shape)


def test_fragment_ops_prio_calls_fill_their_structs_and_refuse_before_the_library():
    import torch
    from phantom_amd.device import DeviceEnv
    from phantom_amd.fragment_ops import FragmentOps
    f32, i64, u8 = torch.float32, torch.int64, torch.uint8
    Cn, n = 300, 5
    words = _abi.prio_layout(Cn)[3]
    ops = make_ops()
    tree, pstate, rstate = torch.zeros(words, dtype=f32), torch.zeros(32, dtype=u8), torch.zeros(4, dtype=i64)
    slots, prios, count = torch.zeros(n, dtype=i64), torch.ones(n, dtype=f32), torch.zeros(1, dtype=i64)
    oslot, oprio = torch.zeros(n, dtype=i64), torch.zeros(n, dtype=f32)
    for x in (tree, pstate, oslot, oprio):
        assert x.data_ptr() % 16 == 0
    base = dict(tree=tree, pstate=pstate, ring_state=rstate, capacity=Cn)
    good = {"prio_add": dict(base, src_capacity=9, count=count), "prio_update": dict(base, slots=slots, priorities=prios),
            "prio_sample": dict(base, n=n, seed=7, draw=2 ** 64 - 1, out=(oslot, oprio))}
    # good calls: which pointer and scalar lands where
    ops.prio_add(**good["prio_add"])
    ops.prio_add(**dict(good["prio_add"], count=4))
    ops.prio_add(**dict(good["prio_add"], count=None))
    ops.prio_update(**good["prio_update"])
    res = ops.prio_sample(**good["prio_sample"])
    assert res[0] is oslot and res[1] is oprio
    made = ops.prio_sample(**dict(good["prio_sample"], out=None))
    assert made[0].dtype == i64 and made[1].dtype == f32 and tuple(made[0].shape) == tuple(made[1].shape) == (n,)
    (e0, a0), (e1, a1), (e2, a2), (e3, up), (e4, sa), _ = ops.lib.calls
    assert (e0, e1, e2, e3, e4) == ("phx_prio_add",) * 3 + ("phx_prio_update", "phx_prio_sample")
    for io in (a0, a1, a2, up):
        assert (io.capacity, io.ring_state, io.tree, io.state) == (Cn, rstate.data_ptr(), tree.data_ptr(), pstate.data_ptr()) and list(io.reserved) == [0, 0]
    assert (a0.src_capacity, a0.count, a0.count_ptr) == (9, 0, count.data_ptr())
    assert (a1.src_capacity, a1.count, a1.count_ptr) == (9, 4, None) and (a2.count, a2.count_ptr) == (9, None)
    assert (up.n, up.slot_in, up.priority) == (n, slots.data_ptr(), prios.data_ptr())
    assert (sa.capacity, sa.n, sa.seed, sa.draw, sa.ring_state, sa.tree, sa.out_slot, sa.out_priority) == (
        Cn, n, 7, 2 ** 64 - 1, rstate.data_ptr(), tree.data_ptr(), oslot.data_ptr(), oprio.data_ptr()) and list(sa.reserved) == [0, 0]
    ops.lib.calls.clear()
    # refusals
    shared = [("tree", dict(tree=tree[:-1])), ("tree", dict(tree=tree.double())), ("tree", dict(tree=None)), ("tree", dict(tree=torch.zeros(words + 16, dtype=f32))),
              ("tree", dict(tree=misaligned(tree))), ("tree", dict(capacity=Cn + 16)), ("pstate", dict(pstate=pstate[:31])), ("pstate", dict(pstate=rstate)),
              ("pstate", dict(pstate=None)), ("pstate", dict(pstate=misaligned(pstate))), ("ring_state", dict(ring_state=rstate[:3])),
              ("ring_state", dict(ring_state=rstate.int())), ("ring_state", dict(ring_state=None)), ("capacity", dict(capacity=0)),
              ("capacity", dict(capacity=2 ** 30 + 1)), ("capacity", dict(capacity=2.0)), ("capacity", dict(capacity=True))]
    own = {"prio_add": [("src_capacity", dict(src_capacity=-1)), ("src_capacity", dict(src_capacity=1.5)), ("count", dict(count=10)), ("count", dict(count=-1)),
                        ("count", dict(count=True)), ("count", dict(count=2.0)), ("count", dict(count=torch.zeros(2, dtype=i64))),
                        ("count", dict(count=count.int()))],
           "prio_update": [("slots", dict(slots=None)), ("slots", dict(slots=slots.int())), ("slots", dict(slots=slots[:0])), ("slots", dict(slots=slots.reshape(1, n))),
                           ("priorities", dict(priorities=prios[:4])), ("priorities", dict(priorities=prios.double())), ("priorities", dict(priorities=None))],
           "prio_sample": [(r"n = ", dict(n=0)), (r"n = ", dict(n=2.5)), (r"n = ", dict(n=True)), ("seed", dict(seed=-1)), ("draw", dict(draw=2 ** 64)),
                           (r"out\[0\]", dict(out=(oslot[:4], oprio))), (r"out\[0\]", dict(out=(oslot.int(), oprio))), (r"out\[1\]", dict(out=(oslot, oprio.double()))),
                           (r"out\[1\]", dict(out=(oslot, None))), (r"out\[1\]", dict(out=(oslot, misaligned(oprio)))), ("out", dict(out=(oslot,)))]}
    for fn, kw in good.items():
        for match, patch in shared + own[fn]:
            with pytest.raises(ValueError, match=match):
                getattr(ops, fn)(**dict(kw, **patch))
    assert ops.lib.calls == []
    for fn in good:                                               # DeviceEnv inherits them
        assert getattr(DeviceEnv, fn) is getattr(FragmentOps, fn)


# ---- PrioritizedReplayBuffer on hand-made batches ---------------------------------------------------------------------------------
class _Dev:
    """stands in for DeviceEnv.replay_* / prio_*: the restatements on host tensors, and a record of what it was asked for"""

    def __init__(self):
        self.asked, self.ring, self.tree = [], None, None

    def _size(self, state):
        return int(state[1])

    def prio_add(self, tree, pstate, ring_state, capacity, src_capacity, count=None):
        import torch
        self.asked.append(("prio_add", capacity, src_capacity, count))
        if self.tree is None:
            self.tree = pr.Tree(capacity)
        K = src_capacity if count is None else int(count.item()) if hasattr(count, "item") else count
        self.tree.add(K, src_capacity, int(ring_state[0]))
        self._store(tree, pstate)

    def _store(self, tree, pstate):
        import torch
        tree.copy_(torch.from_numpy(self.tree.buf))
        pstate.copy_(torch.from_numpy(np.frombuffer(self.tree.state().tobytes(), np.uint8).copy()))

    def prio_update(self, tree, pstate, ring_state, capacity, slots, priorities):
        self.asked.append(("prio_update", slots.tolist(), priorities.clone()))
        assert priorities.dtype.is_floating_point and priorities.element_size() == 4
        self.tree.update(slots.tolist(), priorities.numpy(), self._size(ring_state))
        self._store(tree, pstate)

    def prio_sample(self, tree, pstate, ring_state, capacity, n, seed=0, draw=0, out=None):
        import torch
        self.asked.append(("prio_sample", n, seed, draw))
        s, p = self.tree.sample(n, seed, draw, self._size(ring_state))
        return torch.from_numpy(s), torch.from_numpy(p)

    def replay_add(self, ring, state, records, count=None):
        import torch
        self.asked.append(("replay_add", count))
        if self.ring is None:
            self.ring = rr.Ring(*ring.shape)
        K = records.shape[0] if count is None else int(count.item()) if hasattr(count, "item") else count
        self.ring.add(records.numpy().view(np.uint32), K)
        ring.copy_(torch.from_numpy(self.ring.ring.view(np.int32)))
        state.copy_(torch.from_numpy(np.frombuffer(self.ring.state().tobytes(), "<i8").copy()))

    def replay_sample(self, ring, state, n, seed=0, draw=0, slots=None, out=None):
        import torch
        self.asked.append(("replay_sample", n, slots is not None))
        out, s = self.ring.sample(n, seed, draw, None if slots is None else slots.numpy())
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


def test_prioritized_replay_buffer_on_hand_made_batches():
    import torch
    import phantom_amd as ph
    from phantom_amd.replay import check_replay
    from phantom_amd.rollout import DeviceBatch
    dev = _Dev()
    prb = ph.PrioritizedReplayBuffer(None, 20, alpha=0.5, eps=0.25, seed=6)
    assert isinstance(prb, ph.ReplayBuffer) and ph.PrioritizedReplayBuffer is ph.replay.PrioritizedReplayBuffer
    assert (len(prb), prb.total, prb.refused, prb.ignored, prb.tree, prb.pstate) == (0, 0, 0, 0, None, None)
    assert (prb.alpha, prb.eps, prb.seed) == (0.5, 0.25, 6)
    d = ph.PrioritizedReplayBuffer(None, 4)
    assert (d.alpha, d.eps, d.seed) == (0.6, 1e-6, 0)
    with pytest.raises(ValueError, match="nothing was ever added"):
        prb.sample(4)
    with pytest.raises(ValueError, match="nothing was ever added"):
        prb.update_priorities(torch.zeros(2, dtype=torch.int64), torch.ones(2))
    b1 = _batch(dev, 7, 9, 1)
    prb.add(b1)
    assert [a[0] for a in dev.asked] == ["prio_add", "replay_add"]                  # the tree's call first: it reads the ring's state as it was
    assert dev.asked[0] == ("prio_add", 20, 9, 7) and dev.asked[1] == ("replay_add", 7)
    assert tuple(prb.tree.shape) == (_abi.prio_layout(20)[3],) and prb.tree.dtype == torch.float32
    assert tuple(prb.pstate.shape) == (32,) and prb.pstate.dtype == torch.uint8 and tuple(prb.ring.shape) == (20, 8)
    assert (prb.tree[:7] == 1).all() and (prb.tree[7:32] == 0).all() and (len(prb), prb.total) == (7, 7)
    b2 = _batch(dev, 5, 9, 2, known=False)                          # the host does not know the count: both calls get the device tensor
    prb.add(b2)
    (k1, c1, s1, count1), (k2, count2) = dev.asked[-2:]
    assert (k1, c1, s1, k2) == ("prio_add", 20, 9, "replay_add") and count1 is count2 and count1.data_ptr() == b2.start.data_ptr() + 8
    assert (len(prb), prb.total, prb.refused) == (12, 12, 0) and (prb.tree[:12] == 1).all() and (prb.tree[12:32] == 0).all()
    over = _batch(dev, 12, 9, 3, known=False)                       # a batch whose count exceeded its buffer: refused by both
    prb.add(over)
    assert (len(prb), prb.total, prb.refused) == (12, 12, 1) and dev.tree.refused == 1
    # update_priorities applies eps and alpha
    slots = torch.tensor([0, 3, 3, 11, 12, -1], dtype=torch.int64)
    td = torch.tensor([3.75, 0.0, 8.75, 0.56, 1.0, 1.0], dtype=torch.float32)
    prb.update_priorities(slots, td)
    kind, got_slots, got_p = dev.asked[-1]
    assert kind == "prio_update" and got_slots == slots.tolist() and got_p.dtype == torch.float32
    np.testing.assert_allclose(got_p.numpy(), (td.numpy().astype(np.float64) + 0.25) ** 0.5, rtol=1e-6)
    assert prb.ignored == 2 and prb.tree[0] == 2.0 and prb.tree[3] == 3.0 and abs(float(prb.tree[11]) - 0.9) < 1e-6 and prb.tree[12] == 0
    with pytest.raises(ValueError, match="priorities"):
        prb.update_priorities(slots, None)
    # sample: the fields, and the weights against f64 numpy
    for d_, beta in enumerate((0.4, 1.0, 0.0)):
        mb = prb.sample(64, beta=beta) if d_ else prb.sample(64)
        assert [a[0] for a in dev.asked[-2:]] == ["prio_sample", "replay_sample"]
        assert dev.asked[-2] == ("prio_sample", 64, 6, d_) and dev.asked[-1] == ("replay_sample", 64, True) and prb.draws == d_ + 1
        assert isinstance(mb, DeviceBatch) and mb.count == 64 == len(mb) and mb.epoch == d_ and mb.row is None and mb.col is None
        want_s, want_p = dev.tree.sample(64, 6, d_, 12)
        assert mb.slots.tolist() == want_s.tolist() and mb.priorities.numpy().tobytes() == want_p.tobytes()
        assert mb.slots.dtype == torch.int64 and mb.priorities.dtype == torch.float32 and mb.weights.dtype == torch.float32
        assert ((want_s >= 0) & (want_s < 12)).all() and (mb.records.numpy() == prb.ring.numpy()[want_s]).all()
        pmin = float(dev.tree.pmin())
        assert pmin == float(prb.tree[:12].min()) and abs(pmin - 0.9) < 1e-6
        np.testing.assert_allclose(mb.weights.numpy(), (pmin / want_p.astype(np.float64)) ** beta, rtol=1e-5)
        assert mb.weights.max() <= 1.0 and (beta > 0 or (mb.weights == 1).all())
    for bad in (-0.1, 1.5, None, True, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            prb.sample(4, beta=bad)
    g = prb.gather(torch.tensor([11, 12, 0], dtype=torch.int64))   # the parent's
    assert g.slots.tolist() == [11, -1, 0]
    # nothing held: slots -1, weights 0
    empty = ph.PrioritizedReplayBuffer(None, 5)
    edev = _Dev()
    empty.add(_batch(edev, 0, 4, 5))
    mb = empty.sample(6)
    assert mb.slots.tolist() == [-1] * 6 and (mb.weights == 0).all() and (mb.priorities == 0).all() and (mb.records == 0).all()
    # the constructor's refusals, and check_replay takes it as a ReplayBuffer
    for kw, match in ((dict(capacity=0), "capacity"), (dict(capacity=2 ** 30 + 1), "capacity"), (dict(alpha=0), "alpha"), (dict(alpha=-1.0), "alpha"),
                      (dict(alpha=None), "alpha"), (dict(alpha=True), "alpha"), (dict(eps=-1e-6), "eps"), (dict(eps=None), "eps"), (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match=match):
            ph.PrioritizedReplayBuffer(None, **dict(dict(capacity=4), **kw))

    class _Batcher:
        max_seq_len, policies = None, ["default_policy"]
    assert check_replay(prb, _Batcher()) == {"default_policy": prb}
    with pytest.raises(ValueError, match="layout"):
        prb.add(_batch(dev, 3, 3, 4, words=12))
    assert dev.asked[-1][0] == "replay_sample"                     # the refused add reached neither call
    assert (len(prb), prb.total, prb.refused, prb.ignored) == (12, 12, 1, 2)
