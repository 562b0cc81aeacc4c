"""phx_seq_batch (include/phantom_amd_seq.h) on the GPU, through the C ABI into fenced and poisoned buffers: bit-equality with the numpy
restatement (tests/seq_ref.py) of seq_start, records, out_row, out_col, seq_lens, seq_row, seq_col and moments over row counts around
the scatter's chunk depth, column counts around its tile width and one beyond the scan's block, sequence lengths that close inside a
chunk, on its last row, across a boundary and only at the column's end, Q on both sides of powers of 4, the layouts, keep / flag planes
NULL, classes, both shuffle settings and the standardized plane; the capacity rule, row slices at odd offsets, every refusal,
phx_last_kernel, two calls on one stream, L = 1 against a real phx_train_batch call; then DeviceEnv.seq_batch and
sample(batcher=TrainBatcher(max_seq_len=L)) on real rollouts."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_ref as br
import compact_ref as cr
import seq_ref as sr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, fenced
from helpers import supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import DeviceSeqBatch

pytestmark = pytest.mark.gpu
SRC = open(os.path.join(os.path.dirname(HERE), "phantom_amd", "csrc", "phx_seq_batch.hip")).read()
R = int(re.search(r"constexpr int SQ_R = (\d+);", SRC).group(1))                  # the scatter's chunk depth (rows)
CW = int(re.search(r"constexpr int SQ_C = (\d+);", SRC).group(1))                 # the scatter's tile width (columns)
SB = int(re.search(r"constexpr int SQ_SB = (\d+);", SRC).group(1))                # the scan's block (entries)
TS = (1, R - 1, R, R + 1, 2 * R + 1)
NS = (1, CW - 1, CW, CW + 1, 4 * CW + 1)
EINVAL = -1
# elem_bytes, word_offs (None: packed in order), row_words (None: the default); with a standardized plane, a 4-byte one appended:
# its word_off and the row_words then
LAYOUTS = {"packed": ((1, 4, 12, 20), None, None, None, None),
           "lone byte": ((1,), (0,), 4, 5, 8),
           "gaps": ((1, 4, 12, 20), (2, 17, 5, 9), 20, 15, 20),             # words 0-1, 3-4, 8, 14-16, 18-19 belong to no plane
           "widest": ((4, 1, 256, 12, 20), (250, 255, 3, 70, 100), 256, 0, 256)}
SEQ_OUTS = ("seq_lens", "seq_row", "seq_col")
SLOT_OUTS = ("records", "out_row", "out_col")


def _lens(T):
    return sorted({L for L in (1, 2, R - 1, R, R + 1, T + 3) if L >= 1})


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _offset(host, nbytes):
    """`host` on the device, starting `nbytes` bytes past a 16-byte boundary (0: on one)"""
    a = np.ascontiguousarray(host)
    a = a if a.dtype == np.uint8 else a.view(np.int32)
    raw = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device=_dev())
    assert raw.data_ptr() % 16 == 0
    x = raw[nbytes:nbytes + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    x.copy_(torch.from_numpy(a))
    assert x.data_ptr() % 16 == nbytes
    return x


def _std_source(rng, keep_mask, T, N):
    """f32 3 * N(0, 1) + 1 as u32 bit patterns; what is not kept may hold anything: a NaN and an infinity where there is room"""
    x = (3.0 * rng.standard_normal((T, N)) + 1.0).astype(np.float32)
    holes = np.argwhere(~keep_mask)
    for (t, n), bad in zip(holes[:2], (np.nan, np.inf)):
        x[t, n] = bad
    return x.view(np.uint32)


def _flags(T, N, keep_mask, rate, seed=0):
    """a flag plane: any non-zero byte is a set flag; GARBAGE at the rows that are not kept"""
    rng = np.random.default_rng([seed, T, N, int(rate * 100)])
    f = (rng.random((T, N)) < rate).astype(np.uint8) * rng.integers(1, 256, (T, N)).astype(np.uint8)
    holes = ~keep_mask
    f[holes] = rng.integers(0, 256, int(holes.sum())).astype(np.uint8)
    return f


class Call:
    """one phx_seq_batch call: device inputs, fenced and poisoned outputs, the restatement's result in `want`"""

    def __init__(self, T, N, L, keep, term="random", trunc="random", layout="packed", std=False, shuffle=1, seed=0, epoch=0, col_class=None,
                 class_id=0, capacity=None, absent=(), keep_offset=0, byte_offset=0, word_offset=0, case=0):
        self.T, self.N, self.L, self.keep = T, N, L, keep
        elem_bytes, offs, row_words, std_off, std_row_words = LAYOUTS[layout]
        if offs is None:
            offs, row_words = br.default_layout(elem_bytes + ((4,) if std else ()))
        elif std:
            offs, row_words = list(offs) + [std_off], std_row_words
        self.row_words, self.offs = row_words, offs
        rng = np.random.default_rng([case, T, N, L])
        mask = br.kept_mask(T, N, keep, col_class, class_id)
        self.term = _flags(T, N, mask, 0.15, case) if isinstance(term, str) else term
        self.trunc = _flags(T, N, mask, 0.1, case + 1) if isinstance(trunc, str) else trunc
        self.src = [cr.plane_case(rng, T, N, eb) for eb in elem_bytes] + ([_std_source(rng, mask, T, N)] if std else [])
        self.elem_bytes = list(elem_bytes) + ([4] if std else [])
        self.std_plane = len(self.src) - 1 if std else -1
        self.kw = dict(keep=keep, terminated=self.term, truncated=self.trunc, col_class=col_class, class_id=class_id, shuffle=shuffle, seed=seed,
                       epoch=epoch, std_plane=self.std_plane)
        planes = list(zip(self.src, offs))
        if capacity is None:                            # room for three sequences more than there are
            capacity = sr.seq_batch(T, N, [], row_words, L, **dict(self.kw, std_plane=-1))["Q"] + 3
        self.capacity = capacity
        self.want = sr.seq_batch(T, N, planes, row_words, L, capacity=capacity, **self.kw)
        self.Q, self.K = self.want["Q"], self.want["K"]
        self.dev_keep = None if keep is None else _offset(keep, keep_offset)
        self.dev_term = None if self.term is None else _offset(self.term, keep_offset + 2)
        self.dev_trunc = None if self.trunc is None else _offset(self.trunc, keep_offset + 5)
        self.dev_class = None if col_class is None else _offset(np.asarray(col_class, np.uint8), 1)
        self.dev_src = [_offset(v, byte_offset if v.dtype == np.uint8 else word_offset) for v in self.src]
        i32, u8 = torch.int32, torch.uint8
        shapes = {"seq_start": ((N + 1,), torch.int64), "records": ((capacity * L, row_words), i32), "out_row": ((capacity * L,), i32),
                  "out_col": ((capacity * L,), i32), "seq_lens": ((capacity,), i32), "seq_row": ((capacity,), i32), "seq_col": ((capacity,), i32),
                  "moments": ((32,), u8) if std else None, "workspace": ((24 * N,), u8) if std else None}
        for k in absent:
            shapes[k] = None
        self.out, self.whole = {}, {}
        for k, sd in shapes.items():
            self.out[k], self.whole[k] = fenced(sd[0], sd[1], _dev()) if sd else (None, None)

        def o(k):                                       # (an empty buffer has no data_ptr(): the byte behind the leading guard)
            if self.out[k] is None:
                return None
            w = self.whole[k]
            return w.data_ptr() + (w.shape[0] - self.out[k].shape[0]) // 2 * (w[0].numel() * w.element_size())
        p = lambda x: None if x is None else x.data_ptr()
        self.io = _abi.PhxSeqBatchIO(T=T, N=N, capacity=capacity, n_planes=len(self.src), row_words=row_words,
                                     S=1 if col_class is None else len(col_class), class_id=class_id, std_plane=self.std_plane, shuffle=shuffle,
                                     seed=seed, epoch=epoch, keep=p(self.dev_keep), col_class=p(self.dev_class), max_seq_len=L,
                                     terminated=p(self.dev_term), truncated=p(self.dev_trunc), **{k: o(k) for k in shapes})
        for i, eb in enumerate(self.elem_bytes):
            self.io.plane[i] = _abi.PhxBatchPlane(src=self.dev_src[i].data_ptr(), elem_bytes=eb, word_off=offs[i])

    def launch(self):
        return _abi.load_library().phx_seq_batch(C.byref(self.io), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def check(self, what=""):
        w = self.want
        for k, whole in self.whole.items():
            if whole is not None:
                assert_fences(whole, self.out[k].shape[0], what + k)
        np.testing.assert_array_equal(self.out["seq_start"].cpu().numpy(), w["seq_start"], err_msg=what + "seq_start")
        if self.std_plane >= 0:
            got = self.out["moments"].cpu().numpy().view(br.MOMENTS_DTYPE)[0]
            assert got.tobytes() == w["moments"].tobytes(), f"{what}moments: {got} != {w['moments']}"
        q_out = self.Q if self.Q <= self.capacity else 0          # (Q > capacity: nothing but seq_start and moments is written)
        for k in SLOT_OUTS + SEQ_OUTS:
            if self.out[k] is None:
                continue
            n_out = q_out * (self.L if k in SLOT_OUTS else 1)
            if n_out:
                got = self.out[k][:n_out].cpu().numpy()
                bad = np.flatnonzero((got.view(np.uint32) != w[k].view(np.uint32)).reshape(n_out, -1).any(axis=1))
                assert bad.size == 0, f"{what}{k}: {bad.size} of {n_out} entries differ, first at {bad[:5]}"
            assert_poison(self.out[k][n_out:], f"{what}{k}: entries [{n_out}, ..)")
        for dev, host, name in ((self.dev_keep, self.keep, "keep"), (self.dev_term, self.term, "terminated"), (self.dev_trunc, self.trunc, "truncated")):
            assert dev is None or dev.cpu().numpy().tobytes() == host.tobytes(), what + name      # the inputs are byte-identical after the call
        for i, v in enumerate(self.src):
            assert self.dev_src[i].cpu().numpy().tobytes() == v.tobytes(), f"{what}plane {i}"

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for k, w in self.whole.items():
            if w is not None:
                assert_poison(w, f"{what}: {k}")


def _keep(T, N, density, seed=0):
    return cr.keep_case(np.random.default_rng([seed, T, N, cr.DENSITIES.index(density)]), T, N, density)


def _run(T, N, L, keep, **kw):
    call = Call(T, N, L, keep, **kw)
    assert call.launch() == 0, _abi.load_library().phx_last_error()
    call.check(f"T={T} N={N} L={L} {sorted((k, str(v)[:20]) for k, v in kw.items() if k != 'col_class')}: ")
    return call


# the rest of the parameter space, walked along the (T, L) grid of every N
CONFIGS = (dict(layout="packed", std=False, shuffle=1), dict(layout="packed", std=True, shuffle=1), dict(layout="lone byte", shuffle=1),
           dict(layout="gaps", std=True, shuffle=0), dict(layout="widest", std=True, shuffle=1), dict(layout="gaps", shuffle=1),
           dict(layout="packed", std=True, shuffle=0), dict(layout="widest", shuffle=0), dict(layout="lone byte", std=True, shuffle=1))
FLAGS = (dict(), dict(term=None), dict(trunc=None), dict(term=None, trunc=None))


@pytest.mark.parametrize("N", NS)
def test_bit_equal_to_the_restatement(N):
    i = NS.index(N)
    for T in TS:
        for L in _lens(T):
            density = cr.DENSITIES[i % len(cr.DENSITIES)]
            call = _run(T, N, L, _keep(T, N, density), seed=0xDEADBEEF12345678 + i, epoch=i, case=i, **CONFIGS[i % len(CONFIGS)], **FLAGS[i % len(FLAGS)])
            assert call.Q <= call.K <= T * N and call.Q < call.capacity
            i += 1


def test_sequences_that_only_the_length_or_the_column_end_closes():
    """no flag anywhere and every row kept: a sequence closes inside a chunk, on a chunk's last row, across a chunk boundary, or only
    at the column's end"""
    for T in TS:
        for L in _lens(T):
            for N in (CW + 1, 3):
                call = _run(T, N, L, None, term=None, trunc=None, std=True, seed=L, epoch=T)
                assert call.Q == N * -(-T // L) and call.K == T * N
                call = _run(T, N, L, _keep(T, N, "random 0.5"), term=None, trunc=None, layout="gaps", seed=L)


def _keep_with_q(T, N, L, Q):
    """a keep plane (no flags) with exactly Q sequences: whole columns of ceil(T / L) sequences, then single rows"""
    per = -(-T // L)
    k = np.zeros((T, N), np.uint8)
    full, rest = divmod(Q, per)
    assert full + (rest > 0) <= N
    k[:, :full] = 1
    if rest:
        k[:(rest - 1) * L + 1, full] = 1
    return k


def test_q_on_both_sides_of_powers_of_four():
    """w, h and the mask change where Q passes a power of 4"""
    T, L = 2 * R + 1, R - 1
    for N in (4 * CW + 1, 22 * CW):
        for j in range(1, 7):
            for Q in (4 ** j - 1, 4 ** j, 4 ** j + 1):
                if Q <= N * -(-T // L) and (N < 1000) == (Q < 700):
                    call = _run(T, N, L, _keep_with_q(T, N, L, Q), term=None, trunc=None, layout="lone byte", std=(j % 2 == 0), seed=j, epoch=Q)
                    assert call.Q == Q
    for Q in (0, 1, 2):
        assert _run(R + 1, CW + 1, 3, _keep_with_q(R + 1, CW + 1, 3, Q), term=None, std=True, seed=3).Q >= Q


def test_keep_null_keeps_everything():
    for T, N in ((1, 1), (R + 1, CW + 1), (2 * R + 1, 4 * CW + 1)):
        for cfg in CONFIGS[:4]:
            assert _run(T, N, 3, None, seed=T, **cfg).K == T * N


def test_classes_select_their_columns():
    classes = np.array([0, 1, 0], np.uint8)                      # S = 3: agents 0 and 2 share a policy
    for N in (3, CW - 1, 4 * CW + 2):
        for T in (1, R + 1):
            rows = seqs = 0
            keep = _keep(T, N, "random 0.5")
            for class_id in (0, 1, 2):
                call = _run(T, N, 3, keep, std=True, col_class=classes, class_id=class_id, seed=7, epoch=class_id)
                rows, seqs = rows + call.K, seqs + call.Q
                assert class_id != 2 or call.Q == 0               # a class no column belongs to
                _run(T, N, 3, None, col_class=classes, class_id=class_id, seed=7)
            whole = _run(T, N, 3, keep, seed=7)
            assert rows == int((keep != 0).sum()) == whole.K     # the classes partition the kept elements


def test_the_capacity_rule():
    for T, N, L in ((R + 1, CW + 1, 3), (5, 4 * CW + 1, R)):
        keep = _keep(T, N, "random 0.5")
        Q = Call(T, N, L, keep).Q
        assert Q > 2
        for cap in (Q - 1, Q // 2, 0, Q, Q + 1):
            for std in (False, True):
                call = _run(T, N, L, keep, std=std, capacity=cap, seed=9)
                assert call.Q == Q and (call.want["records"] is None) == (cap < Q)


def test_optional_outputs_and_last_kernel():
    lib = _abi.load_library()
    T, N, L = R + 1, CW + 1, 3
    keep = _keep(T, N, "random 0.5")
    for absent in [(k,) for k in SLOT_OUTS[1:] + SEQ_OUTS] + [SLOT_OUTS[1:], SEQ_OUTS, SLOT_OUTS[1:] + SEQ_OUTS]:
        _run(T, N, L, keep, absent=absent, std=True)
        assert lib.phx_last_kernel() == _abi.SEQ_KERNELS.encode()
    _run(T, N, L, keep)
    assert lib.phx_last_kernel() == b"phx_seq_count_kernel+phx_seq_scan_kernel+phx_seq_scatter_kernel"
    _run(T, N, L, keep, capacity=0, std=True)                             # nothing to write: no scatter
    assert lib.phx_last_kernel() == b"phx_seq_count_kernel+phx_seq_scan_kernel+phx_seq_moments_kernel"
    _run(T, N, L, _keep(T, N, "none"), capacity=0)
    assert lib.phx_last_kernel() == b"phx_seq_count_kernel+phx_seq_scan_kernel"
    call = Call(T, N, L, _keep(T, N, "alternating"))                      # n_planes = 0 without records: the indices alone
    call.io.n_planes, call.io.records = 0, None
    assert call.launch() == 0, lib.phx_last_error()
    torch.cuda.synchronize()
    assert_poison(call.whole["records"], "records were not given")
    call.whole["records"] = call.out["records"] = None
    call.check("n_planes = 0: ")
    call = Call(T, N, L, keep, std=True)                                  # no output but seq_start and moments: no scatter
    for k in SLOT_OUTS + SEQ_OUTS:
        setattr(call.io, k, None)
    call.io.n_planes, call.io.std_plane = 0, -1
    assert call.launch() == 0, lib.phx_last_error()
    assert lib.phx_last_kernel() == b"phx_seq_count_kernel+phx_seq_scan_kernel"
    np.testing.assert_array_equal(call.out["seq_start"].cpu().numpy(), call.want["seq_start"])
    for k in SLOT_OUTS + SEQ_OUTS + ("moments",):
        assert_poison(call.whole[k], k)


@pytest.mark.parametrize("keep_offset,byte_offset,word_offset", [(1, 3, 4), (7, 1, 12)])
def test_inputs_that_are_row_slices_of_a_longer_recording(keep_offset, byte_offset, word_offset):
    for T, N in ((R + 1, CW + 1), (3, 4 * CW + 1), (5, 3)):
        for cfg in (CONFIGS[1], CONFIGS[4]):
            _run(T, N, 2, _keep(T, N, "random 0.5"), keep_offset=keep_offset, byte_offset=byte_offset, word_offset=word_offset, **cfg)


def test_columns_beyond_one_block_of_the_scan():
    for density in ("random 0.5", "alternating"):
        _run(3, SB + 65, 2, _keep(3, SB + 65, density), std=True, seed=5)
    _run(2, 2 * SB, 1, _keep(2, 2 * SB, "random 0.9"), layout="lone byte")


def test_sequences_of_one_row_are_a_real_train_batch_call():
    lib = _abi.load_library()
    for T, N, std in ((R + 1, CW + 1, True), (2 * R + 1, 4 * CW + 1, False), (3, 5, True)):
        keep = _keep(T, N, "random 0.5")
        call = _run(T, N, 1, keep, std=std, seed=21, epoch=4)
        K = call.K
        assert call.Q == K and (call.out["seq_lens"][:K] == 1).all()
        outs = {"start": fenced((N + 1,), torch.int64, _dev()), "records": fenced((K, call.row_words), torch.int32, _dev()),
                "out_row": fenced((K,), torch.int32, _dev()), "out_col": fenced((K,), torch.int32, _dev()),
                "moments": fenced((32,), torch.uint8, _dev()), "workspace": fenced((16 * N,), torch.uint8, _dev())}
        io = _abi.PhxTrainBatchIO(T=T, N=N, capacity=K, n_planes=len(call.src), row_words=call.row_words, S=1, class_id=0, std_plane=call.std_plane,
                                  shuffle=1, seed=21, epoch=4, keep=call.dev_keep.data_ptr(),
                                  **{k: v[0].data_ptr() for k, v in outs.items() if std or k not in ("moments", "workspace")})
        for i, eb in enumerate(call.elem_bytes):
            io.plane[i] = _abi.PhxBatchPlane(src=call.dev_src[i].data_ptr(), elem_bytes=eb, word_off=call.offs[i])
        assert lib.phx_train_batch(C.byref(io), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib.phx_last_error()
        for a, b in (("seq_start", "start"), ("records", "records"), ("out_row", "out_row"), ("out_col", "out_col")) + ((("moments", "moments"),) if std else ()):
            n = call.out[a].shape[0] if a in ("seq_start", "moments") else K
            assert call.out[a][:n].cpu().numpy().tobytes() == outs[b][0].cpu().numpy().tobytes(), (a, T, N)


def test_two_calls_on_one_stream_into_different_buffers():
    a = Call(2 * R + 1, 4 * CW + 1, R - 1, _keep(2 * R + 1, 4 * CW + 1, "random 0.5", seed=11), std=True, seed=11)
    b = Call(R - 1, 2 * CW + 2, 2, _keep(R - 1, 2 * CW + 2, "alternating", seed=12), layout="gaps", absent=("out_col", "seq_row"), seed=12)
    assert a.launch() == 0 and b.launch() == 0          # back to back, nothing in between
    a.check("first: ")
    b.check("second: ")


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _abi.load_library()
    T, N, L = R + 1, 3 * CW, 3                          # (N % 3 == 0: S = 3 is a good value to start from)
    call = Call(T, N, L, _keep(T, N, "random 0.5", seed=1), std=True, col_class=np.array([0, 0, 0], np.uint8), seed=1)
    names = [n for n, _ in _abi.PhxSeqBatchIO._fields_ if n not in ("plane", "reserved")]
    good = {n: getattr(call.io, n) for n in names}
    good_planes = [(p.src, p.elem_bytes, p.word_off) for p in call.io.plane]

    def restore():
        for n, v in good.items():
            setattr(call.io, n, v)
        call.io.reserved[0] = call.io.reserved[1] = 0
        for i, (src, eb, off) in enumerate(good_planes):
            call.io.plane[i] = _abi.PhxBatchPlane(src=src, elem_bytes=eb, word_off=off)

    def refused(what, plane=None, **patch):
        restore()
        for k, v in patch.items():
            target = call.io if plane is None else call.io.plane[plane]
            setattr(target, k, v(getattr(target, k)) if callable(v) else v)
        assert call.launch() == EINVAL, what
        assert b"phx_seq_batch" in lib.phx_last_error(), what
        call.check_untouched(what)

    refused("seq_start NULL", seq_start=None)
    refused("records NULL with planes", records=None)
    for k, bad in (("T", 0), ("T", -3), ("T", 1 << 31), ("N", 0), ("N", -1), ("S", 0), ("S", -1), ("S", 5), ("S", N + 3), ("n_planes", -1),
                   ("n_planes", 33), ("capacity", -1), ("row_words", 0), ("row_words", 8), ("row_words", 18), ("row_words", 260),
                   ("std_plane", -2), ("std_plane", 5), ("std_plane", 0), ("std_plane", 2), ("shuffle", 2), ("shuffle", -1),
                   ("max_seq_len", 0), ("max_seq_len", -1), ("max_seq_len", 65537), ("max_seq_len", 1 << 40)):
        refused(f"{k} = {bad}", **{k: bad})
    refused("capacity * max_seq_len > 2^62", capacity=(1 << 47), max_seq_len=65536)
    refused("T * N > 2^62", T=(1 << 31) - 1, N=3 << 31, out_col=None, seq_col=None)
    refused("N beyond one launch's grid", N=3 * ((CW * 0x7fffffff) // 3 + 1), out_col=None, seq_col=None)
    refused("out_col with N > 2^31 - 1", N=3 << 30, seq_col=None)
    refused("seq_col with N > 2^31 - 1", N=3 << 30, out_col=None)
    refused("moments NULL with std_plane", moments=None)
    refused("workspace NULL with std_plane", workspace=None)
    for r in (0, 1):
        restore()
        call.io.reserved[r] = 1
        assert call.launch() == EINVAL and b"phx_seq_batch" in lib.phx_last_error()
        call.check_untouched(f"reserved[{r}]")
    for i in (0, 3):
        refused(f"plane {i} src NULL", plane=i, src=None)
        for bad in (0, -4, 2, 3, 6, 260, 1 << 20):
            refused(f"plane {i} elem_bytes = {bad}", plane=i, elem_bytes=bad)
        refused(f"plane {i} before the record", plane=i, word_off=-1)
        refused(f"plane {i} beyond the record", plane=i, word_off=call.row_words - (0 if i == 0 else 4))
    refused("plane 2 overlaps plane 3", plane=2, word_off=call.offs[3] - 1)
    refused("plane 0 overlaps plane 1", plane=0, word_off=call.offs[1])
    refused("a word plane's src off a 4-byte boundary", plane=1, src=lambda p: p + 2)
    for k in ("seq_start", "records", "out_row", "out_col", "seq_lens", "seq_row", "seq_col", "moments", "workspace"):
        refused(f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    assert lib.phx_seq_batch(None, None) == EINVAL and b"phx_seq_batch" in lib.phx_last_error()
    restore()                                           # and the same buffers receive a good call
    assert call.launch() == 0, lib.phx_last_error()
    call.check("after the refusals: ")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
T_E2E = 20                                               # crosses two episode boundaries of the envs below
L_E2E = 3


def _fsm_env(seed=5):
    env = supply_chain_env(5, [3] * 5, 8, 4, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


def _plain_env(seed=5):
    env = supply_chain_env(9, [6] * 9, 7, 8, seed=seed, exogenous="device")
    env.reset()
    return env


def _critic(x):
    return 0.5 * x[:, 0] - 0.25 * torch.tanh(x[:, 1]) + 0.125 * x[:, -1] * x[:, -1] + 0.75


def _bits(x):
    a = np.ascontiguousarray(x)
    return a.view(np.uint8) if a.dtype == np.bool_ else a


@pytest.mark.parametrize("make", [_fsm_env, _plain_env], ids=["fsm", "plain"])
def test_device_env_seq_batch_on_a_real_rollout(make):
    env = make()
    tr = env.rollout(12)
    dev = env._device()
    B, S, T, L = dev.B, dev.S, 12, 4
    keep = getattr(tr, "obs_valid", None)
    planes = {"obs": tr.observations, "rewards": tr.rewards, "truncateds": tr.truncations}
    res = dev.seq_batch(planes, L, keep=keep, truncated=tr.truncations, terminated=tr.terminations, standardize="rewards", seed=3, epoch=1)
    start, records, lens, srow, scol, orow, ocol, moments, layout = res
    assert dev.last_kernel() == _abi.SEQ_KERNELS
    assert layout == {"obs": (0, 3, torch.float32), "rewards": (3, 1, torch.float32), "truncateds": (4, 1, torch.uint8)}
    cap = records.shape[0]
    assert tuple(records.shape) == (cap, L, 16) and records.dtype == torch.int32 and tuple(start.shape) == (B * S + 1,) and cap == T * B * S
    assert tuple(orow.shape) == tuple(ocol.shape) == (cap, L) and tuple(lens.shape) == tuple(srow.shape) == tuple(scol.shape) == (cap,)
    host = lambda x: None if x is None else x.cpu().numpy().reshape(T, B * S)
    src = [np.ascontiguousarray(x.cpu().numpy()).reshape((T, B * S) + tuple(x.shape[3:])) for x in planes.values()]
    src = [s if s.dtype == np.uint8 else s.view(np.uint32) for s in src]
    ref = sr.seq_batch(T, B * S, list(zip(src, (0, 3, 4))), 16, L, keep=host(keep), terminated=host(tr.terminations), truncated=host(tr.truncations),
                       seed=3, epoch=1, std_plane=1)
    Q = ref["Q"]
    assert B * S < Q < cap and int(start[-1]) == Q and ref["seq_lens"].max() == L and ref["seq_lens"].min() < L
    assert records[:Q].cpu().numpy().view(np.uint32).tobytes() == ref["records"].tobytes()
    assert moments.cpu().numpy().tobytes() == ref["moments"].tobytes()
    for got, k in ((lens, "seq_lens"), (srow, "seq_row"), (scol, "seq_col"), (orow, "out_row"), (ocol, "out_col")):
        assert got[:Q].cpu().numpy().tobytes() == ref[k].tobytes(), k


def test_device_env_seq_batch_checks_its_arguments_before_any_launch():
    env = _fsm_env()
    tr = env.rollout(8)
    dev = env._device()
    B, S, L = dev.B, dev.S, 3
    planes = {"obs": tr.observations, "rewards": tr.rewards, "truncateds": tr.truncations}
    Q = int(dev.seq_batch(planes, L, keep=tr.obs_valid, truncated=tr.truncations)[0][-1])
    d = dev.device
    outs = {"start": fenced((B * S + 1,), torch.int64, d), "records": fenced((Q, L, 8), torch.int32, d), "lens": fenced((Q,), torch.int32, d),
            "row": fenced((Q, L), torch.int32, d), "moments": fenced((32,), torch.uint8, d), "workspace": fenced((3, B * S), torch.float64, d)}
    out = (outs["start"][0], outs["records"][0], outs["lens"][0], None, None, outs["row"][0], None, outs["moments"][0], outs["workspace"][0])
    good = dict(keep=tr.obs_valid, truncated=tr.truncations, standardize="rewards", row_words=8, capacity=Q, out=out, seed=3, epoch=1)
    for match, bad in (("keep", dict(keep=tr.obs_valid.to(torch.int32))), ("keep", dict(keep=tr.obs_valid.cpu())), ("truncated", dict(truncated=tr.rewards)),
                       ("terminated", dict(terminated=tr.truncations[:4])), ("standardize", dict(standardize="obs")),
                       ("standardize", dict(standardize="nothing")), ("row_words", dict(row_words=6)), ("row_words", dict(row_words=4)),
                       ("capacity", dict(capacity=-1)), (r"out\[1\]", dict(capacity=Q + 1)), ("class_id", dict(class_id=256)),
                       ("col_class", dict(col_class=torch.zeros(S + 1, dtype=torch.uint8, device=d))), ("seed", dict(seed=-1)),
                       ("epoch", dict(epoch=2 ** 64)), ("out", dict(out=out[:8])), (r"out\[7\]", dict(out=out[:7] + (None, None)))):
        with pytest.raises(ValueError, match=match):
            dev.seq_batch(planes, L, **dict(good, **bad))
    for bad in (0, 65537, 2.5, True, None):
        with pytest.raises(ValueError, match="max_seq_len"):
            dev.seq_batch(planes, bad, **good)
    with pytest.raises(ValueError, match="rewards"):
        dev.seq_batch(dict(planes, rewards=tr.rewards.double()), L, **good)
    with pytest.raises(ValueError, match="planes"):
        dev.seq_batch({f"p{i}": tr.rewards for i in range(33)}, L, keep=tr.obs_valid)
    torch.cuda.synchronize()
    for k, (_, whole) in outs.items():
        assert_poison(whole, f"a refused DeviceEnv.seq_batch call: {k}")
    res = dev.seq_batch(planes, L, **good)
    assert res[1].data_ptr() == out[1].data_ptr() and res[3] is None and res[4] is None and res[6] is None
    for k, (plane, whole) in outs.items():
        assert_fences(whole, plane.shape[0], k)
    host = lambda x: x.cpu().numpy().reshape(8, B * S)
    src = [np.ascontiguousarray(x.cpu().numpy()).reshape((8, B * S) + tuple(x.shape[3:])) for x in planes.values()]
    src = [s if s.dtype == np.uint8 else s.view(np.uint32) for s in src]
    ref = sr.seq_batch(8, B * S, list(zip(src, (0, 3, 4))), 8, L, keep=host(tr.obs_valid), truncated=host(tr.truncations), seed=3, epoch=1, std_plane=1)
    assert ref["Q"] == Q and res[1].cpu().numpy().view(np.uint32).tobytes() == ref["records"].tobytes()
    assert res[2].cpu().numpy().tobytes() == ref["seq_lens"].tobytes() and res[5].cpu().numpy().tobytes() == ref["out_row"].tobytes()


@pytest.mark.parametrize("make", [_fsm_env, _plain_env], ids=["fsm", "plain"])
def test_sample_with_a_sequence_batcher_gives_the_sample_batches_as_sequences(make):
    env, twin = make(), make()
    kw = dict(value_fn=_critic, gamma=0.99, lambda_=0.95)
    ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
    fn = lambda aid: "even" if ids.index(aid) % 2 == 0 else "odd"
    tb = ph.TrainBatcher(env, seed=0xDEADBEEF12345678, policy_mapping_fn=fn, max_seq_len=L_E2E)
    S, L = env.spec.n_strategic, L_E2E
    for call in range(2):                                   # the second call continues the episodes under the next epoch
        got = env.sample(T_E2E, batcher=tb, **kw)
        assert env._device().last_kernel() == _abi.SEQ_KERNELS and tb.calls == call + 1
        want = twin.sample(T_E2E, **kw).to_sample_batches(fn)
        assert set(got) == set(want) == {"even", "odd"}
        for pid in tb.policies:
            sb = got[pid]
            assert isinstance(sb, DeviceSeqBatch) and sb.epoch == call and sb.standardized == "advantages" and sb.max_seq_len == L
            Q, K = sb.num_sequences, sb.count
            assert K == len(want[pid]["obs"]) and 0 < Q <= sb.records.shape[0] and K <= Q * L
            lens, mask = sb.seq_lens.cpu().numpy(), sb.mask.cpu().numpy()
            assert ((lens >= 1) & (lens <= L)).all() and lens.sum() == K and lens.min() < L == lens.max()
            row, col = sb.row.cpu().numpy(), sb.col.cpu().numpy()
            assert ((row == -1) == ~mask).all() and ((col == -1) == ~mask).all()
            assert (sb.seq_row.cpu().numpy() == row[:, 0]).all() and (sb.seq_col.cpu().numpy() == col[:, 0]).all()
            # undo the order: the kept slots sorted by (column, row) are to_sample_batches()'s rows
            order = np.lexsort((row[mask], col[mask]))
            index = np.full((Q, L), -1, np.int64)                # a slot's row in the sample batch
            flat = np.flatnonzero(mask.reshape(-1))
            index.reshape(-1)[flat[order]] = np.arange(K)
            assert ((np.diff(index, axis=1) == 1) | ~mask[:, 1:]).all()     # a sequence: consecutive rows of one agent, in time order
            np.testing.assert_array_equal(col[mask][order] // S, want[pid]["env_id"])
            np.testing.assert_array_equal(col[mask][order] % S, want[pid]["agent_index"])
            eps = np.where(mask, want[pid]["eps_id"][np.maximum(index, 0)], -1)
            assert ((eps == eps[:, :1]) | ~mask).all()           # no sequence crosses an episode boundary
            cols = sb.columns
            device_names = set(want[pid]) - {"eps_id", "agent_index", "t", "env_id", "action_prob"}
            assert set(cols) == device_names, set(cols) ^ device_names
            for name in device_names - {"advantages"}:
                full = cols[name].cpu().numpy()
                g, w = full[mask][order], want[pid][name]
                assert g.dtype == w.dtype and g.shape == w.shape, (pid, name, g.dtype, w.dtype, g.shape, w.shape)
                assert _bits(g).tobytes() == _bits(w).tobytes(), (call, pid, name)
                assert not _bits(full[~mask]).any(), (pid, name)  # padding is zero
            m = sb.moments.cpu().numpy().view(br.MOMENTS_DTYPE)[0]
            assert m["count"] == K
            std = ((want[pid]["advantages"] - m["mean"]) / m["den"]).astype(np.float32)
            adv = cols["advantages"].cpu().numpy()
            assert adv[mask][order].tobytes() == std.tobytes() and not adv[~mask].view(np.uint32).any(), (call, pid)
            sizes = [len(mb["seq_lens"]) for mb in sb.minibatches(5)]
            assert sum(sizes) == Q and all(n == 5 for n in sizes[:-1])
            with pytest.raises(ValueError, match="out of scope"):
                tb.reshuffle(sb)
    cr.assert_same_batches(env.sample(T_E2E, **kw).to_sample_batches(fn), twin.sample(T_E2E, **kw).to_sample_batches(fn), "afterwards: ")
    adapter = ph.rllib.BatchedBaseEnv(make()).sample(T_E2E, batcher=ph.TrainBatcher(make(), policy_mapping_fn=fn, max_seq_len=L), **kw)
    assert set(adapter) == {"even", "odd"} and all(isinstance(v, DeviceSeqBatch) for v in adapter.values())
