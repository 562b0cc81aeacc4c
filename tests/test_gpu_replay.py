"""phx_replay_add / phx_replay_sample (include/phantom_amd_replay.h) on the GPU, through the C ABI into fenced and poisoned buffers:
bit-equality with the numpy restatement (tests/replay_ref.py) of the whole ring and its state after every add of sequences that wrap
-- record widths 4, 12 and 256 words, rings of 1, 5 and 257 slots, counts 0, 1, C - 1, C, C + 1 and 3 C + 2 by host value and by
device pointer, refused counts -- and of every sampled record and slot for drawn and for given slots; add then sample without a wait,
every refusal, phx_last_kernel; then ReplayBuffer behind sample(batcher=..., replay=...) on a plain and an FSM supply chain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import replay_ref as rr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import DeviceBatch

pytestmark = pytest.mark.gpu
EINVAL = -1
POISON_WORD = 0xA5A5A5A5
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
SPECIAL_WORDS = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0xFFFFFFFF, 0x00000001)      # NaN payloads, -0.0, a denormal
ROW_WORDS = (4, 12, 256)
RINGS = (1, 5, 257)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    return _abi.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _records(rng, rows, row_words):
    """random words with the special ones planted: u32 [rows][row_words]"""
    a = rng.integers(0, 2 ** 32, (rows, row_words), dtype=np.uint64).astype(np.uint32)
    a[a == POISON_WORD] = 0                                      # (an unwritten word must be told from a copied one)
    flat = a.reshape(-1)
    if flat.size:
        at = rng.integers(0, flat.size, 2 * len(SPECIAL_WORDS))
        flat[at] = np.resize(np.array(SPECIAL_WORDS, np.uint32), at.size)
    return a


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(_dev())


class RingCase:
    """a fenced, poisoned ring with its zero-filled fenced state, and the restatement beside it"""

    def __init__(self, Cn, row_words):
        self.C, self.row_words = Cn, row_words
        self.ring, self.ring_whole = fenced((Cn, row_words), torch.int32, _dev())
        self.state, self.state_whole = fenced((4,), torch.int64, _dev())
        self.state.zero_()
        self.ref = rr.Ring(Cn, row_words, fill=POISON_WORD)

    def add_io(self, src, count=None, count_ptr=None, src_capacity=None):
        return _abi.PhxReplayAddIO(capacity=self.C, src_capacity=src.shape[0] if src_capacity is None else src_capacity,
                                   count=0 if count is None else count, row_words=self.row_words,
                                   count_ptr=None if count_ptr is None else count_ptr.data_ptr(), src=src.data_ptr() if src.shape[0] else None,
                                   ring=self.ring.data_ptr(), state=self.state.data_ptr())

    def add(self, host_src, K, by_pointer):
        """one phx_replay_add of the first K records of `host_src`; returns what must stay alive until the stream has run"""
        src = _to_dev(host_src)
        ptr = torch.tensor([K], dtype=torch.int64, device=_dev()) if by_pointer else None
        io = self.add_io(src, None if by_pointer else K, ptr)
        assert _lib().phx_replay_add(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        assert _lib().phx_last_kernel() == _abi.REPLAY_ADD_KERNELS.encode()
        self.ref.add(host_src, K)
        return src, ptr

    def check(self, what):
        assert_fences(self.ring_whole, self.C, what + "ring")
        assert_fences(self.state_whole, 4, what + "state")
        got = self.ring.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero((got != self.ref.ring).any(axis=1))
        assert bad.size == 0, f"{what}ring: {bad.size} of {self.C} slots differ, first at {bad[:5]}"
        st = self.state.cpu().numpy()
        assert st.tobytes() == self.ref.state().tobytes(), f"{what}state: {st.tolist()} != {self.ref.state()}"

    def sample(self, n, seed=0, draw=0, slot_in=None, with_slots=True):
        """one phx_replay_sample into fenced outputs, checked against the restatement; returns (out, out_slot) on the host"""
        out, out_whole = fenced((n, self.row_words), torch.int32, _dev())
        oslot, oslot_whole = fenced((n,), torch.int64, _dev()) if with_slots else (None, None)
        sin = None if slot_in is None else torch.tensor(slot_in, dtype=torch.int64, device=_dev())
        io = _abi.PhxReplaySampleIO(capacity=self.C, n=n, row_words=self.row_words, seed=seed, draw=draw, slot_in=None if sin is None else sin.data_ptr(),
                                    ring=self.ring.data_ptr(), state=self.state.data_ptr(), out=out.data_ptr(),
                                    out_slot=None if oslot is None else oslot.data_ptr())
        assert _lib().phx_replay_sample(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        assert _lib().phx_last_kernel() == _abi.REPLAY_SAMPLE_KERNEL.encode()
        what = f"C={self.C} row_words={self.row_words} size={self.ref.size} n={n} seed={seed} draw={draw}: "
        want, want_slot = self.ref.sample(n, seed, draw, slot_in)
        assert_fences(out_whole, n, what + "out")
        got = out.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{what}out: {bad.size} of {n} records differ, first at {bad[:5]}"
        if with_slots:
            assert_fences(oslot_whole, n, what + "out_slot")
            assert_written(oslot, what + "out_slot")
            np.testing.assert_array_equal(oslot.cpu().numpy(), want_slot, err_msg=what + "out_slot")
        return got, want_slot


def _counts(Cn):
    return [0, 1, Cn - 1, Cn, Cn + 1, 3 * Cn + 2]


@pytest.mark.parametrize("row_words", ROW_WORDS)
@pytest.mark.parametrize("Cn", RINGS)
def test_add_is_bit_equal_to_the_restatement(Cn, row_words):
    """every count in turn, then again in another order so that the cursor starts anywhere and wraps mid-call; the whole ring and the
    state are read back after every add: slots the definition does not name still hold the poison or their earlier record"""
    rng = np.random.default_rng([Cn, row_words])
    case = RingCase(Cn, row_words)
    cap = 3 * Cn + 2
    order = _counts(Cn)[1:3] + _counts(Cn) + [2, Cn + 1, 1, 3 * Cn + 2, 0, Cn - 1]
    for step, K in enumerate(order):
        rows = cap if step % 3 else max(K, 0)                    # src_capacity == K, and src_capacity beyond it
        case.add(_records(rng, rows, row_words), K, by_pointer=bool(step % 2))
        case.check(f"C={Cn} row_words={row_words} add {step} (K={K}): ")
        assert case.ref.size == Cn or case.ref.cursor == case.ref.size
    assert case.ref.total == sum(order) and case.ref.refused == 0


@pytest.mark.parametrize("Cn", RINGS)
def test_a_count_outside_the_source_is_refused_on_the_device(Cn):
    rng = np.random.default_rng(Cn)
    for first in (False, True):                                   # into the poisoned ring, and into one that holds records
        case = RingCase(Cn, 12)
        if first:
            case.add(_records(rng, Cn + 1, 12), Cn + 1, by_pointer=False)
        for n_refused, K in enumerate((Cn + 3, -1, I64_MIN, I64_MAX), 1):
            case.add(_records(rng, Cn + 2, 12), K, by_pointer=True)
            case.check(f"C={Cn} refused K={K}: ")
            assert case.ref.refused == n_refused
        if not first:
            assert_poison(case.ring, "a ring that only saw refused adds")
        case.add(_records(rng, 2, 12), 2, by_pointer=True)       # and a good call afterwards is accepted
        case.check(f"C={Cn} after the refusals: ")


def test_several_adds_on_one_stream_without_a_wait():
    rng = np.random.default_rng(3)
    for Cn, row_words in ((5, 4), (257, 12), (257, 256)):
        case, alive = RingCase(Cn, row_words), []
        for step, K in enumerate((3, Cn - 1, 2, Cn + 1, 1, 0, 3 * Cn + 2, 4)):
            alive.append(case.add(_records(rng, 3 * Cn + 2, row_words), K, by_pointer=bool(step % 2)))
        case.check(f"C={Cn} row_words={row_words} eight adds back to back: ")
        case.sample(65, seed=Cn)                                 # the sample sees them all, also without a wait


@pytest.mark.parametrize("row_words", ROW_WORDS)
def test_sample_is_bit_equal_to_the_restatement(row_words):
    rng = np.random.default_rng(row_words)
    Cn = 257
    case = RingCase(Cn, row_words)
    ns = (1, 63, 64, 65, 1000)
    for fill in (0, 1, Cn):                                       # size 0, 1 and C
        if fill:
            case.add(_records(rng, fill, row_words), fill - case.ref.size, by_pointer=False)
        assert case.ref.size == fill
        for i, n in enumerate(ns):
            got, slots = case.sample(n, seed=0xDEADBEEF12345678 + n, draw=fill + i, with_slots=bool((i + fill) % 2))
            assert ((slots == -1).all() and (got == 0).all()) if fill == 0 else ((slots >= 0) & (slots < fill)).all()
        case.sample(64, seed=2 ** 64 - 1, draw=2 ** 64 - 1)
    assert len(set(case.sample(1000, seed=1, draw=0)[1].tolist())) > 200      # a full ring of 257: most slots among 1000 draws
    words = case.sample(1000, seed=5, draw=1)[0]
    assert sum(bool((words == s).any()) for s in SPECIAL_WORDS) >= 4            # NaN payloads and -0.0 are copied as integers
    case.check("the samples changed neither ring nor state: ")


def test_the_known_answers_on_the_device():
    case = RingCase(1000, 4)
    host = np.arange(4000, dtype=np.uint32).reshape(1000, 4)
    keep = case.add(host, 1000, by_pointer=True)
    for (seed, draw), want in (((0, 0), [338, 269, 271, 480, 597, 433, 92, 207]), ((0, 1), [522, 286, 949, 176, 367, 247, 151, 218]),
                               ((1, 0), [432, 425, 539, 817, 168, 145, 763, 378]), ((2 ** 64 - 1, 2 ** 64 - 1), [730, 14, 3, 914, 472, 481, 675, 830])):
        got, slots = case.sample(8, seed=seed, draw=draw)
        assert slots.tolist() == want and (got[:, 0] == 4 * np.array(want)).all()
    del keep


@pytest.mark.parametrize("row_words", ROW_WORDS)
def test_given_slots_outside_the_ring_never_become_an_address(row_words):
    rng = np.random.default_rng(row_words + 1)
    Cn = 257
    case = RingCase(Cn, row_words)
    for size in (0, 1, 100, Cn):
        if size:
            case.add(_records(rng, size, row_words), size - case.ref.size, by_pointer=True)
        edge = [0, -1, size, I64_MIN, I64_MAX, size - 1, Cn, Cn - 1, -2 ** 31, 2 ** 31, 2 ** 32 + 1, 1]
        for n in (1, 63, 65, 1000):
            slot_in = (edge * (n // len(edge) + 1))[:n]
            slot_in[n // 2:] = rng.integers(-3, Cn + 3, n - n // 2).tolist()
            got, slots = case.sample(n, slot_in=slot_in, with_slots=bool(n % 2))
            ok = np.array([0 <= s < size for s in slot_in])
            assert (slots[ok] == np.array(slot_in, np.int64)[ok]).all() and (slots[~ok] == -1).all() and (got[~ok] == 0).all()
    case.check("the gathers changed neither ring nor state: ")


def _untouched(bufs, what):
    torch.cuda.synchronize()
    for name, whole in bufs.items():
        assert_poison(whole, f"{what}: {name}")


def test_every_refusal_leaves_the_outputs_untouched_and_a_good_call_fills_them():
    lib = _lib()
    rng = np.random.default_rng(9)
    Cn, row_words, n = 5, 12, 7
    case = RingCase(Cn, row_words)
    host = _records(rng, 9, row_words)
    src, cptr = _to_dev(host), torch.tensor([4], dtype=torch.int64, device=_dev())
    out, out_whole = fenced((n, row_words), torch.int32, _dev())
    oslot, oslot_whole = fenced((n,), torch.int64, _dev())
    sin = torch.zeros(n, dtype=torch.int64, device=_dev())
    R = 1024 // (row_words // 4)                                  # records per tile: the grid's limit is 2^31 - 1 tiles

    def state_zero(what):
        assert (case.state.cpu().numpy() == 0).all(), what
        assert_fences(case.state_whole, 4, what)

    def refused_add(what, **patch):
        io = case.add_io(src, count=4)
        for k, v in patch.items():
            setattr(io, k, v(getattr(io, k)) if callable(v) else v)
        assert lib.phx_replay_add(C.byref(io), _stream()) == EINVAL, what
        assert b"phx_replay_add" in lib.phx_last_error(), what
        _untouched({"ring": case.ring_whole}, "phx_replay_add, " + what)
        state_zero(what)

    def refused_sample(what, **patch):
        io = _abi.PhxReplaySampleIO(capacity=Cn, n=n, row_words=row_words, seed=1, draw=2, slot_in=sin.data_ptr(), ring=case.ring.data_ptr(),
                                    state=case.state.data_ptr(), out=out.data_ptr(), out_slot=oslot.data_ptr())
        for k, v in patch.items():
            setattr(io, k, v(getattr(io, k)) if callable(v) else v)
        assert lib.phx_replay_sample(C.byref(io), _stream()) == EINVAL, what
        assert b"phx_replay_sample" in lib.phx_last_error(), what
        _untouched({"out": out_whole, "out_slot": oslot_whole}, "phx_replay_sample, " + what)

    for k in ("src", "ring", "state"):
        refused_add(f"{k} NULL", **{k: None})
        refused_add(f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    refused_add("count_ptr off an 8-byte boundary", count_ptr=cptr.data_ptr() + 4)
    for k, bad in (("capacity", 0), ("capacity", -1), ("src_capacity", -1), ("row_words", 0), ("row_words", 2), ("row_words", 6), ("row_words", 258),
                   ("row_words", 260), ("row_words", -4), ("count", -1), ("count", 10), ("count", I64_MAX), ("reserved0", 1)):
        refused_add(f"{k} = {bad}", **{k: bad})
    refused_add("src_capacity beyond one launch's grid", src_capacity=R * (2 ** 31 - 1) + 1)
    refused_add("src_capacity beyond one launch's grid, the count on the device", src_capacity=I64_MAX, count_ptr=cptr.data_ptr())
    for k in ("ring", "state", "out"):
        refused_sample(f"{k} NULL", **{k: None})
    for k in ("ring", "state", "out", "out_slot"):
        refused_sample(f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    refused_sample("slot_in off an 8-byte boundary", slot_in=lambda p: p + 4)
    for k, bad in (("capacity", 0), ("capacity", -1), ("n", 0), ("n", -1), ("row_words", 0), ("row_words", 2), ("row_words", 6), ("row_words", 258),
                   ("row_words", 260), ("reserved0", 1), ("n", R * (2 ** 31 - 1) + 1), ("n", I64_MAX)):
        refused_sample(f"{k} = {bad}", **{k: bad})
    for r in (0, 1):
        io = case.add_io(src, count=4)
        io.reserved[r] = 1
        assert lib.phx_replay_add(C.byref(io), _stream()) == EINVAL and b"phx_replay_add" in lib.phx_last_error()
        io = _abi.PhxReplaySampleIO(capacity=Cn, n=n, row_words=row_words, ring=case.ring.data_ptr(), state=case.state.data_ptr(), out=out.data_ptr())
        io.reserved[r] = 1
        assert lib.phx_replay_sample(C.byref(io), _stream()) == EINVAL and b"phx_replay_sample" in lib.phx_last_error()
    _untouched({"ring": case.ring_whole, "out": out_whole, "out_slot": oslot_whole}, "a reserved field")
    state_zero("a reserved field")
    assert lib.phx_replay_add(None, None) == EINVAL and b"phx_replay_add" in lib.phx_last_error()
    assert lib.phx_replay_sample(None, None) == EINVAL and b"phx_replay_sample" in lib.phx_last_error()
    # and the same buffers receive good calls
    case.add(host, 4, by_pointer=False)
    case.check("after the refusals: ")
    got, slots = case.sample(n, seed=1, draw=2)
    assert ((slots >= 0) & (slots < 4)).all()
    empty = RingCase(3, 4)                                        # src_capacity == 0 needs no src
    io = empty.add_io(torch.zeros((0, 4), dtype=torch.int32, device=_dev()), count=0)
    assert io.src is None and lib.phx_replay_add(C.byref(io), _stream()) == 0, lib.phx_last_error()
    assert lib.phx_last_kernel() == b"phx_replay_add_kernel+phx_replay_commit_kernel"
    empty.check("an add of no records: ")
    assert_poison(empty.ring, "an add of no records")


# ---- the host surface ------------------------------------------------------------------------------------------------------------
T_E2E, B_E2E = 12, 8


def _plain_env(seed=5):
    env = supply_chain_env(5, [3] * 5, 8, B_E2E, seed=seed, exogenous="device")
    env.reset()
    return env


def _fsm_env(seed=5):
    env = supply_chain_env(5, [3] * 5, 8, B_E2E, fsm=True, seed=seed, exogenous="device")
    env.reset()
    return env


@pytest.mark.parametrize("make", [_plain_env, _fsm_env], ids=["plain", "fsm"])
@pytest.mark.parametrize("capacity", [37, 1000], ids=["below", "above"])
def test_sample_with_replay_keeps_the_batches_records(make, capacity):
    env, twin = make(), make()
    tb, tb_twin = ph.TrainBatcher(env, seed=3), ph.TrainBatcher(twin, seed=3)
    rb = ph.ReplayBuffer(env, capacity, seed=11)
    ref, total = None, 0
    for call in range(2):                                        # the second call wraps the small ring and half fills the large one
        got = env.sample(T_E2E, n_step=3, batcher=tb, replay=rb)
        assert env._device().last_kernel() == _abi.REPLAY_ADD_KERNELS
        want = twin.sample(T_E2E, n_step=3, batcher=tb_twin)
        assert set(got) == set(want) == {"default_policy"}
        db, dw = got["default_policy"], want["default_policy"]
        assert isinstance(db, DeviceBatch) and (make is _fsm_env) == (db._count is None)      # the FSM count is known on the device only
        K = dw.count
        assert db.count == K and db.layout == dw.layout and "nstep_rewards" in db.layout and 0 < K <= T_E2E * B_E2E * 5
        assert (capacity < K) == (capacity == 37)                # a ring below and a ring above the batch's count
        rec = db.records[:K].cpu().numpy()
        assert rec.tobytes() == dw.records[:K].cpu().numpy().tobytes()      # what the call returns without the keyword
        np.testing.assert_array_equal(db.row.cpu().numpy(), dw.row.cpu().numpy())
        if ref is None:
            ref = rr.Ring(capacity, rec.shape[1], fill=0)
        ref.add(rec.view(np.uint32), K)
        total += K
        ring = rb.ring.cpu().numpy().view(np.uint32)
        assert tuple(ring.shape) == (capacity, rec.shape[1]) and (ring == ref.ring).all()
        m = min(K, capacity)                                     # exactly the batch's last min(K, C) records, in order, up to the cursor
        assert (ring[(ref.cursor - m + np.arange(m)) % capacity] == rec[K - m:].view(np.uint32)).all()
        assert rb.state.cpu().numpy().tobytes() == ref.state().tobytes()
        assert (len(rb), rb.total, rb.refused) == (min(total, capacity), total, 0)
        mb = rb.sample(64)
        assert env._device().last_kernel() == _abi.REPLAY_SAMPLE_KERNEL
        assert isinstance(mb, DeviceBatch) and mb.count == 64 and mb.epoch == 2 * call and mb.row is None and mb.col is None and mb.layout == rb.layout
        slots = mb.slots.cpu().numpy()
        assert slots.tolist() == rr.draws(11, 2 * call, len(rb), 64)
        held = DeviceBatch(rb.ring, rb.layout, None, count=capacity).columns
        again = rb.gather(mb.slots)
        assert again.epoch == 2 * call + 1 and (again.slots.cpu().numpy() == slots).all()
        for name, x in mb.columns.items():
            w = held[name][mb.slots].cpu().numpy()
            g = x.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
            assert again.columns[name].cpu().numpy().tobytes() == g.tobytes(), name
        assert set(mb.columns) == set(db.columns)


def test_one_buffer_per_policy():
    env = _plain_env()
    ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
    fn = lambda aid: "even" if ids.index(aid) % 2 == 0 else "odd"
    tb = ph.TrainBatcher(env, policy_mapping_fn=fn)
    rbs = {"odd": ph.ReplayBuffer(env, 64), "even": ph.ReplayBuffer(env, 4096)}
    got = ph.rllib.BatchedBaseEnv(env).sample(T_E2E, n_step=3, batcher=tb, replay=rbs)       # the RLlib adapter passes the keyword through
    for pid, rb in rbs.items():
        K = got[pid].count
        assert K == T_E2E * B_E2E * (3 if pid == "even" else 2) and (len(rb), rb.total) == (min(K, rb.capacity), K)
        m = min(K, rb.capacity)
        ring, rec = rb.ring.cpu().numpy(), got[pid].records[:K].cpu().numpy()
        assert (ring[(K - m + np.arange(m)) % rb.capacity] == rec[K - m:]).all()
    with pytest.raises(ValueError, match="policy ids"):
        env.sample(T_E2E, batcher=tb, replay=rbs["odd"])
    with pytest.raises(ValueError, match="batcher"):
        env.sample(T_E2E, replay=rbs["odd"])


def test_device_env_replay_calls_check_their_arguments_before_any_launch():
    env = _plain_env()
    dev = env._device()
    d = dev.device
    ring, ring_whole = fenced((6, 8), torch.int32, d)
    state, state_whole = fenced((4,), torch.int64, d)
    state.zero_()
    out, out_whole = fenced((5, 8), torch.int32, d)
    oslot, oslot_whole = fenced((5,), torch.int64, d)
    rec = torch.arange(32, dtype=torch.int32, device=d).reshape(4, 8)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=d)
    for match, kw in (("ring", dict(ring=ring.float())), ("ring", dict(ring=ring.cpu())), ("ring", dict(ring=ring[:, :6])), ("ring", dict(ring=ring[0])),
                      ("ring", dict(ring=None)), ("state", dict(state=state[:3])), ("state", dict(state=state.int())), ("state", dict(state=None)),
                      ("records", dict(records=rec[:, :4])), ("records", dict(records=rec.float())), ("records", dict(records=None)),
                      ("count", dict(count=5)), ("count", dict(count=-1)), ("count", dict(count=True)), ("count", dict(count=2.0)),
                      ("count", dict(count=i64(1, 2))), ("count", dict(count=i64(1).int())), ("count", dict(count=i64(1).cpu()))):
        with pytest.raises(ValueError, match=match):
            dev.replay_add(**dict(dict(ring=ring, state=state, records=rec), **kw))
    for match, kw in (("ring", dict(ring=ring.float())), ("state", dict(state=state[:3])), (r"n = ", dict(n=0)), (r"n = ", dict(n=2.5)), (r"n = ", dict(n=True)),
                      ("seed", dict(seed=-1)), ("draw", dict(draw=2 ** 64)), ("slots", dict(slots=i64(1, 2))), ("slots", dict(slots=i64(*range(5)).int())),
                      (r"out\[0\]", dict(out=(out[:4], oslot))), (r"out\[1\]", dict(out=(out, oslot.int()))), ("out", dict(out=(out,)))):
        with pytest.raises(ValueError, match=match):
            dev.replay_sample(**dict(dict(ring=ring, state=state, n=5, out=(out, oslot)), **kw))
    _untouched({"ring": ring_whole, "out": out_whole, "out_slot": oslot_whole}, "a refused DeviceEnv.replay_add / replay_sample call")
    assert (state.cpu().numpy() == 0).all()
    dev.replay_add(ring, state, rec, count=i64(3))
    assert dev.last_kernel() == _abi.REPLAY_ADD_KERNELS
    dev.replay_add(ring, state, rec)                              # count=None: all four
    dev.replay_add(ring, state, rec, count=2)
    want = rr.Ring(6, 8, fill=POISON_WORD)
    for K in (3, 4, 2):
        want.add(rec.cpu().numpy().view(np.uint32), K)
    assert (ring.cpu().numpy().view(np.uint32) == want.ring).all() and state.cpu().numpy().tobytes() == want.state().tobytes()
    res = dev.replay_sample(ring, state, 5, seed=4, draw=1, out=(out, None))
    assert dev.last_kernel() == _abi.REPLAY_SAMPLE_KERNEL and res[0].data_ptr() == out.data_ptr() and res[1] is None
    assert (out.cpu().numpy().view(np.uint32) == want.sample(5, 4, 1)[0]).all()
    _untouched({"out_slot": oslot_whole}, "out_slot was not given")
    got, slots = dev.replay_sample(ring, state, 5, slots=i64(5, 0, 6, -1, 2))
    assert slots.tolist() == [5, 0, -1, -1, 2] and (got.cpu().numpy().view(np.uint32) == want.sample(5, slot_in=[5, 0, 6, -1, 2])[0]).all()
    for whole, rows in ((ring_whole, 6), (state_whole, 4), (out_whole, 5)):
        assert_fences(whole, rows, "DeviceEnv.replay_*")
