"""phx_prio_add / phx_prio_update / phx_prio_sample (include/phantom_amd_prio.h) on the GPU, through the C ABI into fenced buffers:
bit-equality with the numpy restatement (tests/prio_ref.py) of the whole tree buffer and its state after every call -- rings at the
level edges and with padding, add sequences that wrap with the count by value and by pointer, refused counts, updates with duplicates,
unusable priorities and slots outside the ring -- and of every drawn slot and priority, the header's known answers and the "no k"
fallback; calls queued without a wait; every refusal; then PrioritizedReplayBuffer behind sample(batcher=..., replay=...) on a plain
and an FSM supply chain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prio_ref as pr
import replay_ref as rr
import phantom_amd as ph
from fenced import assert_fences, assert_poison, assert_written, fenced
from helpers import supply_chain_env
from phantom_amd import _abi
from phantom_amd.rollout import DeviceBatch
from prio_ref import BAD_PRIORITIES, FALLBACK_DRAWS, KNOWN

pytestmark = pytest.mark.gpu
EINVAL = -1
I64_MIN, I64_MAX = pr.I64_MIN, pr.I64_MAX
RINGS = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65537)
UPDATE_NS = (1, 63, 64, 65, 257, 5000)
SAMPLE_NS = (1, 255, 256, 257, 5000)
ROW_WORDS = 4


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    return _abi.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class TreeCase:
    """a fenced, zero-filled tree buffer and state next to a real ring of 4-word records (its state is the one the calls read), and
    the restatement beside them"""

    def __init__(self, Cn):
        self.C = Cn
        self.words = _abi.prio_layout(Cn)[3]
        self.tree, self.tree_whole = fenced((self.words,), torch.float32, _dev())
        self.pstate, self.pstate_whole = fenced((32,), torch.uint8, _dev())
        self.tree.zero_()
        self.pstate.zero_()
        self.ring = torch.zeros((Cn, ROW_WORDS), dtype=torch.int32, device=_dev())
        self.rstate = torch.zeros(4, dtype=torch.int64, device=_dev())
        self.src = torch.zeros((3 * Cn + 2, ROW_WORDS), dtype=torch.int32, device=_dev())
        self.ref = pr.Tree(Cn)
        self.cursor = self.size = 0
        self.alive = []                                            # what queued calls read

    def add_io(self, count=None, count_ptr=None, src_capacity=None):
        return _abi.PhxPrioAddIO(capacity=self.C, src_capacity=self.src.shape[0] if src_capacity is None else src_capacity,
                                 count=0 if count is None else count, count_ptr=None if count_ptr is None else count_ptr.data_ptr(),
                                 ring_state=self.rstate.data_ptr(), tree=self.tree.data_ptr(), state=self.pstate.data_ptr())

    def add(self, K, by_pointer, src_capacity=None):
        """phx_prio_add and then the ring's own add of the same count, as a caller orders them"""
        cap = self.src.shape[0] if src_capacity is None else src_capacity
        ptr = torch.tensor([K], dtype=torch.int64, device=_dev()) if by_pointer else None
        self.alive.append(ptr)
        io = self.add_io(None if by_pointer else K, ptr, cap)
        assert _lib().phx_prio_add(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        assert _lib().phx_last_kernel() == _abi.prio_kernels(_abi.PRIO_ADD_KERNELS, self.C).encode()
        rio = _abi.PhxReplayAddIO(capacity=self.C, src_capacity=cap, count=0 if by_pointer else K, row_words=ROW_WORDS,
                                  count_ptr=None if ptr is None else ptr.data_ptr(), src=self.src.data_ptr() if cap else None,
                                  ring=self.ring.data_ptr(), state=self.rstate.data_ptr())
        assert _lib().phx_replay_add(C.byref(rio), _stream()) == 0, _lib().phx_last_error()
        self.ref.add(K, cap, self.cursor)
        if 0 <= K <= cap:
            self.cursor, self.size = (self.cursor + K) % self.C, min(self.C, self.size + K)

    def update(self, slots, prios):
        s = torch.tensor(slots, dtype=torch.int64, device=_dev())
        p = torch.tensor(np.asarray(prios, np.float32), device=_dev())
        self.alive.append((s, p))
        io = _abi.PhxPrioUpdateIO(capacity=self.C, n=len(slots), slot_in=s.data_ptr(), priority=p.data_ptr(), ring_state=self.rstate.data_ptr(),
                                  tree=self.tree.data_ptr(), state=self.pstate.data_ptr())
        assert _lib().phx_prio_update(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        assert _lib().phx_last_kernel() == _abi.prio_kernels(_abi.PRIO_UPDATE_KERNELS, self.C).encode()
        self.ref.update(slots, np.asarray(prios, np.float32), self.size)

    def check(self, what):
        assert_fences(self.tree_whole, self.words, what + "tree")
        assert_fences(self.pstate_whole, 32, what + "state")
        got = self.tree.cpu().numpy()
        bad = np.flatnonzero(got.view(np.uint32) != self.ref.buf.view(np.uint32))
        assert bad.size == 0, f"{what}tree: {bad.size} of {self.words} words differ, first at {bad[:5]}: {got[bad[:5]]} != {self.ref.buf[bad[:5]]}"
        st = self.pstate.cpu().numpy().tobytes()
        assert st == self.ref.state().tobytes(), f"{what}state: {np.frombuffer(st, pr.STATE_DTYPE)} != {self.ref.state()}"
        assert self.rstate.tolist()[:2] == [self.cursor, self.size], what

    def sample_queued(self, n, seed=0, draw=0):
        """one phx_prio_sample into fenced outputs and what the restatement draws now; ``sample_check`` compares after a sync"""
        oslot, oslot_whole = fenced((n,), torch.int64, _dev())
        oprio, oprio_whole = fenced((n,), torch.float32, _dev())
        io = _abi.PhxPrioSampleIO(capacity=self.C, n=n, seed=seed, draw=draw, ring_state=self.rstate.data_ptr(), tree=self.tree.data_ptr(),
                                  out_slot=oslot.data_ptr(), out_priority=oprio.data_ptr())
        assert _lib().phx_prio_sample(C.byref(io), _stream()) == 0, _lib().phx_last_error()
        assert _lib().phx_last_kernel() == _abi.PRIO_SAMPLE_KERNEL.encode()
        want = self.ref.sample(n, seed, draw, self.size)
        return (oslot, oslot_whole, oprio, oprio_whole, want, f"C={self.C} size={self.size} n={n} seed={seed} draw={draw}: ")

    @staticmethod
    def sample_check(queued):
        oslot, oslot_whole, oprio, oprio_whole, (want_s, want_p), what = queued
        n = want_s.size
        assert_fences(oslot_whole, n, what + "out_slot")
        assert_fences(oprio_whole, n, what + "out_priority")
        assert_written(oslot, what + "out_slot")
        assert_written(oprio, what + "out_priority")
        np.testing.assert_array_equal(oslot.cpu().numpy(), want_s, err_msg=what + "out_slot")
        got = oprio.cpu().numpy()
        assert got.tobytes() == want_p.tobytes(), f"{what}out_priority: {np.flatnonzero(got.view(np.uint32) != want_p.view(np.uint32))[:5]}"
        return want_s, want_p

    def sample(self, n, seed=0, draw=0):
        return self.sample_check(self.sample_queued(n, seed, draw))


def _update_lists(rng, Cn, size, n, kind):
    """slots and priorities of one update: random with duplicates, edges and unusable priorities; one slot n times; or none valid"""
    if kind == "invalid":
        slots = ([-1, size, I64_MIN, I64_MAX, Cn, -2 ** 31, 2 ** 32 + size] * (n // 7 + 1))[:n]
        return slots, [1.0] * n
    if kind == "duplicate":
        return [max(size - 1, 0)] * n, (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32).tolist()
    slots = rng.integers(-2, Cn + 2, n).tolist()
    prios = (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32).tolist()
    for i, s in enumerate((-1, size, I64_MIN, I64_MAX, 0, 0, size - 1)):
        if i < n:
            slots[n - 1 - i] = s
    for i, bad in enumerate(BAD_PRIORITIES):
        if i + 8 < n:
            prios[i + 8] = bad
    return slots, prios


@pytest.mark.parametrize("Cn", RINGS)
def test_tree_and_state_are_bit_equal_to_the_restatement(Cn):
    """add sequences that wrap (every count by value and by pointer, refused counts by pointer), an update after each add; the whole
    buffer and the state are read back after every call"""
    rng = np.random.default_rng(Cn)
    case = TreeCase(Cn)
    cap = 3 * Cn + 2
    counts = [0, 1, Cn - 1, Cn, Cn + 1, cap, cap + 1, -1, 1, Cn - 1, 2, Cn + 1, 0, cap, 1, I64_MAX, I64_MIN]
    kinds = ("random", "duplicate", "invalid")
    refused = 0
    for step, K in enumerate(counts):
        outside = K < 0 or K > cap
        by_pointer = outside or bool(step % 2)
        case.add(K, by_pointer)
        case.check(f"C={Cn} add {step} (K={K}, {'pointer' if by_pointer else 'value'}): ")
        refused += outside
        assert case.ref.refused == refused
        n = UPDATE_NS[step % len(UPDATE_NS)]
        slots, prios = _update_lists(rng, Cn, case.size, n, kinds[(step // 2) % 3])
        case.update(slots, prios)
        case.check(f"C={Cn} update {step} (n={n}, {kinds[(step // 2) % 3]}): ")
    for K, by_pointer in ((Cn, False), (Cn, True), (0, True), (1, False)):      # the counts of the other calling form
        case.add(K, by_pointer)
        case.check(f"C={Cn} add K={K}: ")
    assert case.size == Cn and case.ref.ignored > 0
    s, p = case.sample(257, seed=Cn, draw=1)
    assert ((s >= 0) & (s < Cn)).all() and (p > 0).all()


def test_six_levels():
    """C = 2^20 + 1: six levels, three of them served by per-level launches; a wrap-around add of more than C records"""
    Cn = 2 ** 20 + 1
    rng = np.random.default_rng(20)
    case = TreeCase(Cn)
    assert case.ref.L == 6
    for step, (K, by_pointer) in enumerate(((5, False), (Cn - 7, True), (4099, False), (3 * Cn + 2, True), (70000, False))):
        case.add(K, by_pointer)
        case.check(f"C=2^20+1 add {step} (K={K}): ")
        slots, prios = _update_lists(rng, Cn, case.size, (5000, 257, 65, 5000, 1)[step], ("random", "duplicate", "random", "random", "invalid")[step])
        case.update(slots, prios)
        case.check(f"C=2^20+1 update {step}: ")
    s, p = case.sample(5000, seed=3, draw=4)
    assert ((s >= 0) & (s < Cn)).all() and (p > 0).all() and len(set(s.tolist())) > 1000


@pytest.mark.parametrize("Cn", (1, 17, 300, 4097, 65537))
def test_sample_is_bit_equal_to_the_restatement(Cn):
    rng = np.random.default_rng(Cn + 1)
    case = TreeCase(Cn)
    for i, n in enumerate(SAMPLE_NS):                              # an empty tree
        s, p = case.sample(n, seed=n, draw=i)
        assert (s == -1).all() and p.tobytes() == bytes(4 * n)
    for fill in (1, Cn):
        case.add(fill - case.size, by_pointer=True)
        m = min(case.size, 3000)
        case.update(rng.integers(0, case.size, m).tolist(), (10.0 ** rng.uniform(-4, 4, m)).astype(np.float32))
        for i, n in enumerate(SAMPLE_NS):
            s, p = case.sample(n, seed=0xDEADBEEF12345678 + n, draw=fill + i)
            assert ((s >= 0) & (s < case.size)).all() and (p > 0).all()
        case.sample(64, seed=2 ** 64 - 1, draw=2 ** 64 - 1)
    case.update([Cn - 1], [2.0 ** 40])                             # nearly all of the mass in the last slot
    s, p = case.sample(257, seed=5)
    assert (s == Cn - 1).mean() > 0.9
    case.check("the samples changed neither tree nor state: ")


def test_the_known_answers_and_the_fallback_on_the_device():
    case = TreeCase(37)
    case.add(37, by_pointer=True)
    case.update(list(range(37)), [1 + s % 7 for s in range(37)])
    for (seed, draw), (slots, prios) in KNOWN.items():
        s, p = case.sample(8, seed=seed, draw=draw)
        assert s.tolist() == slots and p.tolist() == prios
    s, p = case.sample(7000, seed=0, draw=0)
    assert len(set(s.tolist())) == 37
    prop = TreeCase(7)                                             # the CPU test's proportionality counts
    prop.add(7, by_pointer=False)
    prop.update(list(range(7)), [1, 2, 3, 4, 5, 6, 7])
    s, p = prop.sample(7000, seed=0, draw=0)
    assert np.bincount(s, minlength=7).tolist() == [247, 501, 745, 1002, 1294, 1481, 1730]
    fb = TreeCase(32)                                              # test_prio_cpu.fallback_tree
    fb.add(32, by_pointer=False)
    fb.update(list(range(32)), [3.0] + [0.0] * 15 + [2.0 ** 24 + 4] + [0.0] * 15)
    fb.check("the fallback tree: ")
    for seed, draw in FALLBACK_DRAWS:
        s, p = fb.sample(4, seed=seed, draw=draw)
        assert s[0] == 31 and p[0] == np.float32(2.0 ** -40)
    one = TreeCase(300)                                            # one non-zero leaf, in the last slot held
    one.add(300, by_pointer=True)
    one.check("")
    assert (one.sample(300, seed=9)[1] == 1).all()


def test_calls_queued_without_a_wait():
    rng = np.random.default_rng(6)
    for Cn in (257, 4097):
        case = TreeCase(Cn)
        case.add(Cn - 5, by_pointer=True)
        case.update(*_update_lists(rng, Cn, case.size, 257, "random"))
        q1 = case.sample_queued(257, seed=1, draw=0)
        case.add(40, by_pointer=False)                             # wraps
        case.update(*_update_lists(rng, Cn, case.size, 5000, "random"))
        q2 = case.sample_queued(5000, seed=1, draw=1)
        torch.cuda.synchronize()                                   # the one wait
        case.check(f"C={Cn} six calls back to back: ")
        case.sample_check(q1)
        case.sample_check(q2)


def _untouched(bufs, what):
    torch.cuda.synchronize()
    for name, whole in bufs.items():
        assert_poison(whole, f"{what}: {name}")


def test_every_refusal_leaves_tree_state_and_outputs_untouched_and_a_good_call_fills_them():
    lib = _lib()
    Cn, n = 300, 7
    words = _abi.prio_layout(Cn)[3]
    tree, tree_whole = fenced((words,), torch.float32, _dev())     # poisoned, not zero-filled: a launch would show
    pstate, pstate_whole = fenced((32,), torch.uint8, _dev())
    oslot, oslot_whole = fenced((n,), torch.int64, _dev())
    oprio, oprio_whole = fenced((n,), torch.float32, _dev())
    rstate = torch.tensor([0, 5, 5, 0], dtype=torch.int64, device=_dev())
    cptr = torch.tensor([4], dtype=torch.int64, device=_dev())
    sin, prio = torch.zeros(n, dtype=torch.int64, device=_dev()), torch.ones(n + 1, dtype=torch.float32, device=_dev())
    bufs = {"tree": tree_whole, "state": pstate_whole, "out_slot": oslot_whole, "out_priority": oprio_whole}
    make = {"phx_prio_add": lambda: _abi.PhxPrioAddIO(capacity=Cn, src_capacity=9, count=4, ring_state=rstate.data_ptr(), tree=tree.data_ptr(),
                                                      state=pstate.data_ptr()),
            "phx_prio_update": lambda: _abi.PhxPrioUpdateIO(capacity=Cn, n=n, slot_in=sin.data_ptr(), priority=prio.data_ptr(), ring_state=rstate.data_ptr(),
                                                            tree=tree.data_ptr(), state=pstate.data_ptr()),
            "phx_prio_sample": lambda: _abi.PhxPrioSampleIO(capacity=Cn, n=n, seed=1, draw=2, ring_state=rstate.data_ptr(), tree=tree.data_ptr(),
                                                            out_slot=oslot.data_ptr(), out_priority=oprio.data_ptr())}

    def refused(fn, what, **patch):
        io = make[fn]()
        for k, v in patch.items():
            setattr(io, k, v(getattr(io, k)) if callable(v) else v)
        assert getattr(lib, fn)(C.byref(io), _stream()) == EINVAL, f"{fn}, {what}"
        assert fn.encode() in lib.phx_last_error(), f"{fn}, {what}"
        _untouched(bufs, f"{fn}, {what}")

    for fn in make:
        for k in ("ring_state", "tree"):
            refused(fn, f"{k} NULL", **{k: None})
        refused(fn, "tree off a 16-byte boundary", tree=lambda p: p + 8)
        refused(fn, "ring_state off an 8-byte boundary", ring_state=lambda p: p + 4)
        for bad in (0, -1, 2 ** 30 + 1, I64_MAX):
            refused(fn, f"capacity = {bad}", capacity=bad)
        for r in (0, 1):
            io = make[fn]()
            io.reserved[r] = 1
            assert getattr(lib, fn)(C.byref(io), _stream()) == EINVAL and fn.encode() in lib.phx_last_error()
            _untouched(bufs, f"{fn}, reserved[{r}]")
        assert getattr(lib, fn)(None, None) == EINVAL and fn.encode() in lib.phx_last_error()
    for fn in ("phx_prio_add", "phx_prio_update"):
        refused(fn, "state NULL", state=None)
        refused(fn, "state off a 16-byte boundary", state=lambda p: p + 8)
    refused("phx_prio_add", "count_ptr off an 8-byte boundary", count_ptr=cptr.data_ptr() + 4)
    for k, bad in (("src_capacity", -1), ("count", -1), ("count", 10), ("count", I64_MAX)):
        refused("phx_prio_add", f"{k} = {bad}", **{k: bad})
    for fn in ("phx_prio_update", "phx_prio_sample"):
        for bad in (0, -1, 256 * (2 ** 31 - 1) + 1, I64_MAX):
            refused(fn, f"n = {bad}", n=bad)
    for k in ("slot_in", "priority"):
        refused("phx_prio_update", f"{k} NULL", **{k: None})
    refused("phx_prio_update", "slot_in off an 8-byte boundary", slot_in=lambda p: p + 4)
    refused("phx_prio_update", "priority off a 4-byte boundary", priority=lambda p: p + 2)
    for k in ("out_slot", "out_priority"):
        refused("phx_prio_sample", f"{k} NULL", **{k: None})
        refused("phx_prio_sample", f"{k} off a 16-byte boundary", **{k: lambda p: p + 8})
    # and the same buffers receive good calls: a priority 4 bytes into its buffer is allowed
    tree.zero_()
    pstate.zero_()
    ref = pr.Tree(Cn)
    assert lib.phx_prio_add(C.byref(make["phx_prio_add"]()), _stream()) == 0, lib.phx_last_error()
    ref.add(4, 9, 0)
    io = make["phx_prio_update"]()
    io.priority += 4
    assert lib.phx_prio_update(C.byref(io), _stream()) == 0, lib.phx_last_error()
    ref.update([0] * n, [1.0] * n, 5)
    assert lib.phx_prio_sample(C.byref(make["phx_prio_sample"]()), _stream()) == 0, lib.phx_last_error()
    want_s, want_p = ref.sample(n, 1, 2, 5)
    assert oslot.tolist() == want_s.tolist() and oprio.cpu().numpy().tobytes() == want_p.tobytes()
    assert tree.cpu().numpy().tobytes() == ref.buf.tobytes() and pstate.cpu().numpy().tobytes() == ref.state().tobytes()
    for whole, rows in ((tree_whole, words), (pstate_whole, 32), (oslot_whole, n), (oprio_whole, n)):
        assert_fences(whole, rows, "after the good calls")
    empty = _abi.PhxPrioAddIO(capacity=Cn, src_capacity=0, count=0, ring_state=rstate.data_ptr(), tree=tree.data_ptr(), state=pstate.data_ptr())
    assert lib.phx_prio_add(C.byref(empty), _stream()) == 0, lib.phx_last_error()      # an add of no records
    assert tree.cpu().numpy().tobytes() == ref.buf.tobytes() and pstate.cpu().numpy().tobytes() == ref.state().tobytes()


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
def test_sample_with_a_prioritized_buffer(make, capacity):
    env, twin = make(), make()
    tb, tb_twin = ph.TrainBatcher(env, seed=3), ph.TrainBatcher(twin, seed=3)
    prb = ph.PrioritizedReplayBuffer(env, capacity, alpha=0.5, eps=0.01, seed=11)
    rb = ph.ReplayBuffer(twin, capacity, seed=11)
    ref, cursor, size, beta = pr.Tree(capacity), 0, 0, 0.7
    for call in range(2):                                        # the second call wraps the small ring and half fills the large one
        got = env.sample(T_E2E, n_step=3, batcher=tb, replay=prb)
        assert env._device().last_kernel() == _abi.REPLAY_ADD_KERNELS          # prio_add came first, the ring's add last
        want = twin.sample(T_E2E, n_step=3, batcher=tb_twin, replay=rb)
        db, dw = got["default_policy"], want["default_policy"]
        K = dw.count
        assert isinstance(db, DeviceBatch) and db.count == K and 0 < K <= db.records.shape[0]
        assert db.records[:K].cpu().numpy().tobytes() == dw.records[:K].cpu().numpy().tobytes()
        # the records the uniform buffer would hold, and its state
        assert prb.ring.cpu().numpy().tobytes() == rb.ring.cpu().numpy().tobytes()
        assert prb.state.cpu().numpy().tobytes() == rb.state.cpu().numpy().tobytes()
        assert (len(prb), prb.total, prb.refused) == (len(rb), rb.total, 0)
        ref.add(K, int(db.records.shape[0]), cursor)
        cursor, size = (cursor + K) % capacity, min(capacity, size + K)
        assert prb.tree.cpu().numpy().tobytes() == ref.buf.tobytes() and prb.pstate.cpu().numpy().tobytes() == ref.state().tobytes()
        assert len(prb) == size
        for again in range(2):                                   # sample, update, and a second sample that sees the update
            mb = prb.sample(64, beta)
            assert env._device().last_kernel() == _abi.REPLAY_SAMPLE_KERNEL
            d = 2 * call + again
            want_s, want_p = ref.sample(64, 11, d, size)
            assert isinstance(mb, DeviceBatch) and mb.count == 64 and mb.epoch == d and mb.layout == prb.layout
            slots = mb.slots.cpu().numpy()
            assert slots.tolist() == want_s.tolist() and mb.priorities.cpu().numpy().tobytes() == want_p.tobytes()
            assert ((slots >= 0) & (slots < size)).all()
            assert (mb.records.cpu().numpy() == prb.ring.cpu().numpy()[slots]).all()      # the ring's rows at .slots
            held = DeviceBatch(prb.ring, prb.layout, None, count=capacity).columns
            for name, x in mb.columns.items():
                assert x.cpu().numpy().tobytes() == held[name][mb.slots].cpu().numpy().tobytes(), name
            np.testing.assert_allclose(mb.weights.cpu().numpy(), (float(ref.pmin()) / want_p.astype(np.float64)) ** beta, rtol=1e-5)
            if again == 0:
                td = mb.columns["nstep_rewards"].abs() + (mb.slots % 5).float()
                prb.update_priorities(mb.slots, td)
                assert env._device().last_kernel() == _abi.prio_kernels(_abi.PRIO_UPDATE_KERNELS, capacity)
                ref.update(slots.tolist(), ((td + 0.01) ** 0.5).cpu().numpy(), size)
                assert prb.tree.cpu().numpy().tobytes() == ref.buf.tobytes() and prb.pstate.cpu().numpy().tobytes() == ref.state().tobytes()
    assert prb.ignored == 0
    prb.update_priorities(torch.tensor([-1, capacity, 0], dtype=torch.int64, device=prb.ring.device), torch.ones(3, device=prb.ring.device))
    assert prb.ignored == 2


def test_device_env_prio_calls_check_their_arguments_before_any_launch():
    env = _plain_env()
    dev = env._device()
    d = dev.device
    Cn = 300
    words = _abi.prio_layout(Cn)[3]
    tree, tree_whole = fenced((words,), torch.float32, d)
    pstate, pstate_whole = fenced((32,), torch.uint8, d)
    oslot, oslot_whole = fenced((5,), torch.int64, d)
    oprio, oprio_whole = fenced((5,), torch.float32, d)
    rstate = torch.zeros(4, dtype=torch.int64, device=d)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=d)
    base = dict(tree=tree, pstate=pstate, ring_state=rstate, capacity=Cn)
    for fn, kw, bads in (("prio_add", dict(src_capacity=9), (("tree", dict(tree=tree[:-1])), ("tree", dict(tree=tree.cpu())), ("pstate", dict(pstate=None)),
                                                             ("ring_state", dict(ring_state=rstate.int())), ("capacity", dict(capacity=0)),
                                                             ("count", dict(count=10)), ("count", dict(count=i64(1).cpu())), ("src_capacity", dict(src_capacity=-1)))),
                         ("prio_update", dict(slots=i64(0, 1), priorities=torch.ones(2, device=d)),
                          (("tree", dict(capacity=Cn + 16)), ("slots", dict(slots=i64(0, 1).int())), ("priorities", dict(priorities=torch.ones(3, device=d))),
                           ("priorities", dict(priorities=torch.ones(2, device=d).double())))),
                         ("prio_sample", dict(n=5, out=(oslot, oprio)), ((r"n = ", dict(n=0)), ("seed", dict(seed=-1)), (r"out\[0\]", dict(out=(oslot[:4], oprio))),
                                                                         (r"out\[1\]", dict(out=(oslot, oprio.double()))), ("tree", dict(tree=tree.double()))))):
        for match, patch in bads:
            with pytest.raises(ValueError, match=match):
                getattr(dev, fn)(**dict(dict(base, **kw), **patch))
    _untouched({"tree": tree_whole, "state": pstate_whole, "out_slot": oslot_whole, "out_priority": oprio_whole}, "a refused DeviceEnv.prio_* call")
    tree.zero_()
    pstate.zero_()
    ref = pr.Tree(Cn)
    ring = torch.zeros((Cn, 4), dtype=torch.int32, device=d)
    rec = torch.zeros((9, 4), dtype=torch.int32, device=d)
    cursor = 0
    for count, K in ((i64(3), 3), (None, 9), (2, 2)):
        dev.prio_add(tree, pstate, rstate, Cn, 9, count=count)
        assert dev.last_kernel() == _abi.prio_kernels(_abi.PRIO_ADD_KERNELS, Cn)
        dev.replay_add(ring, rstate, rec, count=count)
        ref.add(K, 9, cursor)
        cursor += K
    dev.prio_update(tree, pstate, rstate, Cn, i64(13, 0, 14, -1, 13), torch.tensor([2.0, 0.5, 1.0, 1.0, 3.0], device=d))
    assert dev.last_kernel() == _abi.prio_kernels(_abi.PRIO_UPDATE_KERNELS, Cn)
    ref.update([13, 0, 14, -1, 13], [2.0, 0.5, 1.0, 1.0, 3.0], 14)
    res = dev.prio_sample(tree, pstate, rstate, Cn, 5, seed=4, draw=1, out=(oslot, oprio))
    assert dev.last_kernel() == _abi.PRIO_SAMPLE_KERNEL and res[0].data_ptr() == oslot.data_ptr() and res[1].data_ptr() == oprio.data_ptr()
    want_s, want_p = ref.sample(5, 4, 1, 14)
    assert oslot.tolist() == want_s.tolist() and oprio.cpu().numpy().tobytes() == want_p.tobytes()
    s, p = dev.prio_sample(tree, pstate, rstate, Cn, 64)
    assert s.tolist() == ref.sample(64, 0, 0, 14)[0].tolist()
    assert tree.cpu().numpy().tobytes() == ref.buf.tobytes() and pstate.cpu().numpy().tobytes() == ref.state().tobytes()
    for whole, rows in ((tree_whole, words), (pstate_whole, 32), (oslot_whole, 5), (oprio_whole, 5)):
        assert_fences(whole, rows, "DeviceEnv.prio_*")
