"""A replay learner's buffer on the device: ``ReplayBuffer`` keeps the records of ``DeviceBatch``es in a ring (one
``DeviceEnv.replay_add`` call per batch, the count taken from device memory) and draws minibatches from it uniformly with replacement
(one ``DeviceEnv.replay_sample`` call each) -- include/phantom_amd_replay.h.  Nothing is copied to the host and no call waits."""
import numpy as np

from . import _abi
from .batch import DeviceBatch, DeviceSeqBatch


class ReplayBuffer:
    """``rb = ReplayBuffer(env, capacity)``; ``env.sample(T, n_step=n, batcher=tb, replay=rb)`` appends every fragment's records, or
    ``rb.add(batch)`` does; ``rb.sample(n)`` gives a ``DeviceBatch`` of n records drawn uniformly with replacement, as RLlib's
    ``ReplayBuffer.sample`` draws.

    The first ``add`` fixes the record width and the column layout and allocates the ring, i32 ``[capacity, row_words]``, and its
    32-byte state on the batch's device; once ``capacity`` records are held the oldest are overwritten.  Draw number d (``draws``,
    counted from 0) is the stream ``(seed, d)`` of the header: reproducible, and different for every call.  ``len(rb)`` (the records
    held), ``rb.total`` (ever accepted) and ``rb.refused`` (batches that held no records because their count exceeded their buffer)
    read the state's 32 bytes once, when asked, and again only after a further ``add``.

    Out of scope here as in the header: sampling without replacement, sequence batches, spilling to the host, more than one GPU.
    Prioritized sampling is ``PrioritizedReplayBuffer`` (include/phantom_amd_prio.h), built on ``gather(slots)``."""

    def __init__(self, env, capacity: int, seed: int = 0):
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise ValueError(f"ReplayBuffer: capacity = {capacity!r} must be an int >= 1")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"ReplayBuffer: seed = {seed!r} must be an int in [0, 2^64)")
        self.env, self.capacity, self.seed, self.draws = env, int(capacity), int(seed), 0
        self.ring = self.state = self.layout = self.row_words = self.dev = None
        self._host_state = None

    def _accept(self, batch):
        """``add``'s checks and, the first time, its allocations: the batch's count, a host int or a device i64 [1] tensor"""
        import torch
        if isinstance(batch, DeviceSeqBatch):
            raise ValueError("ReplayBuffer.add: a sequence batch (DeviceSeqBatch) is out of scope; build the batcher without max_seq_len")
        if not isinstance(batch, DeviceBatch):
            raise ValueError(f"ReplayBuffer.add: a DeviceBatch is expected, got {type(batch).__name__}")
        records = batch.records
        if records.dim() != 2:
            raise ValueError(f"ReplayBuffer.add: records of shape {tuple(records.shape)}, expected [capacity, row_words]")
        if self.ring is None:
            self.row_words, self.layout = int(records.shape[1]), dict(batch.layout)
            self.dev = batch.dev if batch.dev is not None else self.env._device()      # (a hand-made batch names no DeviceEnv)
            self.ring = torch.zeros((self.capacity, self.row_words), dtype=records.dtype, device=records.device)
            self.state = torch.zeros(4, dtype=torch.int64, device=records.device)
        elif int(records.shape[1]) != self.row_words or dict(batch.layout) != self.layout:
            raise ValueError(f"ReplayBuffer.add: the batch's layout {dict(batch.layout)} ({int(records.shape[1])} words) is not the ring's "
                             f"{self.layout} ({self.row_words} words)")
        return batch._count if batch._count is not None else batch.start[-1:]

    def add(self, batch) -> None:
        """append ``batch``'s records, the last ``capacity`` of them where it holds more; no wait: a count the host does not know
        is read on the device from ``batch.start``"""
        count = self._accept(batch)
        self.dev.replay_add(self.ring, self.state, batch.records, count)
        self._host_state = None

    def _result(self, out, slots):
        batch = DeviceBatch(out, self.layout, None, count=int(out.shape[0]), epoch=self.draws, dev=self.dev)
        batch.slots = slots
        self.draws += 1
        return batch

    def _need_ring(self, what):
        if self.ring is None:
            raise ValueError(f"ReplayBuffer.{what}: nothing was ever added")

    def sample(self, n: int):
        """a ``DeviceBatch`` of n records drawn uniformly with replacement from the records held: ``count = n``, ``epoch`` the number
        of this draw, ``.slots`` i64 ``[n]`` the slot of every record (-1 and a record of zeros while the ring holds none); ``row`` /
        ``col`` are None"""
        self._need_ring("sample")
        out, slots = self.dev.replay_sample(self.ring, self.state, n, seed=self.seed, draw=self.draws)
        return self._result(out, slots)

    def gather(self, slots):
        """``sample``'s result for the caller's own slots (a device i64 ``[n]`` tensor): a slot outside the records held gives a
        record of zeros and -1 in ``.slots``"""
        self._need_ring("gather")
        if slots is None or not hasattr(slots, "dim") or slots.dim() != 1 or slots.numel() < 1:
            raise ValueError("ReplayBuffer.gather: `slots` must be a device i64 [n] tensor with n >= 1")
        out, got = self.dev.replay_sample(self.ring, self.state, int(slots.numel()), slots=slots)
        return self._result(out, got)

    def _read_state(self):
        if self.state is None:
            return np.zeros((), _abi.REPLAY_STATE_DTYPE)
        if self._host_state is None:
            self._host_state = self.state.cpu().numpy().view(_abi.REPLAY_STATE_DTYPE)[0]
        return self._host_state

    def __len__(self):
        return int(self._read_state()["size"])

    @property
    def total(self) -> int:
        return int(self._read_state()["total"])

    @property
    def refused(self) -> int:
        return int(self._read_state()["refused"])


class PrioritizedReplayBuffer(ReplayBuffer):
    """``prb = PrioritizedReplayBuffer(env, capacity, alpha=0.6, eps=1e-6)``: a ``ReplayBuffer`` whose minibatches are drawn with
    probability proportional to priority, as RLlib's ``PrioritizedReplayBuffer`` draws (DQN, Ape-X, optionally SAC) --
    include/phantom_amd_prio.h.  ``env.sample(T, n_step=n, batcher=tb, replay=prb)`` and ``prb.add(batch)`` work as the parent's; a new
    record gets the largest priority seen so far (1 at first).  ``prb.sample(n, beta)`` gives the parent's ``DeviceBatch`` with
    ``.priorities`` and ``.weights`` next to ``.slots``; the learner computes its TD errors and calls
    ``prb.update_priorities(mb.slots, td_error.abs())``.  A sum tree and a min tree of 16 children per node (f32, about 1.13 words per
    slot in all) and a 32-byte state live next to the ring; no call copies anything to the host or waits.

    Out of scope as in the header: stratified draws, sampling without replacement, a slot overwritten by an ``add`` between its draw
    and its update (the new record then gets the old one's priority; RLlib has the same hazard), more than one GPU."""

    def __init__(self, env, capacity: int, alpha: float = 0.6, eps: float = 1e-6, seed: int = 0):
        super().__init__(env, capacity, seed=seed)
        if self.capacity > _abi.PRIO_MAX_CAPACITY:
            raise ValueError(f"PrioritizedReplayBuffer: capacity = {capacity!r} must be an int in [1, 2^30]")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.floating, np.integer)) or not alpha > 0:
            raise ValueError(f"PrioritizedReplayBuffer: alpha = {alpha!r} must be a number > 0")
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.floating, np.integer)) or not eps >= 0:
            raise ValueError(f"PrioritizedReplayBuffer: eps = {eps!r} must be a number >= 0")
        self.alpha, self.eps = float(alpha), float(eps)
        self.tree = self.pstate = None
        self._host_pstate = None

    def add(self, batch) -> None:
        """the parent's ``add``, after ``prio_add`` has given the slots it will write the largest priority seen so far: two calls in
        stream order, the tree's first because it reads the ring's state before the ring's add advances it"""
        import torch
        count = self._accept(batch)
        if self.tree is None:
            self.tree = torch.zeros(_abi.prio_layout(self.capacity)[3], dtype=torch.float32, device=self.ring.device)
            self.pstate = torch.zeros(_abi.PRIO_STATE_BYTES, dtype=torch.uint8, device=self.ring.device)
            self._pmin = self.tree[_abi.prio_min_root(self.capacity):][:1]      # a one-element view of the min tree's root
        self.dev.prio_add(self.tree, self.pstate, self.state, self.capacity, int(batch.records.shape[0]), count)
        self.dev.replay_add(self.ring, self.state, batch.records, count)
        self._host_state = self._host_pstate = None

    def sample(self, n: int, beta: float = 0.4):
        """a ``DeviceBatch`` of n records drawn with replacement, each with probability priority / total: the parent's result with
        ``.priorities`` f32 ``[n]`` (each record's priority as the tree holds it) and ``.weights`` f32 ``[n]``, RLlib's normalized
        importance weights ``(pmin / priority) ** beta`` = ``(p_i N) ** -beta / max_weight`` with pmin the smallest priority held
        (0 where ``.slots`` is -1: nothing is held)"""
        import torch
        self._need_ring("sample")
        if isinstance(beta, bool) or not isinstance(beta, (int, float, np.floating, np.integer)) or not 0 <= beta <= 1:
            raise ValueError(f"PrioritizedReplayBuffer.sample: beta = {beta!r} must lie in [0, 1]")
        slots, prios = self.dev.prio_sample(self.tree, self.pstate, self.state, self.capacity, n, seed=self.seed, draw=self.draws)
        out, got = self.dev.replay_sample(self.ring, self.state, n, slots=slots)
        batch = self._result(out, got)
        batch.priorities = prios
        held = got >= 0
        batch.weights = torch.where(held, (self._pmin / torch.where(held, prios, torch.ones_like(prios))) ** float(beta), torch.zeros_like(prios))
        return batch

    def update_priorities(self, slots, priorities) -> None:
        """the sampled ``slots`` (device i64 ``[n]``) get ``(priorities + eps) ** alpha``; ``priorities`` (device f32 ``[n]``) are the
        learner's TD-error magnitudes.  Slots outside the records held are ignored (``ignored`` counts them)"""
        self._need_ring("update_priorities")
        if priorities is None or not hasattr(priorities, "dim"):
            raise ValueError("PrioritizedReplayBuffer.update_priorities: `priorities` must be a device f32 [n] tensor")
        self.dev.prio_update(self.tree, self.pstate, self.state, self.capacity, slots, (priorities + self.eps) ** self.alpha)
        self._host_pstate = None

    @property
    def ignored(self) -> int:
        """update entries whose slot held no record; read from the device once, when asked, and again only after a further call"""
        if self.pstate is None:
            return 0
        if self._host_pstate is None:
            self._host_pstate = self.pstate.cpu().numpy().view(_abi.PRIO_STATE_DTYPE)[0]
        return int(self._host_pstate["ignored"])


def check_replay(replay, batcher):
    """``sample(replay=...)``'s argument against its batcher, before anything runs: ``{policy_id: ReplayBuffer}``"""
    if batcher is None:
        raise ValueError("sample: `replay` needs `batcher` (the ring holds a DeviceBatch's records)")
    if batcher.max_seq_len is not None:
        raise ValueError("sample: `replay` does not take the sequence batches of a batcher built with max_seq_len")
    pids = list(batcher.policies)
    if isinstance(replay, ReplayBuffer):
        if len(pids) != 1:
            raise ValueError(f"sample: `replay` must be a dict with the batcher's policy ids {pids}: one ReplayBuffer serves one policy")
        return {pids[0]: replay}
    if not isinstance(replay, dict) or set(replay) != set(pids) or not all(isinstance(rb, ReplayBuffer) for rb in replay.values()):
        raise ValueError(f"sample: `replay` must be a ReplayBuffer (one policy) or a dict of them with exactly the batcher's policy ids {pids}")
    return dict(replay)
