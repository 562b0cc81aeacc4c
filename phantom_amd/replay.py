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

    Out of scope here as in the header: prioritized sampling (``gather(slots)`` and a sample's ``.slots`` are its building block),
    sampling without replacement, sequence batches, spilling to the host, more than one GPU."""

    def __init__(self, env, capacity: int, seed: int = 0):
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise ValueError(f"ReplayBuffer: capacity = {capacity!r} must be an int >= 1")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"ReplayBuffer: seed = {seed!r} must be an int in [0, 2^64)")
        self.env, self.capacity, self.seed, self.draws = env, int(capacity), int(seed), 0
        self.ring = self.state = self.layout = self.row_words = self.dev = None
        self._host_state = None

    def add(self, batch) -> None:
        """append ``batch``'s records, the last ``capacity`` of them where it holds more; no wait: a count the host does not know
        is read on the device from ``batch.start``"""
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
        count = batch._count if batch._count is not None else batch.start[-1:]
        self.dev.replay_add(self.ring, self.state, records, count)
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
