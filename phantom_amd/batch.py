"""A torch learner's batches on the device: ``TrainBatcher`` turns the time-major planes of a ``PhantomEnv.sample()`` fragment into one
``DeviceBatch`` per policy -- hole rows dropped, rows in (env instance, agent, step) order, ``advantages`` standardized, the rows
shuffled -- with one ``DeviceEnv.train_batch`` call each (include/phantom_amd_batch.h); with ``max_seq_len`` into one ``DeviceSeqBatch``
per policy -- every agent's rows cut into padded sequences, the sequences shuffled -- with one ``DeviceEnv.seq_batch`` call each
(include/phantom_amd_seq.h).  Nothing is copied to the host."""
import numpy as np

DEFAULT_POLICY_ID = "default_policy"
FLAG_COLUMNS = ("terminateds", "truncateds", "nstep_terminateds", "nstep_truncateds")


class DeviceBatch:
    """One policy's shuffled records on the device.  ``records`` is i32 ``[capacity, row_words]``; ``layout[name] = (word_off, w,
    dtype, tail)`` places a column in a record (``tail``: the column's trailing shape, ``()`` or ``(w,)``).  ``columns[name]`` is a
    strided view ``[K, ..]`` of ``records`` in the column's dtype (a flag column: ``!= 0`` of its word, a bool tensor); ``row`` /
    ``col`` the fragment row t and column n = b * S + s of every record (env_id = col // S, agent_index = col % S); ``moments`` the
    uint8 ``[32]`` record of ``_abi.BATCH_MOMENTS_DTYPE`` of the standardized column, or None.  ``count`` is K: given at construction
    where it is known without a wait, else one lazy 8-byte read of ``start[N]``."""

    def __init__(self, records, layout, start, row=None, col=None, moments=None, count=None, epoch=0, standardized=None, dev=None):
        self.records, self.layout, self.start, self.moments, self.dev = records, dict(layout), start, moments, dev
        self._row, self._col, self._count, self._columns = row, col, count, None
        self.epoch, self.standardized = epoch, standardized

    @property
    def count(self) -> int:
        if self._count is None:
            self._count = int(self.start[-1].item())
            if self._count > self.records.shape[0]:
                raise RuntimeError(f"DeviceBatch: {self._count} records do not fit the buffer of {self.records.shape[0]}: none was written")
        return self._count

    def __len__(self):
        return self.count

    @property
    def row(self):
        return None if self._row is None else self._row[:self.count]

    @property
    def col(self):
        return None if self._col is None else self._col[:self.count]

    @property
    def columns(self):
        if self._columns is None:
            K, cols = self.count, {}
            for name, (off, w, dtype, tail) in self.layout.items():
                x = self.records[:K, off:off + w]
                if name in FLAG_COLUMNS:
                    cols[name] = x[:, 0] != 0
                    continue
                if dtype != self.records.dtype:                  # (a byte column that is no flag: its word narrowed again, a copy)
                    x = x.view(dtype) if dtype.itemsize == 4 else x.to(dtype)
                cols[name] = x if tail else x[:, 0]
            self._columns = cols
        return self._columns

    def minibatches(self, size: int, drop_last: bool = False):
        """dicts of contiguous slices ``[i, i + size)`` of every column, in record order: the shuffle was done by the call"""
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
            raise ValueError(f"DeviceBatch.minibatches: size = {size!r} must be an int >= 1")
        K, cols = self.count, self.columns
        for i in range(0, K, size):
            if drop_last and i + size > K:
                return
            yield {name: x[i:i + size] for name, x in cols.items()}


class DeviceSeqBatch:
    """One policy's shuffled, padded sequences on the device (include/phantom_amd_seq.h).  ``records`` is i32 ``[capacity, L,
    row_words]``; ``layout`` is ``DeviceBatch``'s.  ``columns[name]`` is a strided view ``[Q, L, ..]`` of ``records`` in the column's
    dtype (a flag column: ``!= 0`` of its word), zero in padding; ``seq_lens`` ``[Q]`` the rows of every sequence and ``mask`` the bool
    ``[Q, L]`` ``arange(L) < seq_lens[:, None]``; ``seq_row`` / ``seq_col`` ``[Q]`` the fragment row and column n = b * S + s of a
    sequence's first row (where a learner gathers ``state_in`` from its own planes), ``row`` / ``col`` ``[Q, L]`` those of every slot,
    -1 in padding; ``moments`` as ``DeviceBatch``'s.  ``num_sequences`` is Q, one lazy 8-byte read of ``seq_start[N]``; ``count`` is K,
    the rows, one lazy read of the sum of ``seq_lens``."""

    def __init__(self, records, layout, seq_start, seq_lens, seq_row=None, seq_col=None, row=None, col=None, moments=None, epoch=0,
                 standardized=None, dev=None):
        self.records, self.layout, self.seq_start, self.moments, self.dev = records, dict(layout), seq_start, moments, dev
        self._lens, self._seq_row, self._seq_col, self._row, self._col = seq_lens, seq_row, seq_col, row, col
        self._q, self._count, self._columns, self._mask = None, None, None, None
        self.epoch, self.standardized = epoch, standardized
        self.max_seq_len = int(records.shape[1])

    @property
    def num_sequences(self) -> int:
        if self._q is None:
            self._q = int(self.seq_start[-1].item())
            if self._q > self.records.shape[0]:
                raise RuntimeError(f"DeviceSeqBatch: {self._q} sequences do not fit the buffer of {self.records.shape[0]}: none was written")
        return self._q

    def __len__(self):
        return self.num_sequences

    @property
    def count(self) -> int:
        if self._count is None:
            self._count = int(self.seq_lens.sum().item())
        return self._count

    @property
    def seq_lens(self):
        return self._lens[:self.num_sequences]

    @property
    def seq_row(self):
        return None if self._seq_row is None else self._seq_row[:self.num_sequences]

    @property
    def seq_col(self):
        return None if self._seq_col is None else self._seq_col[:self.num_sequences]

    @property
    def row(self):
        return None if self._row is None else self._row[:self.num_sequences]

    @property
    def col(self):
        return None if self._col is None else self._col[:self.num_sequences]

    @property
    def mask(self):
        if self._mask is None:
            lens = self.seq_lens
            self._mask = _arange_like(lens, self.max_seq_len)[None, :] < lens[:, None]
        return self._mask

    @property
    def columns(self):
        if self._columns is None:
            Q, cols = self.num_sequences, {}
            for name, (off, w, dtype, tail) in self.layout.items():
                x = self.records[:Q, :, off:off + w]
                if name in FLAG_COLUMNS:
                    cols[name] = x[..., 0] != 0
                    continue
                if dtype != self.records.dtype:                  # (a byte column that is no flag: its word narrowed again, a copy)
                    x = x.view(dtype) if dtype.itemsize == 4 else x.to(dtype)
                cols[name] = x if tail else x[..., 0]
            self._columns = cols
        return self._columns

    def minibatches(self, n_sequences: int, drop_last: bool = False):
        """dicts of contiguous slices ``[i, i + n_sequences)`` of every column plus ``seq_lens`` and ``mask``, whole sequences in
        record order: the shuffle was done by the call"""
        if isinstance(n_sequences, bool) or not isinstance(n_sequences, (int, np.integer)) or n_sequences < 1:
            raise ValueError(f"DeviceSeqBatch.minibatches: n_sequences = {n_sequences!r} must be an int >= 1")
        Q, cols = self.num_sequences, dict(self.columns, seq_lens=self.seq_lens, mask=self.mask)
        for i in range(0, Q, n_sequences):
            if drop_last and i + n_sequences > Q:
                return
            yield {name: x[i:i + n_sequences] for name, x in cols.items()}


def _arange_like(x, n):
    import torch
    return torch.arange(n, dtype=x.dtype, device=x.device)


class TrainBatcher:
    """``tb = TrainBatcher(env)``; ``batches = env.sample(T, ..., batcher=tb)`` gives ``{policy_id: DeviceBatch}``.

    ``policy_mapping_fn(agent_id)`` splits the strategic agents into policies (default: one, ``"default_policy"``); a policy's columns
    are selected by class inside the call.  ``standardize`` names at most one column, standardized over the policy's kept rows where
    the fragment has it.  The shuffle of call number c (``calls``, counted from 0 and shared with ``reshuffle``) is ``perm_K`` of
    ``(seed, epoch = c)``: every call and every reshuffle draws a new order, reproducibly.

    ``max_seq_len``: None, or an int L for a recurrent or attention learner: ``collect`` then makes one ``DeviceEnv.seq_batch`` call per
    policy in place of ``train_batch`` and returns ``{policy_id: DeviceSeqBatch}`` -- every agent's rows in time order, cut at the
    ``"terminateds"`` / ``"truncateds"`` planes it is handed and every L rows, padded to L, the sequences shuffled -- under the same
    epoch counter and with the same standardized column."""

    def __init__(self, env, seed: int = 0, standardize=("advantages",), policy_mapping_fn=None, max_seq_len=None):
        standardize = (standardize,) if isinstance(standardize, str) else tuple(standardize or ())
        if len(standardize) > 1:
            raise ValueError(f"TrainBatcher: one call standardizes one column, got {standardize}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"TrainBatcher: seed = {seed!r} must be an int in [0, 2^64)")
        self.agent_ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
        self.B, self.S = int(env.batch_size), int(env.spec.n_strategic)
        self.seed, self.standardize, self.calls = int(seed), standardize[0] if standardize else None, 0
        fn = policy_mapping_fn or (lambda aid: DEFAULT_POLICY_ID)
        self.policies = {}                                   # policy id -> its agents' indices, in agent order
        for s, aid in enumerate(self.agent_ids):
            self.policies.setdefault(fn(aid), []).append(s)
        if len(self.policies) > 256:
            raise ValueError(f"TrainBatcher: {len(self.policies)} policies, a column's class is one byte")
        self.col_class = np.zeros(self.S, np.uint8)
        for c, idx in enumerate(self.policies.values()):
            self.col_class[idx] = c
        self._class_dev = None
        self.max_seq_len = None
        if max_seq_len is not None:
            if isinstance(max_seq_len, bool) or not isinstance(max_seq_len, (int, np.integer)) or not 1 <= max_seq_len <= 65536:
                raise ValueError(f"TrainBatcher: max_seq_len = {max_seq_len!r} must be None or an int in [1, 65536]")
            self.max_seq_len, self.num_steps = int(max_seq_len), int(env.num_steps)

    def seq_capacity(self, T: int, n_agents: int) -> int:
        """the sequences ``n_agents`` agents' columns can have in a fragment of T rows: a column's length cuts, plus one per episode end
        inside the fragment (a done flag appears at most once per agent and episode)"""
        return self.B * n_agents * (-(-T // self.max_seq_len) + (T - 1) // self.num_steps + 1)

    def next_epoch(self) -> int:
        self.calls += 1
        return self.calls - 1

    def collect(self, dev, planes, keep=None):
        """``{policy_id: DeviceBatch}`` from time-major device planes ``[T, B, S, ..]`` named as ``to_sample_batches()``'s columns;
        ``keep``: who acted (u8 ``[T, B, S]``), None on a plain env.  One ``dev.train_batch`` call per policy, all with this call's
        epoch; no wait"""
        import torch
        first = next(iter(planes.values()))
        T = int(first.shape[0])
        if tuple(first.shape[1:3]) != (self.B, self.S):
            raise ValueError(f"TrainBatcher.collect: planes of shape {tuple(first.shape)}, expected [T, {self.B}, {self.S}, ..]")
        if self._class_dev is None or self._class_dev.device != dev.device:
            self._class_dev = torch.from_numpy(self.col_class).to(dev.device)
        std = self.standardize if self.standardize in planes else None
        epoch = self.next_epoch()
        tails = {name: tuple(x.shape[3:]) for name, x in planes.items()}
        one = len(self.policies) == 1
        out = {}
        for c, (pid, idx) in enumerate(self.policies.items()):
            if self.max_seq_len is not None:
                cap = self.seq_capacity(T, len(idx))
                start, records, lens, srow, scol, row, col, moments, lay = dev.seq_batch(
                    planes, self.max_seq_len, keep=keep, terminated=planes.get("terminateds"), truncated=planes.get("truncateds"),
                    col_class=None if one else self._class_dev, class_id=c, standardize=std, shuffle=True, seed=self.seed, epoch=epoch,
                    capacity=cap, lead_dims=3)
                layout = {name: (off, w, dtype, tails[name]) for name, (off, w, dtype) in lay.items()}
                out[pid] = DeviceSeqBatch(records, layout, start, lens, srow, scol, row, col, moments, epoch=epoch, standardized=std, dev=dev)
                continue
            cap = T * self.B * len(idx)
            start, records, row, col, moments, lay = dev.train_batch(planes, keep=keep, col_class=None if one else self._class_dev, class_id=c,
                                                                     standardize=std, shuffle=True, seed=self.seed, epoch=epoch, capacity=cap,
                                                                     lead_dims=3)
            layout = {name: (off, w, dtype, tails[name]) for name, (off, w, dtype) in lay.items()}
            out[pid] = DeviceBatch(records, layout, start, row, col, moments, count=cap if keep is None else None, epoch=epoch, standardized=std,
                                   dev=dev)
        return out

    def reshuffle(self, batch):
        """the next epoch's order of ``batch``: the same call on its dense records (T = 1, N = K, every record kept, nothing
        standardized), written into a second buffer; ``row`` / ``col`` follow their records.  Records of up to 64 words.  A
        ``DeviceSeqBatch`` is refused: reshuffling sequences is not offered"""
        if isinstance(batch, DeviceSeqBatch):
            raise ValueError("TrainBatcher.reshuffle: reshuffling a sequence batch (DeviceSeqBatch) is out of scope; collect a new one")
        K, rw, dev = batch.count, int(batch.records.shape[1]), batch.dev
        if rw > 64:
            raise ValueError(f"TrainBatcher.reshuffle: records of {rw} words, one plane moves at most 64")
        epoch = self.next_epoch()
        if K == 0:
            return DeviceBatch(batch.records, batch.layout, batch.start, batch._row, batch._col, batch.moments, count=0, epoch=epoch,
                               standardized=batch.standardized, dev=dev)
        src = batch.records[:K].view(1, K, rw)
        start, records, _, src_of, _, _ = dev.train_batch({"records": src}, shuffle=True, seed=self.seed, epoch=epoch, row_words=rw, capacity=K,
                                                            lead_dims=2)
        pick = lambda x: None if x is None else x[:K].index_select(0, src_of.long())
        return DeviceBatch(records, batch.layout, start, pick(batch._row), pick(batch._col), batch.moments, count=K, epoch=epoch,
                           standardized=batch.standardized, dev=dev)
