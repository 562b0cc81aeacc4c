"""DeviceEnv: the thin ctypes layer between the Python host surface and libphantom_amd.so.

PyTorch-ROCm tensors own every buffer (state blob, inputs, outputs); the library receives raw
device pointers plus torch's current HIP stream, so all calls are stream-ordered with the
caller's other torch work and nothing synchronises unless the caller reads values back.
There is NO CPU fallback: without a visible GPU or the built HIP library this raises.
"""
import ctypes as C
from contextlib import contextmanager
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from . import _abi
from ._buffers import AtLeast, Layout, check_tensor
from .message import Message, payload_to_record, record_to_payload
from .spec import EnvSpec


def _torch():
    import torch
    return torch


_ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else None
# rollout argument-block cache keys: address AND size, so that a buffer freed and reallocated smaller misses
_sig = lambda x: (x.data_ptr(), x.numel()) if hasattr(x, "data_ptr") else None


def _step_layout(B, S, D) -> Layout:
    """the step outputs: 256-byte aligned sections of ONE device buffer, so that the dict API (PhantomEnv.step) brings
    them to the host with a single copy (pull_step)"""
    t = _torch()
    return Layout([("obs", (B, S, D), t.float32), ("reward", (B, S), t.float64)] +
                  [(k, (B, S), t.uint8) for k in ("obs_valid", "reward_valid", "terminated", "truncated", "done_valid")] +
                  [("all_terminated", (B,), t.uint8), ("all_truncated", (B,), t.uint8), ("err", (B,), t.int32)])


def _fragment_layout(T, B, S, D, valid_planes: bool, flag_planes: int) -> Layout:
    """a flat fragment (alloc_trajectory(flat=True)); ``packed_flags``: ``flag_planes`` bit-packed done planes of whole 64-bit words"""
    t = _torch()
    step = (T, B, S)
    masks = [("obs_valid", step, t.uint8), ("reward_valid", step, t.uint8)] if valid_planes else []
    return Layout([("observations", (T, B, S, D), t.float32), ("actions", step, t.float32), ("rewards", step, t.float32)] + masks +
                  [("packed_flags", (flag_planes * ((T * B * S + 63) // 64) * 8,), t.uint8),
                   ("truncations", step, t.uint8), ("terminations", step, t.uint8), ("last_obs", (B, S, D), t.float32)])


class StepTensors(NamedTuple):
    """Device-resident result of one batched step (views of persistent buffers; valid until
    the next step call on the same env)."""
    observations: "object"   # f32 [B, S, D]
    rewards: "object"        # f64 [B, S]
    terminations: "object"   # u8  [B, S]
    truncations: "object"    # u8  [B, S]
    obs_valid: "object"      # u8  [B, S]
    reward_valid: "object"   # u8  [B, S]  0 absent / 1 value / 2 None
    done_valid: "object"     # u8  [B, S]
    all_terminated: "object" # u8  [B]
    all_truncated: "object"  # u8  [B]


class Trajectory(NamedTuple):
    """Device-resident rollout fragment, time-major."""
    observations: "object"   # f32 [T, B, S, D]
    actions: "object"        # f32 [T, B, S]
    rewards: "object"        # f32 [T, B, S]
    terminations: "object"   # u8  [T, B, S]
    truncations: "object"    # u8  [T, B, S]
    last_obs: "object"       # f32 [B, S, D]
    obs_valid: "object" = None      # u8 [T, B, S]  (FSM envs: key present in step.observations)
    reward_valid: "object" = None   # u8 [T, B, S]  (FSM envs: 0 absent / 1 value / 2 None)
    msg_log: "object" = None        # u8 [T, B, trace_cap, 16]  ordered message records per step (tracking on)
    msg_count: "object" = None      # i32 [T, B]
    flat: "object" = None           # u8 [nbytes]: the one buffer every plane above is a section of (alloc_trajectory(flat=True))
    packed_flags: "object" = None   # u8 view of `flat`: bit-packed done flags for rollout collection (pack_done_flags)
    gather_nbytes: int = 0          # prefix of `flat` a learner needs from every rank (distributed.TrajectoryGather)
    # an exploring rollout (rollout(noise=...), alloc_trajectory(explore=True)): RLlib's columns of a Gaussian policy
    raw_actions: "object" = None    # f32 [T, B, S]     z = mean + exp(log_std) noise, SampleBatch "actions" (`actions` above: the env's)
    action_logp: "object" = None    # f32 [T, B, S]     log N(z; mean, exp(log_std)), "action_logp"
    dist_inputs: "object" = None    # f32 [T, B, S, 2]  (mean, log_std) unclamped, "action_dist_inputs"


class DeviceError(RuntimeError):
    pass


class HostStep:
    """A step's outputs in flight to the host (DeviceEnv.pull_step_async)."""

    def __init__(self, dev, buf, event, seq):
        self._dev, self._buf, self._event, self._seq, self._arrays = dev, buf, event, seq, None
        self._consumed = False          # read_into() has copied the arrays out: nothing is left to keep alive

    @contextmanager
    def _host_views(self):
        """the step's arrays on the host, as views that are valid inside the ``with`` block only (get(): copies that last)"""
        if self._arrays is not None:
            yield self._arrays
        elif self._buf is None:                                   # lazy: from the step outputs themselves
            if self._dev._out_seq != self._seq:
                raise DeviceError("a poll() result was first read after a later step / reset had overwritten the step outputs: read it "
                                  "before the next send_actions(), or build the adapter with keep_results=True")
            yield self._dev.pull_step()
        else:
            if self._dev._host_ring_k - self._seq > 3:            # three pinned buffers rotate: this one has been reused since
                raise DeviceError("a poll() result was first read more than three steps after it was produced: its host buffer has been reused")
            self._event.synchronize()
            yield self._dev._out_layout.numpy_views(self._buf.numpy())
            if self._dev._host_ring_k - self._seq > 3:            # (reused while it was being read: what the caller took is void)
                raise DeviceError("a poll() result was read while its host buffer was being reused")

    def read_into(self, dst: Dict[str, "object"]) -> None:
        """the arrays copied straight into ``dst`` (same names, shapes and dtypes): one copy instead of get()'s copy + the caller's"""
        with self._host_views() as views:
            for k, v in views.items():
                np.copyto(dst[k], v)
        self._consumed = True

    def materialise(self) -> None:
        """bring the arrays to the host now if nobody has read them yet (DeviceEnv calls this for a result that is still referenced
        right before its pinned buffer is reused: a poll() result then outlives any number of later steps)"""
        if self._arrays is None and not self._consumed:
            self.get()

    def get(self) -> Dict[str, "object"]:
        """copies of the arrays, made on the first call and kept (not kept when that read raised)"""
        if self._arrays is None:
            with self._host_views() as views:
                arrays = {k: v.copy() for k, v in views.items()}
            self._arrays = arrays
        return self._arrays


class StepGraph:
    """``n`` captured ``phx_step`` launches (DeviceEnv.step_graph); ``replay()`` enqueues them on the
    current stream without per-step host work."""

    def __init__(self, graph, actions, out, n, dev=None):
        self.graph, self.actions, self.out, self.n, self._dev = graph, actions, out, n, dev

    def replay(self):
        if self._dev is not None:
            self._dev._out_seq += 1      # the replay rewrites the step outputs: a lazy poll() result of an earlier step must not read them
        self.graph.replay()
        return self.out


class RolloutGraph:
    """Consecutive ``phx_rollout`` fragments captured ONCE into a hipGraph (DeviceEnv.rollout_graph): ``replay()`` enqueues them on
    the current stream; fragment i of a replay lands in ``trajectories[i]`` (rewritten by every replay)."""

    def __init__(self, graph, trajectories, T):
        self.graph, self.trajectories, self.T = graph, trajectories, T

    def replay(self):
        self.graph.replay()
        return self.trajectories


class DeviceEnv:
    def __init__(self, spec: EnvSpec, device=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise DeviceError("phantom_amd needs a visible AMD GPU (torch.cuda.is_available() is "
                              "False); the PhantomEnv.step() path has no CPU fallback")
        self.lib = _abi.load_library()
        self.spec = spec
        self.device = torch.device(device if device is not None
                                   else f"cuda:{torch.cuda.current_device()}")
        if self.device.index is None:
            self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        self._cspec, self._keep = spec.to_ctypes()
        cs = C.byref(self._cspec)
        self.B, self.S = spec.batch, spec.n_strategic
        self.D = self.lib.phx_obs_dim(cs)
        self.n_exo = self.lib.phx_n_exo(cs)
        assert self.lib.phx_n_strategic(cs) == self.S
        nbytes = self.lib.phx_state_nbytes(cs)
        if nbytes <= 0:
            raise DeviceError("phx_state_nbytes failed: " + self._err())
        self.state = torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)
        handle = C.c_void_p()
        # phx_create uploads tables and runs the initial reset on the NULL stream; the zero fill above ran
        # on torch's current stream, which need not be ordered against it (non-blocking side streams)
        torch.cuda.current_stream(self.device).synchronize()
        with torch.cuda.device(self.device):
            rc = self.lib.phx_create(cs, self.device.index, self.state.data_ptr(), nbytes,
                                     C.byref(handle))
        if rc != 0:
            raise DeviceError(f"phx_create failed ({rc}): " + self._err())
        self.handle = handle

        self._kind_rank = spec.kind_rank()
        self._fields: Dict[str, "object"] = {}
        dt = {0: torch.int32, 1: torch.float64, 2: torch.uint8, 3: torch.float32}       # phx_field.dtype
        for k in range(self.lib.phx_n_fields(handle)):
            f = _abi.PhxField()
            self.lib.phx_field_info(handle, k, C.byref(f))
            n = f.dim0 * f.dim1 * f.dim2
            view = self.state[f.offset:f.offset + n * dt[f.dtype].itemsize].view(dt[f.dtype])
            shape = [f.dim0, f.dim1] + ([f.dim2] if f.dim2 > 1 else [])
            self._fields[f.name.decode()] = view.view(*shape)
        B, S, D = self.B, max(self.S, 1), self.D
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=self.device)
        self._out_layout = _step_layout(B, S, D)
        self._out_flat = z(self._out_layout.nbytes, dtype=torch.uint8)
        self._out_host = None                                                # pinned; allocated by the first pull_step()
        self._host_ring, self._host_ring_owner, self._host_ring_k = [], [None, None, None], 0       # pull_step_async(): ditto
        self._rollout_io_cache = {}
        for name, view in self._out_layout.torch_views(self._out_flat).items():
            setattr(self, name, view)
        self.ones_valid = None
        self.msg_log = self.msg_count = None
        if spec.trace_cap > 0:
            self.msg_log = z(B, spec.trace_cap, 16, dtype=torch.uint8)
            self.msg_count = z(B, dtype=torch.int32)
        self.topology_version = 0
        self._step_io = None
        self._out_seq = 0                 # bumped by every call that rewrites the step outputs (HostStep: lazy reads)

    # ---- helpers --------------------------------------------------------------------------
    def _err(self) -> str:
        return (self.lib.phx_last_error() or b"").decode()

    def last_kernel(self) -> str:
        """names of the kernels this thread's last step / rollout / resolve call launched, joined by '+'"""
        return (self.lib.phx_last_kernel() or b"").decode()

    def autotune_note(self) -> str:
        """what PHX_VR_AUTO measured when it last had two kernels for a rollout shape of this env (phx_autotune_note), or ''"""
        return (self.lib.phx_autotune_note(self.handle) or b"").decode()

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise DeviceError(f"{what} failed ({rc}): {self._err()}")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.phx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def uses_fused(self) -> bool:
        """a fused static-schedule kernel serves step/rollout (can turn False: a host-injected
        message moves a fused Stackelberg env onto the generic engine for good)."""
        return bool(self.lib.phx_uses_fused(self.handle))

    def field(self, name: str):
        """torch view [B, n] into the state blob (zero-copy).  ``buyer.prices`` is kept in
        compressed per-seller form by the fused Stackelberg kernel and materialised here."""
        if name == "buyer.prices":
            self._check(self.lib.phx_sync_fields(self.handle, self._stream()), "phx_sync_fields")
        return self._fields[name]

    def field_names(self) -> List[str]:
        return list(self._fields)

    def _read_agent_state(self, agent, field_name: str):
        a = self.spec.index_of(agent.id)
        col = int(self._kind_rank[a])
        v = self._fields[field_name][:, col].cpu().numpy()
        if v.ndim > 1:                      # a per-agent vector (adv.total_*: counts keyed by user id)
            return v[0] if self.B == 1 else v
        return v[0].item() if self.B == 1 else v

    # ---- entry points ---------------------------------------------------------------------
    def reset(self, mask=None, sampler_values=None, conn_on=None):
        """``sampler_values``: f64 [B, n_samplers] (host array or device tensor) = what
        `sampler.sample()` returned for each env (env.py:211-212); ``conn_on``: u8 [B, n_conn] =
        the StochasticNetwork draws (network.py:444-447); None -> device-drawn."""
        torch = _torch()
        mp = vp = cp = None
        if conn_on is not None:
            self._conn_on = torch.as_tensor(conn_on, dtype=torch.uint8).to(self.device).contiguous()
            check_tensor("reset", "conn_on", self._conn_on, torch.uint8, (self.B, self.spec.n_conn), device=self.device)
            cp = self._conn_on.data_ptr()
        if sampler_values is not None:
            self._sampler_values = torch.as_tensor(sampler_values, dtype=torch.float64).to(
                self.device).contiguous()
            check_tensor("reset", "sampler_values", self._sampler_values, torch.float64, (self.B, self.spec.n_samplers), device=self.device)
            vp = self._sampler_values.data_ptr()
        if mask is not None:
            mask = torch.as_tensor(mask, dtype=torch.uint8, device=self.device).contiguous()
            check_tensor("reset", "mask", mask, torch.uint8, (self.B,), device=self.device)
            mp = mask.data_ptr()
            self.err.masked_fill_(mask.bool(), 0)
        else:
            self.err.zero_()
        self._out_seq += 1
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_reset(self.handle, mp, vp, cp, self.obs.data_ptr(),
                                           self.obs_valid.data_ptr(), self._stream()), "phx_reset")
        return self.obs, self.obs_valid

    def reset_agents(self):
        """Network.reset() without an env: agent.reset() for every agent."""
        self.reset()

    def _ensure_step_io(self):
        # the output pointers never change: build the struct once, patch the inputs per call
        if self._step_io is None:
            io = self._step_io = _abi.PhxStepIO()
            for name in self._out_layout.sections:         # (phx_step_io names its outputs as the layout does)
                setattr(io, name, getattr(self, name).data_ptr())
            if self.msg_log is not None:
                io.msg_log, io.msg_count = self.msg_log.data_ptr(), self.msg_count.data_ptr()
            self._step_io_ref = C.byref(io)
            self._step_out = StepTensors(self.obs, self.reward, self.terminated, self.truncated,
                                         self.obs_valid, self.reward_valid, self.done_valid,
                                         self.all_terminated, self.all_truncated)
        return self._step_io

    def step_begin(self, actions, action_valid=None, exo=None, shuffle=None):
        """phx_step_begin: the acting phase and resolve_network() of a step (fsm.py:275-280); agent state is the resolved one
        afterwards, the env's clock words and the step outputs are untouched.  Followed by ``step_end``."""
        return self.step(actions, action_valid, exo, shuffle, None, _entry="phx_step_begin")

    def step_end(self, next_stage=None) -> StepTensors:
        """phx_step_end: the transition to ``next_stage`` (int32 [B]; None: next_stages[0] / the tabulated handler) and the
        step's observations, rewards and done flags (fsm.py:304-380)."""
        torch = _torch()
        io = self._step_io if self._step_io is not None else self._ensure_step_io()
        io.next_stage = self._next_stage_ptr(next_stage)
        self._out_seq += 1
        rc = self.lib.phx_step_end(self.handle, self._step_io_ref, torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            self._check(rc, "phx_step_end")
        return self._step_out

    def _input_ptr(self, name, x, dtype, *shape):
        """the address of an optional per-step input, checked (None: not given)"""
        if x is None:
            return None
        check_tensor("step", name, x, dtype, shape, device=self.device)
        return x.data_ptr()

    def _next_stage_ptr(self, next_stage):
        """FSM stage handlers' return values, one stage index per env (None: next_stages[0] / the tabulated handler)"""
        return self._input_ptr("next_stage", next_stage, _torch().int32, self.B)

    def step(self, actions, action_valid=None, exo=None, shuffle=None, next_stage=None, _entry="phx_step") -> StepTensors:
        torch = _torch()
        io = self._step_io
        if io is None:
            io = self._ensure_step_io()
        if self.S > 0:
            # (the once-per-env-step check: the passing case is these comparisons alone, check_tensor states them and raises)
            if actions.dtype != torch.float32 or not actions.is_contiguous() \
                    or actions.shape != (self.B, self.S) or actions.device != self.device:
                check_tensor("step", "actions", actions, torch.float32, (self.B, self.S), device=self.device)
            io.actions = actions.data_ptr()
        io.action_valid = action_valid.data_ptr() if action_valid is not None else None
        io.exo = self._input_ptr("exo", exo, torch.uint8, self.B, self.n_exo) if exo is not None else None
        # recorded np.random.shuffle outcomes (BatchResolver(shuffle_batches=True))
        io.shuffle = self._input_ptr("shuffle", shuffle, (torch.int16, torch.uint16), self.B, 8 * self.spec.queue_cap) if shuffle is not None else None
        io.next_stage = self._next_stage_ptr(next_stage) if next_stage is not None else None
        self._out_seq += 1
        rc = getattr(self.lib, _entry)(self.handle, self._step_io_ref,
                                       torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            self._check(rc, _entry)
        return self._step_out

    def pull_step(self) -> Dict[str, "object"]:
        """numpy views of the last step's outputs (and err), fetched with ONE device-to-host copy."""
        torch = _torch()
        if self._out_host is None:
            self._out_host = torch.empty(self._out_flat.shape, dtype=torch.uint8, pin_memory=True)
        self._out_host.copy_(self._out_flat, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._out_layout.numpy_views(self._out_host.numpy())

    def pull_step_lazy(self) -> "HostStep":
        """The last step's outputs, brought to the host only if somebody reads them: ``HostStep.get()`` makes the one device-to-host
        copy (and the synchronisation) on its first call -- which has to come before the next launch overwrites the step outputs
        (DeviceError otherwise).  Costs nothing when the result is never read (a tensor-native loop that polls for form's sake)."""
        return HostStep(self, None, None, self._out_seq)

    def pull_step_async(self) -> "HostStep":
        """The last step's outputs on their way to the host WITHOUT a synchronisation: one non-blocking copy of the output buffer
        into one of three rotating pinned buffers with an event behind it.  ``HostStep.get()`` waits for the event (once) and
        returns copies of the arrays, so a result stays valid however many steps follow -- also one that is FIRST read many steps
        later: a result that is still referenced when its buffer comes up for reuse is copied out before the reuse; a HostStep
        nobody kept costs the copy (~25 us of stream time at SC64, B = 4096) and nothing on the host."""
        import weakref
        torch = _torch()
        ring, owners, k = self._host_ring, self._host_ring_owner, self._host_ring_k
        if len(ring) < 3:
            ring.append(torch.empty(self._out_flat.shape, dtype=torch.uint8, pin_memory=True))
        slot = k % 3 if len(ring) == 3 else len(ring) - 1
        prev = owners[slot]() if owners[slot] is not None else None
        if prev is not None:
            prev.materialise()           # somebody still holds the result that lives in this buffer and has not read it: copy it out first
        self._host_ring_k = k + 1
        buf = ring[slot]
        buf.copy_(self._out_flat, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        hs = HostStep(self, buf, ev, k)
        owners[slot] = weakref.ref(hs)
        return hs

    def _needs_valid_planes(self) -> bool:
        # validity masks: stage-masked envs, and kinds whose encode_observation can return None
        return self.spec.env_type != _abi.ENV_PLAIN or bool((self.spec.kind == _abi.KIND_ADVERTISER).any())

    def never_terminates(self) -> bool:
        """no strategic kind of this env can return is_terminated() == True (ShopAgent, the market's
        Seller/Buyer: agents.py:292-323 defaults), so the `terminations` plane of a trajectory is all zero."""
        k = self.spec.kind[self.spec.strategic_idx] if self.S else np.zeros(0, np.uint8)
        return bool(np.isin(k, (_abi.KIND_SHOP, _abi.KIND_SELLER, _abi.KIND_BUYER)).all())

    def alloc_trajectory(self, T: int, record_messages: bool = False, flat: bool = False,
                         terminations: bool = True, explore: bool = False) -> Trajectory:
        """Uninitialised device buffers for a T-step fragment (time-major).  ``record_messages``:
        also the per-step ordered message log (rollout.py:369-373, needs enable_tracking).
        ``explore``: also the planes of an exploring rollout (raw_actions, action_logp, dist_inputs).
        ``flat``: every plane is a 256-byte aligned section of ONE buffer, ordered so that what a
        learner on another GPU needs is a prefix: obs | actions | rewards | [obs_valid | reward_valid] |
        bit-packed done flags, then (not gathered) the u8 truncations / terminations planes."""
        torch = _torch()
        B, S, D = self.B, self.S, self.D
        e = lambda *s, dtype: torch.empty(*s, dtype=dtype, device=self.device)
        fsm = self._needs_valid_planes()
        if record_messages and self.spec.trace_cap <= 0:
            raise DeviceError("record_messages needs BatchResolver(enable_tracking=True)")
        if explore and flat:
            raise ValueError("alloc_trajectory: `explore` planes are not part of a flat fragment")
        if flat:
            layout = _fragment_layout(T, B, S, D, fsm, 1 if self.never_terminates() else 2)
            buf = torch.empty(layout.nbytes, dtype=torch.uint8, device=self.device)
            v = layout.torch_views(buf)
            return Trajectory(v["observations"], v["actions"], v["rewards"], v["terminations"], v["truncations"],
                              v["last_obs"], v.get("obs_valid"), v.get("reward_valid"), None, None,
                              buf, v["packed_flags"], layout.end("packed_flags"))
        # terminations=False: no `terminations` plane (it is all zero for kinds that never terminate; phx_rollout accepts
        # the omission where the serving kernel can leave the plane out and returns an error otherwise)
        # (truncations directly followed by terminations: where the library zero-fills the flag planes before a rollout kernel
        #  that only stores the non-zero flags, ONE fill covers both)
        if terminations and (T * B * S) % 256 == 0:
            flags = e(2, T, B, S, dtype=torch.uint8)
            trunc, term = flags[0], flags[1]
        else:
            trunc, term = e(T, B, S, dtype=torch.uint8), (e(T, B, S, dtype=torch.uint8) if terminations else None)
        tr = Trajectory(e(T, B, S, D, dtype=torch.float32), e(T, B, S, dtype=torch.float32),
                        e(T, B, S, dtype=torch.float32), term,
                        trunc, e(B, S, D, dtype=torch.float32),
                        e(T, B, S, dtype=torch.uint8) if fsm else None,
                        e(T, B, S, dtype=torch.uint8) if fsm else None,
                        e(T, B, self.spec.trace_cap, 16, dtype=torch.uint8) if record_messages else None,
                        e(T, B, dtype=torch.int32) if record_messages else None)
        if explore:
            tr = tr._replace(raw_actions=e(T, B, S, dtype=torch.float32), action_logp=e(T, B, S, dtype=torch.float32),
                             dist_inputs=e(T, B, S, 2, dtype=torch.float32))
        return tr

    def _check_rollout_planes(self, T, out: Trajectory):
        """the planes of a fragment that receives T steps: at least T rows each, on a 16-byte boundary.  Raw pointers go straight
        to the kernel, so every buffer is checked here (python -O strips asserts: these are real errors)."""
        torch = _torch()
        B, S, D = self.B, self.S, self.D

        def need(name, dtype, *tail):
            check_tensor("rollout", "out." + name, getattr(out, name), dtype, (B,) + tail, lead=AtLeast(T), align=16, device=self.device)

        if T < 1:
            raise ValueError("rollout: T must be >= 1")
        need("observations", torch.float32, S, D)
        need("actions", torch.float32, S)
        need("rewards", torch.float32, S)
        if out.terminations is not None:                   # None: the all-zero plane left out (the library decides whether it can be)
            need("terminations", torch.uint8, S)
        need("truncations", torch.uint8, S)
        check_tensor("rollout", "out.last_obs", out.last_obs, torch.float32, (B, S, D), align=16, device=self.device)
        if self._needs_valid_planes() or out.obs_valid is not None or out.reward_valid is not None:
            need("obs_valid", torch.uint8, S)
            need("reward_valid", torch.uint8, S)
        if out.msg_log is not None or out.msg_count is not None:
            if self.spec.trace_cap <= 0:
                raise ValueError("rollout: a message log needs BatchResolver(enable_tracking=True)")
            need("msg_count", torch.int32)
            need("msg_log", torch.uint8, self.spec.trace_cap, 16)

    def _check_explore_buffers(self, T, noise, out: Trajectory):
        """an exploring rollout's noise and planes (alloc_trajectory(T, explore=True)): [T, B, S] ([T, B, S, 2] for dist_inputs)"""
        f32, tail = _torch().float32, (self.B, self.S)
        check_tensor("rollout", "noise", noise, f32, tail, lead=T, device=self.device)
        check_tensor("rollout", "out.raw_actions", out.raw_actions, f32, tail, lead=AtLeast(T), device=self.device)
        check_tensor("rollout", "out.action_logp", out.action_logp, f32, tail, lead=AtLeast(T), device=self.device)
        check_tensor("rollout", "out.dist_inputs", out.dist_inputs, f32, tail + (2,), lead=AtLeast(T), device=self.device)

    def _rollout_io(self, what, T, actions, exo, actions_in_domain, exo_in_domain, last_obs):
        """the argument block of a T-step phx_rollout: hints, the (checked) replayed inputs, last_obs and err (the planes: _set_planes)"""
        torch = _torch()
        if actions is not None:
            check_tensor(what, "actions", actions, torch.float32, (self.B, self.S), lead=T, device=self.device)
        if exo is not None:
            check_tensor(what, "exo", exo, torch.uint8, (self.B, self.n_exo), lead=T, device=self.device)
        io = _abi.PhxRolloutIO()
        io.T = T
        io.hints = (_abi.RH_ACTIONS_IN_DOMAIN if actions_in_domain else 0) | (_abi.RH_EXO_IN_DOMAIN if exo_in_domain else 0)
        io.actions, io.exo, io.last_obs, io.err = _ptr(actions), _ptr(exo), _ptr(last_obs), self.err.data_ptr()
        return io

    @staticmethod
    def _set_planes(dst, o: Trajectory):
        """a fragment's seven plane pointers into a PhxRolloutIO or a PhxRolloutFrag (the same field names)"""
        dst.obs, dst.action_out, dst.reward = _ptr(o.observations), _ptr(o.actions), _ptr(o.rewards)
        dst.terminated, dst.truncated = _ptr(o.terminations), _ptr(o.truncations)
        dst.obs_valid, dst.reward_valid = _ptr(o.obs_valid), _ptr(o.reward_valid)

    def _cache_put(self, key, entry):
        if len(self._rollout_io_cache) >= 4:               # tiny LRU: drop the oldest entry
            self._rollout_io_cache.pop(next(iter(self._rollout_io_cache)))
        self._rollout_io_cache[key] = entry

    def rollout(self, T: int, actions=None, exo=None, out: Optional[Trajectory] = None, actions_in_domain: bool = False,
                exo_in_domain: bool = False, policy=None, noise=None) -> Trajectory:
        """T fused steps into ``out`` (allocated here when None); ``actions`` f32 [T, B, S] / ``exo`` u8 [T, B, n_exo] replay a recorded
        policy / recorded draws (None: the device's random policy / RNG stream).  ``actions_in_domain`` / ``exo_in_domain``: the caller
        vouches that every action rounds to >= 0 (clipped to the action space) / every exo byte is < 5 (``mt_draw`` output): a plain supply
        chain's replay then takes the store-wave kernel without a scan of the inputs (phx_rollout_io.hints).
        ``policy``: a ``phantom_amd.policy.MLPPolicy`` evaluated on the device for every (env, strategic agent) and step from the agent's
        previous observation (phx_rollout_io.policy, ABI 10): T ON-POLICY steps in one launch (plain supply-chain envs).
        ``noise``: f32 [T, B, S] standard-normal draws (e.g. torch.randn) -- a stochastic ``policy`` EXPLORES with them
        (phx_policy_explore): the env takes clip(out_scale z + out_bias), z = mean + exp(log_std) noise, and ``out.raw_actions`` /
        ``out.action_logp`` / ``out.dist_inputs`` receive z, its log-probability and (mean, log_std)."""
        if policy is not None and actions is not None:
            raise ValueError("rollout: `policy` and replayed `actions` exclude each other")
        if noise is not None and (policy is None or not policy.stochastic):
            raise ValueError("rollout: `noise` needs a stochastic policy (a (mean, log_std) head or MLPPolicy(log_std=...))")
        owned = out is None
        if owned:
            out = self.alloc_trajectory(T, explore=noise is not None)
        # The argument block of a repeated call into CALLER-owned buffers is built once.  The key is
        # the buffers' addresses and the entry holds no tensor: a fragment allocated here (out=None)
        # is never cached, so repeated env.rollout(T) calls pin nothing (a T=100 SC64 fragment is
        # ~80 MB at B=4096).
        key = (T, bool(actions_in_domain), bool(exo_in_domain)) + tuple(_sig(x) for x in out[:10]) + (_sig(actions), _sig(exo), id(policy)) \
            + ((_sig(noise), _sig(out.raw_actions), _sig(out.action_logp), _sig(out.dist_inputs)) if noise is not None else ())
        cached = None if owned else self._rollout_io_cache.get(key)
        if cached is None:
            self._check_rollout_planes(T, out)
            io = self._rollout_io("rollout", T, actions, exo, actions_in_domain, exo_in_domain, out.last_obs)
            self._set_planes(io, out)
            io.msg_log, io.msg_count = _ptr(out.msg_log), _ptr(out.msg_count)
            pol_keep = None
            if policy is not None:
                if policy.obs_dim != self.D:
                    raise ValueError(f"rollout: the policy takes {policy.obs_dim} inputs, the env's observations have {self.D}")
                pol_keep = policy.on(self.device)              # (device weights + the argument struct: kept alive with the cached block)
                io.policy = C.addressof(pol_keep[2])
                if noise is not None:
                    self._check_explore_buffers(T, noise, out)
                    ex = policy.explore_struct(self.device, noise, out.raw_actions, out.action_logp, out.dist_inputs)
                    pol_keep = pol_keep + (ex,)
                    io.reserved_ptr = C.addressof(ex)          # (phx_rollout_io.explore)
            cached = (io, C.byref(io), pol_keep, policy)
            if not owned:
                self._cache_put(key, cached)
        self._check(self.lib.phx_rollout(self.handle, cached[1], self._stream()), "phx_rollout")     # the library selects its device itself
        return out

    def rollout_fragments(self, T: int, outs, actions=None, exo=None, actions_in_domain: bool = False,
                          exo_in_domain: bool = False) -> List[Trajectory]:
        """``len(outs)`` consecutive T-step fragments from ONE ``phx_rollout`` call (``phx_rollout_io.frags``, ABI 9): the env
        advances ``len(outs) * T`` steps exactly as the same number of ``rollout(T, out=outs[i])`` calls would, fragment i holds
        rows ``[i T, (i + 1) T)``.  The fixed cost of a launch (pipeline fill, placing a 160 KB workgroup on every CU, the kernel
        boundary: ~9 us against 12.5 us of streaming per 100 steps of SC64 at B = 4096) is paid once per call instead of once per
        fragment where the store-wave supply-chain kernel serves the env; other envs run one launch per fragment inside the call.
        ``actions`` / ``exo``: replayed inputs for all ``len(outs) * T`` steps (``*_in_domain``: as in ``rollout``).
        ONE difference from separate calls: only the observation after the LAST step is produced (``phx_rollout_io.last_obs``, written to
        ``outs[-1].last_obs``); the library has no per-fragment boundary observation, so the returned fragments i < k - 1 carry
        ``last_obs=None`` (their ``last_obs`` tensors are left untouched) -- a learner that bootstraps from a fragment's boundary uses the
        next fragment's first row inputs, or asks for one fragment per call."""
        outs = list(outs)
        k = len(outs)
        if k == 1:
            return [self.rollout(T, actions, exo, out=outs[0], actions_in_domain=actions_in_domain, exo_in_domain=exo_in_domain)]
        if not 2 <= k <= _abi.MAX_FRAGMENTS:
            raise ValueError(f"rollout_fragments: 1 .. {_abi.MAX_FRAGMENTS} fragments per call, got {k}")
        key = ("frags", T, bool(actions_in_domain), bool(exo_in_domain)) + tuple(_sig(x) for o in outs for x in o[:8]) + (_sig(actions), _sig(exo))
        cached = self._rollout_io_cache.get(key)
        if cached is None:
            for o in outs:
                if o.msg_log is not None:
                    raise ValueError("rollout_fragments: plane fragments without message logs (alloc_trajectory(T))")
                self._check_rollout_planes(T, o)
            if any((o.terminations is None) != (outs[0].terminations is None) for o in outs):
                raise ValueError("rollout_fragments: `terminations` must be present in every fragment or in none")
            arr = (_abi.PhxRolloutFrag * k)()
            for i, o in enumerate(outs):
                self._set_planes(arr[i], o)
            io = self._rollout_io("rollout_fragments", k * T, actions, exo, actions_in_domain, exo_in_domain, outs[-1].last_obs)
            io.n_frag, io.frags = k, C.cast(arr, C.c_void_p)
            cached = (io, C.byref(io), arr, [o._replace(last_obs=None) for o in outs[:-1]] + [outs[-1]])
            self._cache_put(key, cached)
        self._check(self.lib.phx_rollout(self.handle, cached[1], self._stream()), "phx_rollout")
        return cached[3]

    # ---- per-env legacy-numpy MT19937 streams (ABI 7, PHX_F_MT19937) -------------------------------------------------
    def mt_seed(self, seeds):
        """``np.random.seed(seeds[b])`` for the stream of env instance b (32-bit integers)."""
        s = np.ascontiguousarray(np.asarray(seeds).astype(np.uint32)).reshape(-1)
        if s.size != self.B:
            raise ValueError(f"mt_seed: {s.size} seeds for {self.B} env instances")
        self._check(self.lib.phx_mt_seed(self.handle, s.ctypes.data, self._stream()), "phx_mt_seed")

    def mt_draw(self, T: int = 1, out=None):
        """The T * n_exo ``np.random.randint(5)`` calls each instance's reference worker makes in T steps, from the instance's own
        stream: u8 [T, B, n_exo] on the device, the layout phx_step (row t) and phx_rollout replay."""
        torch = _torch()
        if out is None:
            out = torch.empty((T, self.B, self.n_exo), dtype=torch.uint8, device=self.device)
        else:
            check_tensor("mt_draw", "out", out, torch.uint8, (T, self.B, self.n_exo), device=self.device)
        self._check(self.lib.phx_mt_draw(self.handle, out.data_ptr(), int(T), self._stream()), "phx_mt_draw")
        return out

    def pack_done_flags(self, traj: Trajectory):
        """bit-pack the done planes of a flat fragment into its ``packed_flags`` section (SURVEY 8e iii):
        word w, bit j = truncations.flat[64 w + j] != 0; a second block of words holds `terminations` unless
        the env's kinds never terminate.  One small launch on the current stream."""
        if traj.flat is None:
            raise ValueError("pack_done_flags needs a fragment from alloc_trajectory(flat=True)")
        n = traj.truncations.numel()
        words = (n + 63) // 64
        pf = traj.packed_flags.view(-1)
        self.pack_flags(traj.truncations, pf)
        if pf.numel() >= 2 * words * 8:
            self.pack_flags(traj.terminations, pf[words * 8:])

    def pack_flags(self, plane, dst):
        """u8 plane [n] (any shape, contiguous) -> ceil(n / 64) little-endian 64-bit words at the start of the u8 tensor ``dst``:
        word w, bit j = plane.flat[64 w + j] != 0.  One small launch on the current stream."""
        n = plane.numel()
        self._check(self.lib.phx_pack_flags(plane.data_ptr(), dst.data_ptr(), n, self._stream()), "phx_pack_flags")

    def unpack_flags(self, packed, n: int, out=None):
        """inverse of the packing above: u8 [n] (0 / 1) from ceil(n / 64) little-endian 64-bit words."""
        torch = _torch()
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._check(self.lib.phx_unpack_flags(packed.data_ptr(), out.data_ptr(), n, self._stream()),
                    "phx_unpack_flags")
        return out

    def gae(self, rewards, truncations, vf_pred=None, vf_next=None, terminations=None, gamma: float = 0.99,
            lambda_: float = 1.0, out=None):
        """``(advantages, value_targets)`` of a time-major fragment in ONE launch on the current stream (phx_gae,
        include/phantom_amd_gae.h): RLlib's ``compute_advantages(use_gae=True)`` for every (env instance, agent) column at
        once.  All tensors are ``[T, B, S]`` (or ``[T, N]``) on the env's device: ``rewards`` f32 and ``truncations`` u8 as a
        rollout wrote them (slices of longer recordings are fine), ``vf_pred`` f32 = V(the observation the policy acted on),
        ``vf_next`` f32 = V(new_obs[t]), read only where a trajectory is cut without terminating (a truncation, the fragment's
        last row), ``terminations`` u8; a missing value plane reads as 0 (``vf_pred=None, lambda_=1``: discounted returns), a
        missing ``terminations`` as all zero.  ``out``: the two f32 result tensors, 16-byte aligned (allocated here when None).
        Plain envs: there are no validity planes (FSM / Stackelberg dicts omit keys)."""
        torch = _torch()
        f32, u8 = torch.float32, torch.uint8
        if rewards is None or rewards.dim() < 2:
            raise ValueError("gae: `rewards` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(rewards.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"gae: `rewards` has shape {shape}: T and N must be >= 1")
        if not (0.0 <= gamma <= 1.0 and 0.0 <= lambda_ <= 1.0):
            raise ValueError(f"gae: gamma = {gamma} and lambda_ = {lambda_} must lie in [0, 1]")
        check_tensor("gae", "rewards", rewards, f32, shape, device=self.device)
        check_tensor("gae", "truncations", truncations, u8, shape, device=self.device)
        for name, x, dtype in (("vf_pred", vf_pred, f32), ("vf_next", vf_next, f32), ("terminations", terminations, u8)):
            if x is not None:
                check_tensor("gae", name, x, dtype, shape, device=self.device)
        if out is None:
            out = (torch.empty(shape, dtype=f32, device=self.device), torch.empty(shape, dtype=f32, device=self.device))
        adv, vt = out
        check_tensor("gae", "out[0]", adv, f32, shape, align=16, device=self.device)
        check_tensor("gae", "out[1]", vt, f32, shape, align=16, device=self.device)
        io = _abi.PhxGaeIO(T=T, N=N, gamma=gamma, lambda_=lambda_, reward=_ptr(rewards), vf_pred=_ptr(vf_pred), vf_next=_ptr(vf_next),
                           terminated=_ptr(terminations), truncated=_ptr(truncations), advantage=_ptr(adv), value_target=_ptr(vt))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_gae(C.byref(io), self._stream()), "phx_gae")
        return adv, vt

    def gae_masked(self, rewards, truncations, vf_pred=None, vf_next=None, terminations=None, acted=None, reward_valid=None,
                   gamma: float = 0.99, lambda_: float = 1.0, out=None):
        """``(advantages, value_targets, trajectory_rewards)`` of a time-major fragment whose per-agent trajectories have holes
        (FSM / Stackelberg envs), in ONE launch on the current stream (phx_gae_masked, include/phantom_amd_gae.h).  The planes are
        ``gae()``'s, plus ``acted`` u8 (!= 0: the agent held an observation and acted at step t -- a trajectory row) and
        ``reward_valid`` u8 as a rollout wrote it (only the value 1 counts); each missing one reads as all one.  At a trajectory row
        ``trajectory_rewards`` is the sum of the rewards that arrived from that row until the agent's next trajectory row or the first
        cut row (a done flag, the fragment's last row), whichever comes first; that cut row's ``terminations`` flag and ``vf_next``
        element give the bootstrap value, and the advantage chain links trajectory rows only.  Rows that are no trajectory rows
        hold +0.0 in all three results.  ``vf_pred`` is read at trajectory rows only, ``rewards`` where ``reward_valid == 1``,
        ``vf_next`` at the closing cut rows.  ``out``: the three f32 result tensors, 16-byte aligned (allocated here when None)."""
        torch = _torch()
        f32, u8 = torch.float32, torch.uint8
        if rewards is None or rewards.dim() < 2:
            raise ValueError("gae_masked: `rewards` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(rewards.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"gae_masked: `rewards` has shape {shape}: T and N must be >= 1")
        if not (0.0 <= gamma <= 1.0 and 0.0 <= lambda_ <= 1.0):
            raise ValueError(f"gae_masked: gamma = {gamma} and lambda_ = {lambda_} must lie in [0, 1]")
        check_tensor("gae_masked", "rewards", rewards, f32, shape, device=self.device)
        check_tensor("gae_masked", "truncations", truncations, u8, shape, device=self.device)
        for name, x, dtype in (("vf_pred", vf_pred, f32), ("vf_next", vf_next, f32), ("terminations", terminations, u8),
                               ("acted", acted, u8), ("reward_valid", reward_valid, u8)):
            if x is not None:
                check_tensor("gae_masked", name, x, dtype, shape, device=self.device)
        if out is None:
            out = tuple(torch.empty(shape, dtype=f32, device=self.device) for _ in range(3))
        adv, vt, rs = out
        for i, x in enumerate(out):
            check_tensor("gae_masked", f"out[{i}]", x, f32, shape, align=16, device=self.device)
        io = _abi.PhxGaeMaskedIO(T=T, N=N, gamma=gamma, lambda_=lambda_, reward=_ptr(rewards), vf_pred=_ptr(vf_pred), vf_next=_ptr(vf_next),
                                 terminated=_ptr(terminations), truncated=_ptr(truncations), acted=_ptr(acted),
                                 reward_valid=_ptr(reward_valid), advantage=_ptr(adv), value_target=_ptr(vt), reward_sum=_ptr(rs))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_gae_masked(C.byref(io), self._stream()), "phx_gae_masked")
        return adv, vt, rs

    def vtrace(self, rewards, truncations, vf_pred, behaviour_logp, target_logp, vf_next=None, terminations=None,
               gamma: float = 0.99, lambda_: float = 1.0, clip_rho_threshold: float = 1.0, clip_c_threshold: float = 1.0,
               clip_pg_rho_threshold: float = 1.0, out=None):
        """``(vs, pg_advantages)`` of a time-major fragment in ONE launch on the current stream (phx_vtrace,
        include/phantom_amd_vtrace.h): the V-trace value targets and policy-gradient advantages of IMPALA / APPO (RLlib's
        ``vtrace_torch.from_importance_weights``) for every (env instance, agent) column at once.  All tensors are ``[T, B, S]`` (or
        ``[T, N]``) on the env's device: ``rewards`` f32 and ``truncations`` u8 as a rollout wrote them, ``vf_pred`` f32 = V(the
        observation the policy acted on), ``behaviour_logp`` f32 = the rollout's ``action_logp``, ``target_logp`` f32 = the learner's
        log-density of the same draws (the same tensor is allowed: on-policy), ``vf_next`` f32 = V(new_obs[t]), read only where a
        trajectory is cut without terminating (a truncation, the fragment's last row; missing: 0), ``terminations`` u8 (missing: all
        zero).  The importance ratio is exp of the log-ratio clamped to [-20, 20]; the three thresholds clip it for the TD term, the
        trace and the advantage.  ``out``: the two f32 result tensors, 16-byte aligned (allocated here when None)."""
        torch = _torch()
        f32, u8 = torch.float32, torch.uint8
        if rewards is None or rewards.dim() < 2:
            raise ValueError("vtrace: `rewards` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(rewards.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"vtrace: `rewards` has shape {shape}: T and N must be >= 1")
        if not (0.0 <= gamma <= 1.0 and 0.0 <= lambda_ <= 1.0):
            raise ValueError(f"vtrace: gamma = {gamma} and lambda_ = {lambda_} must lie in [0, 1]")
        clips = [float(np.float32(x)) for x in (clip_rho_threshold, clip_c_threshold, clip_pg_rho_threshold)]      # (as the struct holds them)
        if not all(np.isfinite(x) and x > 0.0 for x in clips):
            raise ValueError(f"vtrace: clip_rho_threshold = {clip_rho_threshold}, clip_c_threshold = {clip_c_threshold} and "
                             f"clip_pg_rho_threshold = {clip_pg_rho_threshold} must be finite and > 0")
        check_tensor("vtrace", "rewards", rewards, f32, shape, device=self.device)
        check_tensor("vtrace", "truncations", truncations, u8, shape, device=self.device)
        for name, x in (("vf_pred", vf_pred), ("behaviour_logp", behaviour_logp), ("target_logp", target_logp)):
            check_tensor("vtrace", name, x, f32, shape, device=self.device)
        for name, x, dtype in (("vf_next", vf_next, f32), ("terminations", terminations, u8)):
            if x is not None:
                check_tensor("vtrace", name, x, dtype, shape, device=self.device)
        if out is None:
            out = (torch.empty(shape, dtype=f32, device=self.device), torch.empty(shape, dtype=f32, device=self.device))
        vs, pg = out
        check_tensor("vtrace", "out[0]", vs, f32, shape, align=16, device=self.device)
        check_tensor("vtrace", "out[1]", pg, f32, shape, align=16, device=self.device)
        io = _abi.PhxVtraceIO(T=T, N=N, gamma=gamma, lambda_=lambda_, rho_bar=clips[0], c_bar=clips[1], pg_rho_bar=clips[2],
                              reward=_ptr(rewards), vf_pred=_ptr(vf_pred), vf_next=_ptr(vf_next), behaviour_logp=_ptr(behaviour_logp),
                              target_logp=_ptr(target_logp), terminated=_ptr(terminations), truncated=_ptr(truncations), vs=_ptr(vs),
                              pg_advantage=_ptr(pg))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_vtrace(C.byref(io), self._stream()), "phx_vtrace")
        return vs, pg

    def traj_next(self, truncations, terminations=None, acted=None, new_obs_valid=None, obs=None, new_obs=None, out=None):
        """``(next_row, next_terminated, next_truncated, next_obs or None)`` of a time-major fragment whose per-agent trajectories have
        holes (FSM / Stackelberg envs), on the current stream (phx_traj_next, include/phantom_amd_traj.h): what a learner that reads
        one agent's transitions needs next to ``gae_masked``'s ``trajectory_rewards``, over the same segments.  The flag planes are
        ``[T, B, S]`` (or ``[T, N]``) u8 on the env's device: ``truncations`` / ``terminations`` as a rollout wrote them (slices of
        longer recordings are fine), ``acted`` (!= 0: a trajectory row, as in ``gae_masked``) and ``new_obs_valid`` (the rollout's
        ``obs_valid`` plane: != 0, step t returned an observation to the agent); a missing ``terminations`` reads as all zero, a
        missing ``acted`` or ``new_obs_valid`` as all one.  At a trajectory row ``next_row`` (i32) is the latest row of the agent's
        segment -- up to its next trajectory row or the first done flag, whichever comes first -- whose ``new_obs`` the agent received
        (-1: none, it still holds ``obs`` of the row itself), and the two u8 flags are those of the row that closed the segment
        (terminated wins over truncated; the fragment's last row without a flag sets neither).  With ``obs`` and ``new_obs`` (f32
        ``[T, B, S, D]``, D <= 64; both or neither) a second launch gathers ``next_obs`` = ``new_obs[next_row]``, or ``obs`` of the
        row itself where ``next_row`` is -1, bit for bit.  Rows that are no trajectory rows hold -1, 0, 0 and +0.0.  A trajectory row
        is a complete transition iff one of its flags is set or ``next_row >= 0``.  ``out``: the four result tensors (the last one
        None without ``obs``), 16-byte aligned (allocated here when None)."""
        torch = _torch()
        f32, u8, i32 = torch.float32, torch.uint8, torch.int32
        if truncations is None or not hasattr(truncations, "dim") or truncations.dim() < 2:
            raise ValueError("traj_next: `truncations` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(truncations.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"traj_next: `truncations` has shape {shape}: T and N must be >= 1")
        check_tensor("traj_next", "truncations", truncations, u8, shape, device=self.device)
        for name, x in (("terminations", terminations), ("acted", acted), ("new_obs_valid", new_obs_valid)):
            if x is not None:
                check_tensor("traj_next", name, x, u8, shape, device=self.device)
        if (obs is None) != (new_obs is None):
            raise ValueError("traj_next: `obs` and `new_obs` come together (both for `next_obs`, neither without it)")
        gather, D = obs is not None, 0
        if gather:
            if not hasattr(obs, "dim") or obs.dim() != len(shape) + 1 or not 1 <= obs.shape[-1] <= 64:
                raise ValueError(f"traj_next: `obs` must be a {shape + ('D',)} tensor with 1 <= D <= 64")
            D = int(obs.shape[-1])
            check_tensor("traj_next", "obs", obs, f32, shape + (D,), device=self.device)
            check_tensor("traj_next", "new_obs", new_obs, f32, shape + (D,), device=self.device)
        if out is None:
            e = lambda s, dtype: torch.empty(s, dtype=dtype, device=self.device)
            out = (e(shape, i32), e(shape, u8), e(shape, u8), e(shape + (D,), f32) if gather else None)
        if len(out) != 4:
            raise ValueError("traj_next: `out` is (next_row, next_terminated, next_truncated, next_obs or None)")
        nr, nte, ntr, nob = out
        check_tensor("traj_next", "out[0]", nr, i32, shape, align=16, device=self.device)
        check_tensor("traj_next", "out[1]", nte, u8, shape, align=16, device=self.device)
        check_tensor("traj_next", "out[2]", ntr, u8, shape, align=16, device=self.device)
        if gather:
            check_tensor("traj_next", "out[3]", nob, f32, shape + (D,), align=16, device=self.device)
        elif nob is not None:
            raise ValueError("traj_next: `out[3]` (next_obs) needs `obs` and `new_obs`")
        io = _abi.PhxTrajNextIO(T=T, D=D, N=N, truncated=_ptr(truncations), terminated=_ptr(terminations), acted=_ptr(acted),
                                new_obs_valid=_ptr(new_obs_valid), obs=_ptr(obs), new_obs=_ptr(new_obs), next_row=_ptr(nr),
                                next_terminated=_ptr(nte), next_truncated=_ptr(ntr), next_obs=_ptr(nob))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_traj_next(C.byref(io), self._stream()), "phx_traj_next")
        return nr, nte, ntr, nob

    def nstep(self, rewards, truncations, terminations=None, acted=None, next_row=None, next_obs=None, n: int = 3, gamma: float = 0.99,
              out=None):
        """``(nstep_rewards, nstep_discounts, nstep_last, nstep_terminateds, nstep_truncateds, nstep_next_row, nstep_next_obs or None)``:
        the n-step transitions of a time-major fragment for a replay learner (RLlib's ``adjust_nstep``, over trajectories with holes as
        well), on the current stream (phx_nstep, include/phantom_amd_nstep.h).  The inputs describe one TRANSITION per trajectory row:
        on an FSM / Stackelberg env ``rewards`` is ``gae_masked``'s ``trajectory_rewards`` and ``truncations`` / ``terminations`` /
        ``next_row`` / ``next_obs`` are ``traj_next``'s four results, with the same ``acted``; on a plain env they are the rollout's own
        ``rewards`` / ``truncations`` / ``terminations`` / ``observations`` planes and ``acted`` and ``next_row`` stay None.  Planes are
        ``[T, B, S]`` (or ``[T, N]``) on the env's device -- ``rewards`` f32, the flags and ``acted`` u8, ``next_row`` i32 -- and
        ``next_obs`` f32 ``[T, B, S, D]``, D <= 64; slices of longer recordings are fine.  At a row where the agent acted the call folds
        the rewards of up to ``n`` of the agent's consecutive transitions, ``r0 + gamma r1 + ..`` (f32 ``fmaf`` chain), stopping after a
        transition with a done flag, at the agent's last trajectory row, and before a transition that is incomplete (``next_row`` -1
        without a flag; an incomplete row itself folds only its own reward); ``nstep_discounts`` is gamma to the number of transitions
        folded, ``nstep_last`` (i32) the row of the last one, the two u8 flags and ``nstep_next_row`` (i32) are that row's, and
        ``nstep_next_obs`` (only with ``next_obs``; a further launch) its ``next_obs`` bit for bit: the learner's target is
        ``nstep_rewards + nstep_discounts * (1 - nstep_terminateds) * Q(nstep_next_obs)``.  Rows that are no trajectory rows hold +0.0,
        +0.0, -1, 0, 0, -1 and +0.0.  ``n`` in [1, 64] (1: the inputs themselves), ``gamma`` in [0, 1].  ``out``: the seven result
        tensors (the last one None without ``next_obs``), 16-byte aligned, optionally followed by an eighth, the i32 ``[T, B, S]`` scratch
        that receives every row's next trajectory row (``succ_row``, used with ``acted`` only); whatever is missing is allocated here
        with ``torch.empty`` -- the caching allocator's stream-ordered reuse makes a per-call scratch safe, and a caller that captures the
        call into a graph or wants no allocation passes all eight.  The call does not synchronise."""
        torch = _torch()
        f32, u8, i32 = torch.float32, torch.uint8, torch.int32
        if rewards is None or not hasattr(rewards, "dim") or rewards.dim() < 2:
            raise ValueError("nstep: `rewards` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(rewards.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"nstep: `rewards` has shape {shape}: T and N must be >= 1")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= _abi.NSTEP_MAX_N:
            raise ValueError(f"nstep: n = {n!r} must be an int in [1, {_abi.NSTEP_MAX_N}]")
        if not 0.0 <= float(np.float32(gamma)) <= 1.0:           # (as the struct holds it; NaN fails both comparisons)
            raise ValueError(f"nstep: gamma = {gamma} must lie in [0, 1]")
        check_tensor("nstep", "rewards", rewards, f32, shape, device=self.device)
        check_tensor("nstep", "truncations", truncations, u8, shape, device=self.device)
        for name, x, dtype in (("terminations", terminations, u8), ("acted", acted, u8), ("next_row", next_row, i32)):
            if x is not None:
                check_tensor("nstep", name, x, dtype, shape, device=self.device)
        gather, D = next_obs is not None, 0
        if gather:
            if not hasattr(next_obs, "dim") or next_obs.dim() != len(shape) + 1 or not 1 <= next_obs.shape[-1] <= 64:
                raise ValueError(f"nstep: `next_obs` must be a {shape + ('D',)} tensor with 1 <= D <= 64")
            D = int(next_obs.shape[-1])
            check_tensor("nstep", "next_obs", next_obs, f32, shape + (D,), device=self.device)
        e = lambda s, dtype: torch.empty(s, dtype=dtype, device=self.device)
        if out is None:
            out = (e(shape, f32), e(shape, f32), e(shape, i32), e(shape, u8), e(shape, u8), e(shape, i32), e(shape + (D,), f32) if gather else None)
        if len(out) not in (7, 8):
            raise ValueError("nstep: `out` is (nstep_rewards, nstep_discounts, nstep_last, nstep_terminateds, nstep_truncateds, "
                             "nstep_next_row, nstep_next_obs or None[, succ_row])")
        res, succ = tuple(out[:7]), (out[7] if len(out) == 8 else None)
        for i, (x, dtype) in enumerate(zip(res[:6], (f32, f32, i32, u8, u8, i32))):
            check_tensor("nstep", f"out[{i}]", x, dtype, shape, align=16, device=self.device)
        if gather:
            check_tensor("nstep", "out[6]", res[6], f32, shape + (D,), align=16, device=self.device)
        elif res[6] is not None:
            raise ValueError("nstep: `out[6]` (nstep_next_obs) needs `next_obs`")
        if succ is not None:
            check_tensor("nstep", "out[7]", succ, i32, shape, align=16, device=self.device)
        elif acted is not None:
            succ = e(shape, i32)
        io = _abi.PhxNstepIO(T=T, D=D, N=N, n=int(n), gamma=gamma, reward=_ptr(rewards), truncated=_ptr(truncations),
                             terminated=_ptr(terminations), acted=_ptr(acted), next_row=_ptr(next_row), next_obs=_ptr(next_obs),
                             succ_row=_ptr(succ), nstep_reward=_ptr(res[0]), nstep_discount=_ptr(res[1]), nstep_last=_ptr(res[2]),
                             nstep_terminated=_ptr(res[3]), nstep_truncated=_ptr(res[4]), nstep_next_row=_ptr(res[5]),
                             nstep_next_obs=_ptr(res[6]))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_nstep(C.byref(io), self._stream()), "phx_nstep")
        return res

    def episode_stats(self, rewards, truncations, terminations=None, acted=None, reward_valid=None, group: int = 1, classes: int = 1,
                      carry=None, planes: bool = False, summary: bool = True, out=None):
        """``(col_stats, summary or None, episode_return or None, episode_len or None)``: the returns and lengths of the episodes that
        close inside a time-major fragment, on the current stream (phx_episode_stats, include/phantom_amd_episodes.h).  Planes are
        ``[T, B, S]`` (or ``[T, N]``) on the env's device -- ``rewards`` f32, the flags, ``acted`` and ``reward_valid`` u8, as a rollout
        wrote them; slices of longer recordings are fine; a missing ``terminations`` reads as all zero, a missing ``acted`` or
        ``reward_valid`` as all one (a plain env).  ``group`` consecutive input columns form an output column (1: one per (env
        instance, agent); S: one per env instance, RLlib's episode -- it closes in the row where every member carries a flag), C =
        N / group of them, and output column c belongs to class c % ``classes``.  ``carry`` is a ``(f32 [C], i32 [C])`` pair of device
        tensors holding each output column's open episode (return so far, length so far; -1: none open), read and updated in place:
        an episode a fragment cuts is finished by the next call.  None: every column starts with no episode open and what is open at
        the end is dropped.  ``col_stats`` is uint8 ``[C, 48]`` and ``summary`` (``summary=True``; a second launch) uint8
        ``[classes, 48]``: records of ``_abi.EPISODE_STATS_DTYPE`` (count, len_sum, ret_sum, ret_sumsq, ret_min, ret_max, len_min,
        len_max) of the episodes THIS call closed, per output column and per class; a host copy is viewed with
        ``.numpy().view(_abi.EPISODE_STATS_DTYPE)``.  With ``planes=True`` ``episode_return`` (f32) and ``episode_len`` (i32), both
        ``[T, C]``, hold the return and length at the rows that close an episode and +0.0 / -1 elsewhere.  ``out``: the same four,
        caller-owned and 16-byte aligned (None where a result is not wanted: ``planes`` and ``summary`` are then read from it);
        allocated here when None.  The call does not synchronise."""
        torch = _torch()
        f32, u8, i32 = torch.float32, torch.uint8, torch.int32
        if rewards is None or not hasattr(rewards, "dim") or rewards.dim() < 2:
            raise ValueError("episode_stats: `rewards` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(rewards.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"episode_stats: `rewards` has shape {shape}: T and N must be >= 1")
        for name, v, hi in (("group", group, _abi.EPISODE_MAX_G), ("classes", classes, None)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or (hi is not None and v > hi):
                raise ValueError(f"episode_stats: {name} = {v!r} must be an int >= 1" + (f" and <= {hi}" if hi else ""))
        if N % group:
            raise ValueError(f"episode_stats: group = {group} must divide the {N} input columns")
        Cn = N // int(group)
        if Cn % classes or classes >= 2 ** 31:
            raise ValueError(f"episode_stats: classes = {classes} must divide the {Cn} output columns")
        check_tensor("episode_stats", "rewards", rewards, f32, shape, device=self.device)
        check_tensor("episode_stats", "truncations", truncations, u8, shape, device=self.device)
        for name, x in (("terminations", terminations), ("acted", acted), ("reward_valid", reward_valid)):
            if x is not None:
                check_tensor("episode_stats", name, x, u8, shape, device=self.device)
        cr = cl = None
        if carry is not None:
            if len(carry) != 2:
                raise ValueError("episode_stats: `carry` is a (f32 [C], i32 [C]) pair of device tensors")
            cr, cl = carry
            check_tensor("episode_stats", "carry[0]", cr, f32, (Cn,), device=self.device)
            check_tensor("episode_stats", "carry[1]", cl, i32, (Cn,), device=self.device)
        nb = _abi.EPISODE_STATS_BYTES
        e = lambda s, dtype: torch.empty(s, dtype=dtype, device=self.device)
        if out is None:
            out = (e((Cn, nb), u8), e((int(classes), nb), u8) if summary else None, e((T, Cn), f32) if planes else None,
                   e((T, Cn), i32) if planes else None)
        if len(out) != 4:
            raise ValueError("episode_stats: `out` is (col_stats, summary or None, episode_return or None, episode_len or None)")
        col, summ, eret, elen = out
        check_tensor("episode_stats", "out[0]", col, u8, (Cn, nb), align=16, device=self.device)
        if summ is not None:
            check_tensor("episode_stats", "out[1]", summ, u8, (int(classes), nb), align=16, device=self.device)
        if eret is not None:
            check_tensor("episode_stats", "out[2]", eret, f32, (T, Cn), align=16, device=self.device)
        if elen is not None:
            check_tensor("episode_stats", "out[3]", elen, i32, (T, Cn), align=16, device=self.device)
        io = _abi.PhxEpisodeIO(T=T, G=int(group), N=N, K=int(classes), reward=_ptr(rewards), truncated=_ptr(truncations),
                               terminated=_ptr(terminations), acted=_ptr(acted), reward_valid=_ptr(reward_valid), carry_return=_ptr(cr),
                               carry_len=_ptr(cl), episode_return=_ptr(eret), episode_len=_ptr(elen), col_stats=_ptr(col),
                               summary=_ptr(summ))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_episode_stats(C.byref(io), self._stream()), "phx_episode_stats")
        return col, summ, eret, elen

    def compact(self, keep, planes, capacity=None, out=None):
        """``(start, out_row, out_col, {name: dense tensor})``: the kept elements of time-major planes, dense and in (column, row) =
        (env instance, agent, step) order, on the current stream (phx_traj_compact, include/phantom_amd_compact.h) -- the hole rows of
        an FSM / Stackelberg fragment dropped on the device, fused with the transpose ``to_sample_batches()``'s row order needs.
        ``keep`` is u8 ``[T, B, S]`` (or ``[T, N]``), != 0 keeps the element; ``planes`` maps a name to a tensor ``[T, N..]`` (u8, f32,
        i32) or ``[T, N.., w]`` (f32, i32; w <= 64) on the env's device -- slices of longer recordings are fine.  ``start`` i64
        ``[N + 1]`` holds every column's first position and, in ``start[N]``, the number K of kept elements; ``out_row`` / ``out_col``
        i32 ``[capacity]`` the row and column of every position; a dense tensor is ``[capacity]`` or ``[capacity, w]``.  Only the first
        ``min(K, capacity)`` elements of them are written (``capacity`` defaults to T * N: everything fits), the caller reads K from
        ``start[N]`` -- the call does not synchronise.  ``out``: the same four, caller-owned and 16-byte aligned (``out_row`` /
        ``out_col`` may be None there: not written); allocated here when None.  More than 16 planes are served by further launches of
        up to 16 planes each, and each of them counts and scans ``keep`` again (T * N bytes read and one scan of N + 1 entries)."""
        torch = _torch()
        f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
        if keep is None or not hasattr(keep, "dim") or keep.dim() < 2:
            raise ValueError("compact: `keep` must be a [T, B, S] (or [T, N]) tensor")
        shape = tuple(keep.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"compact: `keep` has shape {shape}: T and N must be >= 1")
        check_tensor("compact", "keep", keep, u8, shape, device=self.device)
        capacity = T * N if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"compact: capacity = {capacity} must be >= 0")
        planes = dict(planes)
        words = {}
        for name, x in planes.items():
            if x is None or not hasattr(x, "dim") or x.dim() not in (len(shape), len(shape) + 1):
                raise ValueError(f"compact: plane `{name}` must be a {shape} or {shape + ('w',)} tensor")
            tail = tuple(x.shape[len(shape):])
            if tail and (x.dtype == u8 or not 1 <= tail[0] <= 64):
                raise ValueError(f"compact: plane `{name}`: a trailing axis needs f32 or i32 and 1 <= w <= 64")
            check_tensor("compact", f"plane `{name}`", x, (u8, f32, i32), shape + tail, device=self.device)
            words[name] = tail
        e = lambda s, dtype: torch.empty(s, dtype=dtype, device=self.device)
        if out is None:
            out = (e((N + 1,), i64), e((capacity,), i32), e((capacity,), i32), {k: e((capacity,) + words[k], x.dtype) for k, x in planes.items()})
        if len(out) != 4 or set(out[3]) != set(planes):
            raise ValueError("compact: `out` is (start, out_row or None, out_col or None, {name: dense tensor}) with the planes' names")
        start, orow, ocol, dense = out
        check_tensor("compact", "out[0]", start, i64, (N + 1,), align=16, device=self.device)
        for i, x in ((1, orow), (2, ocol)):
            if x is not None:
                check_tensor("compact", f"out[{i}]", x, i32, (capacity,), align=16, device=self.device)
        for name, x in planes.items():
            check_tensor("compact", f"out[3][`{name}`]", dense[name], x.dtype, (capacity,) + words[name], align=16, device=self.device)
        names = list(planes)
        with torch.cuda.device(self.device):
            for first in range(0, max(len(names), 1), _abi.COMPACT_MAX_PLANES):
                part = names[first:first + _abi.COMPACT_MAX_PLANES]
                io = _abi.PhxTrajCompactIO(T=T, n_planes=len(part), N=N, capacity=capacity, keep=_ptr(keep), start=_ptr(start),
                                           out_row=_ptr(orow) if first == 0 else None, out_col=_ptr(ocol) if first == 0 else None)
                for k, name in enumerate(part):
                    io.plane[k] = _abi.PhxCompactPlane(src=_ptr(planes[name]), dst=_ptr(dense[name]),
                                                       elem_bytes=planes[name].element_size() * int(np.prod(words[name])), reserved=0)
                self._check(self.lib.phx_traj_compact(C.byref(io), self._stream()), "phx_traj_compact")
        return start, orow, ocol, dense

    def _batch_planes(self, fn, planes, keep, col_class, class_id, standardize, seed, epoch, row_words, lead_dims):
        """the arguments ``train_batch`` and ``seq_batch`` share, checked: ``(planes, shape, T, N, S, layout, row_words, std_plane)``"""
        torch = _torch()
        f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
        planes = dict(planes)
        if len(planes) > _abi.BATCH_MAX_PLANES:
            raise ValueError(f"{fn}: {len(planes)} planes, at most {_abi.BATCH_MAX_PLANES} fit one call")
        lead = keep if keep is not None else min((x for x in planes.values() if hasattr(x, "dim")), key=lambda x: x.dim(), default=None)
        if lead is None or not hasattr(lead, "dim") or lead.dim() < 2:
            raise ValueError(f"{fn}: `keep` or a plane must give the leading shape [T, B, S] (or [T, N])")
        if keep is None and lead_dims is not None:
            if isinstance(lead_dims, bool) or not isinstance(lead_dims, (int, np.integer)) or not 2 <= lead_dims <= lead.dim():
                raise ValueError(f"{fn}: lead_dims = {lead_dims!r} must be an int in [2, {lead.dim()}]")
            shape = tuple(lead.shape[:lead_dims])
        else:
            shape = tuple(lead.shape)
        T, N = shape[0], int(np.prod(shape[1:]))
        if T < 1 or N < 1:
            raise ValueError(f"{fn}: the leading shape is {shape}: T and N must be >= 1")
        if keep is not None:
            check_tensor(fn, "keep", keep, u8, shape, device=self.device)
        S = 1
        if col_class is not None:
            if not hasattr(col_class, "dim") or col_class.dim() != 1 or col_class.numel() < 1 or N % col_class.numel():
                raise ValueError(f"{fn}: `col_class` must be a u8 [S] tensor with S >= 1 dividing the {N} columns")
            S = col_class.numel()
            check_tensor(fn, "col_class", col_class, u8, (S,), device=self.device)
        if isinstance(class_id, bool) or not isinstance(class_id, (int, np.integer)) or not 0 <= class_id <= 255:
            raise ValueError(f"{fn}: class_id = {class_id!r} must be an int in [0, 255]")
        for name, v in (("seed", seed), ("epoch", epoch)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 64:
                raise ValueError(f"{fn}: {name} = {v!r} must be an int in [0, 2^64)")
        layout, off = {}, 0
        for name, x in planes.items():
            if x is None or not hasattr(x, "dim") or x.dim() not in (len(shape), len(shape) + 1):
                raise ValueError(f"{fn}: plane `{name}` must be a {shape} or {shape + ('w',)} tensor")
            tail = tuple(x.shape[len(shape):])
            if tail and (x.dtype == u8 or not 1 <= tail[0] <= 64):
                raise ValueError(f"{fn}: plane `{name}`: a trailing axis needs f32 or i32 and 1 <= w <= 64")
            check_tensor(fn, f"plane `{name}`", x, (u8, f32, i32), shape + tail, device=self.device)
            w = tail[0] if tail else 1
            layout[name] = (off, w, x.dtype)
            off += w
        if row_words is None:
            row_words = max(16, -(-off // 16) * 16)
        if isinstance(row_words, bool) or not isinstance(row_words, (int, np.integer)) or not 4 <= row_words <= 256 or row_words % 4 or off > row_words:
            raise ValueError(f"{fn}: row_words = {row_words!r} must be a multiple of 4 in [4, 256] that holds the planes' {off} words")
        std_plane = -1
        if standardize is not None:
            if standardize not in planes or planes[standardize].dtype != f32 or planes[standardize].dim() != len(shape):
                raise ValueError(f"{fn}: standardize = {standardize!r} must name an f32 plane without a trailing axis")
            std_plane = list(planes).index(standardize)
        return planes, shape, T, N, S, layout, int(row_words), std_plane

    def train_batch(self, planes, keep=None, col_class=None, class_id: int = 0, standardize=None, shuffle: bool = True, seed: int = 0,
                    epoch: int = 0, row_words=None, capacity=None, out=None, lead_dims=None):
        """``(start, records, out_row, out_col, moments, layout)``: a learner's batch from time-major planes, on the current stream
        (phx_train_batch, include/phantom_amd_batch.h) -- the kept elements in (env instance, agent, step) order, one class of
        columns, one plane standardized, the rows shuffled by ``(seed, epoch)``, written as records: all columns of a row contiguous.
        ``planes`` maps a name to a tensor ``[T, N..]`` (u8, f32, i32) or ``[T, N.., w]`` (f32, i32; w <= 64) on the env's device, at
        most 32 of them; the leading shape ``[T, N..]`` is ``keep``'s (u8, != 0 keeps the element), without ``keep`` the first
        ``lead_dims`` axes of the planes, and with neither the shape of the plane with the fewest dimensions.  ``col_class`` u8
        ``[S]`` (S divides N) with ``class_id`` keeps the columns n with ``col_class[n % S] == class_id``.  ``standardize`` names an f32 plane without a trailing axis: its kept values leave as
        ``(x - mean) / max(1e-4, std)``, and ``moments`` (uint8 ``[32]``, a record of ``_abi.BATCH_MOMENTS_DTYPE``) holds count, sum,
        sumsq, mean and den.  ``layout[name] = (word_off, w, dtype)``: the plane's 32-bit words ``[word_off, word_off + w)`` of a
        record (a u8 plane: one word, zero-extended); the planes are packed in order and ``row_words`` defaults to their words rounded
        up to a multiple of 16, whole 64-byte units.  ``records`` is i32 ``[capacity, row_words]``, ``out_row`` / ``out_col`` i32
        ``[capacity]`` (``capacity`` defaults to T * N), ``start`` i64 ``[N + 1]`` with K, the number of records, in ``start[N]``:
        records ``[0, K)`` are written, or NOTHING but ``start`` and ``moments`` when K > capacity -- the caller compares; the call
        does not synchronise.  ``out``: ``(start, records, out_row or None, out_col or None, moments, workspace)``, caller-owned and
        16-byte aligned, ``workspace`` f64 ``[N, 2]``, the last two None without ``standardize``; allocated here when None."""
        torch = _torch()
        f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
        planes, shape, T, N, S, layout, row_words, std_plane = self._batch_planes("train_batch", planes, keep, col_class, class_id, standardize,
                                                                                  seed, epoch, row_words, lead_dims)
        capacity = T * N if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"train_batch: capacity = {capacity} must be >= 0")
        e = lambda s, dtype: torch.empty(s, dtype=dtype, device=self.device)
        if out is None:
            out = (e((N + 1,), i64), e((capacity, int(row_words)), i32), e((capacity,), i32), e((capacity,), i32),
                   e((_abi.BATCH_MOMENTS_BYTES,), u8) if std_plane >= 0 else None, e((N, 2), torch.float64) if std_plane >= 0 else None)
        if len(out) != 6:
            raise ValueError("train_batch: `out` is (start, records, out_row or None, out_col or None, moments or None, workspace or None)")
        start, records, orow, ocol, moments, workspace = out
        check_tensor("train_batch", "out[0]", start, i64, (N + 1,), align=16, device=self.device)
        check_tensor("train_batch", "out[1]", records, i32, (capacity, int(row_words)), align=16, device=self.device)
        for i, x in ((2, orow), (3, ocol)):
            if x is not None:
                check_tensor("train_batch", f"out[{i}]", x, i32, (capacity,), align=16, device=self.device)
        if std_plane >= 0:
            check_tensor("train_batch", "out[4]", moments, u8, (_abi.BATCH_MOMENTS_BYTES,), align=16, device=self.device)
            check_tensor("train_batch", "out[5]", workspace, torch.float64, (N, 2), align=16, device=self.device)
        elif moments is not None or workspace is not None:
            raise ValueError("train_batch: `out[4]` (moments) and `out[5]` (workspace) need `standardize`")
        io = _abi.PhxTrainBatchIO(T=T, N=N, capacity=capacity, n_planes=len(planes), row_words=int(row_words), S=S, class_id=int(class_id),
                                  std_plane=std_plane, shuffle=1 if shuffle else 0, seed=int(seed), epoch=int(epoch), keep=_ptr(keep),
                                  col_class=_ptr(col_class), start=_ptr(start), records=_ptr(records), out_row=_ptr(orow), out_col=_ptr(ocol),
                                  moments=_ptr(moments), workspace=_ptr(workspace))
        for k, (name, x) in enumerate(planes.items()):
            io.plane[k] = _abi.PhxBatchPlane(src=_ptr(x), elem_bytes=x.element_size() * layout[name][1], word_off=layout[name][0])
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_train_batch(C.byref(io), self._stream()), "phx_train_batch")
        return start, records, orow, ocol, moments, layout

    def seq_batch(self, planes, max_seq_len, keep=None, terminated=None, truncated=None, col_class=None, class_id: int = 0, standardize=None,
                  shuffle: bool = True, seed: int = 0, epoch: int = 0, row_words=None, capacity=None, out=None, lead_dims=None):
        """``(seq_start, records, seq_lens, seq_row, seq_col, out_row, out_col, moments, layout)``: a recurrent learner's batch from
        time-major planes, on the current stream (phx_seq_batch, include/phantom_amd_seq.h) -- ``train_batch``'s kept elements, every
        column's kept rows cut into sequences at a set ``terminated`` / ``truncated`` flag (u8 of the leading shape, read at kept
        elements only; None: all zero) and every ``max_seq_len`` = L rows, each sequence zero-padded to L, one plane standardized over
        the kept rows and the SEQUENCES shuffled by ``(seed, epoch)``.  ``planes``, ``keep``, ``col_class`` / ``class_id``,
        ``standardize``, ``row_words``, ``lead_dims`` and ``layout`` are ``train_batch``'s.  ``capacity`` counts sequences and defaults
        to N * ceil(T / L) without flag planes and to T * N (every row could close a sequence) with one.  ``records`` is i32 ``[capacity, L, row_words]``,
        ``out_row`` / ``out_col`` i32 ``[capacity, L]`` (-1 in padding), ``seq_lens`` / ``seq_row`` / ``seq_col`` i32 ``[capacity]``
        (a sequence's rows, its first fragment row and its column), ``seq_start`` i64 ``[N + 1]`` with Q, the number of sequences,
        in ``seq_start[N]``: sequences ``[0, Q)`` are written, or NOTHING but ``seq_start`` and ``moments`` when Q > capacity -- the
        caller compares; the call does not synchronise.  ``out``: ``(seq_start, records, seq_lens or None, seq_row or None, seq_col or
        None, out_row or None, out_col or None, moments, workspace)``, caller-owned and 16-byte aligned, ``workspace`` f64 ``[3, N]``,
        the last two None without ``standardize``; allocated here when None."""
        torch = _torch()
        f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
        if isinstance(max_seq_len, bool) or not isinstance(max_seq_len, (int, np.integer)) or not 1 <= max_seq_len <= _abi.SEQ_MAX_LEN:
            raise ValueError(f"seq_batch: max_seq_len = {max_seq_len!r} must be an int in [1, {_abi.SEQ_MAX_LEN}]")
        L = int(max_seq_len)
        planes, shape, T, N, S, layout, row_words, std_plane = self._batch_planes("seq_batch", planes, keep, col_class, class_id, standardize,
                                                                                  seed, epoch, row_words, lead_dims)
        for name, x in (("terminated", terminated), ("truncated", truncated)):
            if x is not None:
                check_tensor("seq_batch", name, x, u8, shape, device=self.device)
        if capacity is None:                                     # (the length cuts, and a flag per row where flags are given)
            capacity = N * -(-T // L) if terminated is None and truncated is None else T * N
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
            raise ValueError(f"seq_batch: capacity = {capacity!r} must be an int >= 0")
        capacity = int(capacity)
        e = lambda s, dtype: torch.empty(s, dtype=dtype, device=self.device)
        if out is None:
            out = (e((N + 1,), i64), e((capacity, L, int(row_words)), i32), e((capacity,), i32), e((capacity,), i32), e((capacity,), i32),
                   e((capacity, L), i32), e((capacity, L), i32), e((_abi.BATCH_MOMENTS_BYTES,), u8) if std_plane >= 0 else None,
                   e((3, N), torch.float64) if std_plane >= 0 else None)
        if len(out) != 9:
            raise ValueError("seq_batch: `out` is (seq_start, records, seq_lens or None, seq_row or None, seq_col or None, out_row or None, "
                             "out_col or None, moments or None, workspace or None)")
        start, records, lens, srow, scol, orow, ocol, moments, workspace = out
        check_tensor("seq_batch", "out[0]", start, i64, (N + 1,), align=16, device=self.device)
        check_tensor("seq_batch", "out[1]", records, i32, (capacity, L, int(row_words)), align=16, device=self.device)
        for i, x in ((2, lens), (3, srow), (4, scol)):
            if x is not None:
                check_tensor("seq_batch", f"out[{i}]", x, i32, (capacity,), align=16, device=self.device)
        for i, x in ((5, orow), (6, ocol)):
            if x is not None:
                check_tensor("seq_batch", f"out[{i}]", x, i32, (capacity, L), align=16, device=self.device)
        if std_plane >= 0:
            check_tensor("seq_batch", "out[7]", moments, u8, (_abi.BATCH_MOMENTS_BYTES,), align=16, device=self.device)
            check_tensor("seq_batch", "out[8]", workspace, torch.float64, (3, N), align=16, device=self.device)
        elif moments is not None or workspace is not None:
            raise ValueError("seq_batch: `out[7]` (moments) and `out[8]` (workspace) need `standardize`")
        io = _abi.PhxSeqBatchIO(T=T, N=N, capacity=capacity, n_planes=len(planes), row_words=int(row_words), S=S, class_id=int(class_id),
                                std_plane=std_plane, shuffle=1 if shuffle else 0, seed=int(seed), epoch=int(epoch), keep=_ptr(keep),
                                col_class=_ptr(col_class), seq_start=_ptr(start), records=_ptr(records), out_row=_ptr(orow), out_col=_ptr(ocol),
                                moments=_ptr(moments), workspace=_ptr(workspace), max_seq_len=L, terminated=_ptr(terminated),
                                truncated=_ptr(truncated), seq_lens=_ptr(lens), seq_row=_ptr(srow), seq_col=_ptr(scol))
        for k, (name, x) in enumerate(planes.items()):
            io.plane[k] = _abi.PhxBatchPlane(src=_ptr(x), elem_bytes=x.element_size() * layout[name][1], word_off=layout[name][0])
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_seq_batch(C.byref(io), self._stream()), "phx_seq_batch")
        return start, records, lens, srow, scol, orow, ocol, moments, layout

    def _replay_ring(self, fn, ring, state):
        """the arguments ``replay_add`` and ``replay_sample`` share, checked: ``(C, row_words)``"""
        torch = _torch()
        if ring is None or not hasattr(ring, "dim") or ring.dim() != 2 or ring.shape[0] < 1:
            raise ValueError(f"{fn}: `ring` must be an i32 [C, row_words] tensor with C >= 1")
        Cn, row_words = int(ring.shape[0]), int(ring.shape[1])
        if not 4 <= row_words <= 256 or row_words % 4:
            raise ValueError(f"{fn}: `ring` has records of {row_words} words: row_words must be a multiple of 4 in [4, 256]")
        check_tensor(fn, "ring", ring, torch.int32, (Cn, row_words), align=16, device=self.device)
        check_tensor(fn, "state", state, torch.int64, (4,), align=16, device=self.device)
        return Cn, row_words

    def replay_add(self, ring, state, records, count=None):
        """Append records to a ring on the current stream (phx_replay_add, include/phantom_amd_replay.h).  ``ring`` is i32
        ``[C, row_words]`` and ``state`` i64 ``[4]`` (cursor, size, total, refused; zero-filled once: the empty ring), both 16-byte
        aligned on the env's device; ``records`` i32 ``[src_capacity, row_words]``, a ``DeviceBatch``'s.  ``count``: None for all of
        ``records``, an int K in ``[0, src_capacity]``, or a device i64 tensor of one element that holds K (``batch.start[-1:]``) --
        read on the device, the call does not synchronise: a K outside ``[0, src_capacity]`` adds nothing and counts in
        ``state[3]``.  The last ``min(K, C)`` of the first K records go to the slots from the cursor on, wrapping."""
        torch = _torch()
        Cn, row_words = self._replay_ring("replay_add", ring, state)
        if records is None or not hasattr(records, "dim") or records.dim() != 2:
            raise ValueError(f"replay_add: `records` must be an i32 [src_capacity, {row_words}] tensor")
        src_capacity = int(records.shape[0])
        check_tensor("replay_add", "records", records, torch.int32, (src_capacity, row_words), align=16, device=self.device)
        count_ptr, host_count = None, 0
        if count is None:
            host_count = src_capacity
        elif hasattr(count, "dim"):
            if count.numel() != 1:
                raise ValueError(f"replay_add: a device `count` must hold one element, got shape {tuple(count.shape)}")
            check_tensor("replay_add", "count", count, torch.int64, tuple(count.shape), align=8, device=self.device)
            count_ptr = count
        else:
            if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 0 <= count <= src_capacity:
                raise ValueError(f"replay_add: count = {count!r} must be None, a device i64 tensor or an int in [0, {src_capacity}]")
            host_count = int(count)
        io = _abi.PhxReplayAddIO(capacity=Cn, src_capacity=src_capacity, count=host_count, row_words=row_words, count_ptr=_ptr(count_ptr),
                                 src=_ptr(records) if src_capacity else None, ring=_ptr(ring), state=_ptr(state))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_replay_add(C.byref(io), self._stream()), "phx_replay_add")

    def replay_sample(self, ring, state, n, seed: int = 0, draw: int = 0, slots=None, out=None):
        """``(out, out_slot)``: n records of a ring on the current stream (phx_replay_sample, include/phantom_amd_replay.h) --
        ``out`` i32 ``[n, row_words]`` and ``out_slot`` i64 ``[n]``, the slot every record came from.  ``ring`` / ``state`` are
        ``replay_add``'s.  Without ``slots`` the slots are uniform draws with replacement from the valid ones, stream ``(seed,
        draw)``; with ``slots`` (a device i64 ``[n]`` tensor) they are the caller's, as a prioritized sampler needs.  A slot outside
        ``[0, size)`` -- every one while the ring is empty -- gives a record of zeros and -1.  ``out``: ``(out, out_slot or None)``,
        caller-owned and 16-byte aligned; allocated here when None.  The call does not synchronise."""
        torch = _torch()
        Cn, row_words = self._replay_ring("replay_sample", ring, state)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"replay_sample: n = {n!r} must be an int >= 1")
        n = int(n)
        for name, v in (("seed", seed), ("draw", draw)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 64:
                raise ValueError(f"replay_sample: {name} = {v!r} must be an int in [0, 2^64)")
        if slots is not None:
            check_tensor("replay_sample", "slots", slots, torch.int64, (n,), align=8, device=self.device)
        if out is None:
            out = (torch.empty((n, row_words), dtype=torch.int32, device=self.device), torch.empty((n,), dtype=torch.int64, device=self.device))
        if len(out) != 2:
            raise ValueError("replay_sample: `out` is (out, out_slot or None)")
        rec, oslot = out
        check_tensor("replay_sample", "out[0]", rec, torch.int32, (n, row_words), align=16, device=self.device)
        if oslot is not None:
            check_tensor("replay_sample", "out[1]", oslot, torch.int64, (n,), align=16, device=self.device)
        io = _abi.PhxReplaySampleIO(capacity=Cn, n=n, row_words=row_words, seed=int(seed), draw=int(draw), slot_in=_ptr(slots), ring=_ptr(ring),
                                    state=_ptr(state), out=_ptr(rec), out_slot=_ptr(oslot))
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_replay_sample(C.byref(io), self._stream()), "phx_replay_sample")
        return rec, oslot

    def step_graph(self, actions=None, n: Optional[int] = None, policy=None, action_valid=None):
        """Capture ``n`` consecutive ``phx_step`` launches ONCE into a hipGraph and return a replayable
        ``StepGraph``: per-step launch cadence drops from the host's ~6-9 us to the graph's.

        * ``actions`` f32 [n, B, S]: step i reads ``actions[i]`` -- refill the tensor in place between
          replays (``graph.actions``);
        * or ``policy(step_tensors) -> f32 [B, S]``: a capturable torch callable (no host sync) that maps
          the previous step's device outputs to the next actions -- the whole act/step loop is one graph.
        Outputs of the LAST captured step are in ``graph.out`` (the env's persistent StepTensors)."""
        torch = _torch()
        if actions is None and policy is None:
            raise ValueError("step_graph needs an actions tensor [n, B, S] or a policy callable")
        if actions is not None:
            n = actions.shape[0] if n is None else n
            check_tensor("step_graph", "actions", actions, torch.float32, (n, self.B, self.S), device=self.device)
        elif n is None:
            raise ValueError("step_graph(policy=...) needs n")
        self._ensure_step_io()
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(self.device)
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g, stream=side):          # stream capture records the launches, it does not run them
            out = self._step_out                        # the first policy call sees the env's current outputs
            for i in range(n):                          # (after reset(): the reset observations)
                a = actions[i] if actions is not None else policy(out).contiguous()
                out = self.step(a, action_valid)
        torch.cuda.synchronize(self.device)
        return StepGraph(g, actions, self._step_out, n, self)

    def rollout_graph(self, T: int, trajectories):
        """Capture one ``phx_rollout`` of T steps per buffer of ``trajectories`` (from ``alloc_trajectory(T)``), in order, into a
        hipGraph: a collection loop that consumes fragment after fragment replays the graph instead of paying a host launch per
        fragment (the gap between dependent launches drops from the host's cadence to the graph's).  The env advances
        ``len(trajectories) * T`` steps per replay, exactly as the same sequence of ``rollout`` calls would."""
        torch = _torch()
        trajectories = list(trajectories)
        if not trajectories:
            raise ValueError("rollout_graph needs at least one trajectory buffer")
        for tr in trajectories:
            self._check_rollout_planes(T, tr)
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(self.device)
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g, stream=side):          # stream capture records the launches, it does not run them
            for tr in trajectories:
                self.rollout(T, out=tr)
        torch.cuda.synchronize(self.device)
        return RolloutGraph(g, trajectories, T)

    def inject(self, messages: List[Message]):
        if not messages:
            return
        arr = (_abi.PhxMsgRec * len(messages))()
        for k, m in enumerate(messages):
            t, is_f, v = payload_to_record(m.payload)
            arr[k].sender = self.spec.index_of(m.sender_id)
            arr[k].receiver = self.spec.index_of(m.receiver_id)
            arr[k].type = t
            if is_f:
                arr[k].payload.f = float(v)
            else:
                arr[k].payload.i = int(v)
        self._check(self.lib.phx_inject(self.handle, arr, len(messages)), "phx_inject")

    def resolve(self, pending: List[Message], network=None):
        torch = _torch()
        self.inject(pending)
        lp = self.msg_log.data_ptr() if self.msg_log is not None else None
        cp = self.msg_count.data_ptr() if self.msg_count is not None else None
        self.err.zero_()
        with torch.cuda.device(self.device):
            self._check(self.lib.phx_resolve(self.handle, self.err.data_ptr(), lp, cp,
                                             self._stream()), "phx_resolve")
        self.raise_errors(network)
        if network is not None and network.resolver.enable_tracking:
            network.resolver._tracked_messages.extend(self.read_log(0))

    # ---- read-back ----------------------------------------------------------------------------
    def read_log_records(self, b: int = 0) -> np.ndarray:
        """structured array (sender, receiver, type, round, raw i64) of env b's last step."""
        if self.msg_log is None:
            raise DeviceError("tracking is disabled (BatchResolver(enable_tracking=True))")
        n = int(self.msg_count[b].item())
        if n > self.spec.trace_cap:
            raise DeviceError(f"message log overflow: {n} > trace capacity {self.spec.trace_cap}")
        raw = self.msg_log[b, :n].cpu().numpy().tobytes()
        dt = np.dtype([("sender", "<u2"), ("receiver", "<u2"), ("type", "<u2"), ("round", "<u2"),
                       ("raw", "<i8")])
        return np.frombuffer(raw, dtype=dt)

    def read_log(self, b: int = 0) -> List[Message]:
        recs = self.read_log_records(b)
        ids = self.spec.agent_ids
        out = []
        for r in recs:
            raw_i = int(r["raw"])
            raw_f = np.array([raw_i], dtype="<i8").view("<f8")[0].item()
            out.append(Message(ids[int(r["sender"])], ids[int(r["receiver"])],
                               record_to_payload(int(r["type"]), raw_i, raw_f)))
        return out

    def raise_errors(self, network=None, err=None):
        """Re-raise per-env soft error codes as the exceptions the reference raises in step()."""
        if err is None:
            err = self.err.cpu().numpy()
        bad = np.flatnonzero(err)
        if bad.size == 0:
            return
        from .network import NetworkError
        b, code = int(bad[0]), int(err[bad[0]])
        where = f"env instance {b} (+{bad.size - 1} more)" if bad.size > 1 else f"env instance {b}"
        if code == _abi.ERR_NETWORK:
            raise NetworkError(f"No connection between sender and receiver ({where}).")
        if code == _abi.ERR_PAYLOAD:
            raise NetworkError(f"Message payload not allowed between these agent types ({where}).")
        if code == _abi.ERR_UNKNOWN_MSG:
            raise ValueError(f"Unknown message type: receiving agent has no handler ({where}).")
        if code == _abi.ERR_ROUND_LIMIT:
            raise RuntimeError("message(s) still in queue after BatchResolver round limit "
                               f"reached ({where}).")
        if code == _abi.ERR_FSM_TRANSITION:                # fsm.py:304-307
            from .fsm import FSMRuntimeError
            raise FSMRuntimeError(f"FiniteStateMachineEnv attempted invalid transition ({where}).")
        if code == _abi.ERR_CONTEXT:                       # ctx[agent_id] of a non-neighbour, context.py:36-37
            raise KeyError(f"agent view / table entry not present in the handler's context ({where}).")
        raise DeviceError(f"per-round message capacity exceeded ({where}); raise queue capacity")
