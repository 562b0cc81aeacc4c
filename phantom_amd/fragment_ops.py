"""FragmentOps: the learner-side entry points over time-major fragments (phx_gae .. phx_replay_sample, phx_prio_*, phx_filter_*), and their
argument checks.

None of them needs an env handle: a loaded library and a device are enough, and ``DeviceEnv`` inherits them.  The library
receives raw device pointers, so every rule a tensor or a scalar has to meet is stated once here, as a helper or as a table the
ops fill in.  Pure host code up to ``_launch``: importing this module touches neither torch.cuda nor the built library.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from ._buffers import check_tensor


def _torch():
    import torch
    return torch


_ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else None

# an output row's ``wanted`` (FragmentOps._outputs).  REQUIRED: allocated here, a caller's may not be None.  OPTIONAL: allocated here,
# a caller may pass None (not written).  UNWANTED: not allocated here, a caller may still pass one.  Any other string: the output
# must be None because its input is missing, and the string is what the refusal says.
REQUIRED, OPTIONAL, UNWANTED = _WANTED = ("required", "optional", "unwanted")


class DeviceError(RuntimeError):
    pass


def _lead(fn, name, x):
    """``(shape, T, N)`` of the plane that gives an op its leading shape ``[T, B, S]`` (or ``[T, N]``)"""
    if x is None or not hasattr(x, "dim") or x.dim() < 2:
        raise ValueError(f"{fn}: `{name}` must be a [T, B, S] (or [T, N]) tensor")
    return _rows_cols(fn, f"`{name}` has shape", tuple(x.shape))


def _rows_cols(fn, what, shape):
    T, N = shape[0], math.prod(shape[1:])
    if T < 1 or N < 1:
        raise ValueError(f"{fn}: {what} {shape}: T and N must be >= 1")
    return shape, T, N


def _is_int(v, lo, hi=None) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and v >= lo and (hi is None or v <= hi)


def _int(fn, name, v, lo, hi=None, must=None) -> int:
    """``v`` as an int in [lo, hi] (no upper end: None); a bool is none.  ``must``: the message's wording where it is not the default"""
    if not _is_int(v, lo, hi):
        raise ValueError(f"{fn}: {name} = {v!r} must be " + (must or (f"an int >= {lo}" if hi is None else f"an int in [{lo}, {hi}]")))
    return int(v)


def _unit_interval(fn, as_f32=False, **values):
    """every value lies in [0, 1] (NaN fails both comparisons); ``as_f32``: tested as the f32 the struct holds"""
    if not all(0.0 <= (float(np.float32(v)) if as_f32 else v) <= 1.0 for v in values.values()):
        raise ValueError(f"{fn}: " + " and ".join(f"{k} = {v}" for k, v in values.items()) + " must lie in [0, 1]")


def _capacity(fn, capacity, default) -> int:
    capacity = default if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError(f"{fn}: capacity = {capacity} must be >= 0")
    return capacity


def _count(fn, count, src_capacity, device):
    """``(count_ptr, host_count)`` of an add's ``count``: None for all ``src_capacity`` records, an int in ``[0, src_capacity]`` or a
    device i64 tensor of one element"""
    if count is None:
        return None, src_capacity
    if hasattr(count, "dim"):
        if count.numel() != 1:
            raise ValueError(f"{fn}: a device `count` must hold one element, got shape {tuple(count.shape)}")
        check_tensor(fn, "count", count, _torch().int64, tuple(count.shape), align=8, device=device)
        return count, 0
    return None, _int(fn, "count", count, 0, src_capacity, f"None, a device i64 tensor or an int in [0, {src_capacity}]")


def _draws(fn, n, seed, draw):
    """``(n, seed, draw)`` of a sampling call: n >= 1 draws of the stream ``(seed, draw)``"""
    return (_int(fn, "n", n, 1), _int(fn, "seed", seed, 0, 2 ** 64 - 1, "an int in [0, 2^64)"),
            _int(fn, "draw", draw, 0, 2 ** 64 - 1, "an int in [0, 2^64)"))


def _set_batch_planes(io, planes, layout):
    for k, (name, x) in enumerate(planes.items()):
        io.plane[k] = _abi.PhxBatchPlane(src=_ptr(x), elem_bytes=x.element_size() * layout[name][1], word_off=layout[name][0])


class FragmentOps:
    def __init__(self, lib, device):
        self.lib, self.device = lib, device

    # ---- helpers --------------------------------------------------------------------------
    def _err(self) -> str:
        return (self.lib.phx_last_error() or b"").decode()

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise DeviceError(f"{what} failed ({rc}): {self._err()}")

    def _launch(self, entry, io):
        """one call of a fragment entry point (``_abi.FRAGMENT_OPS``, ``_abi.PRIORITY_OPS``, ``_abi.FILTER_OPS``) on torch's current stream of the device"""
        torch = _torch()
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, entry)(C.byref(io), self._stream()), entry)

    def _planes(self, fn, shape, rows):
        """input planes ``(name, tensor, dtype, required)`` of one ``shape``; one that is not required may be None"""
        for name, x, dtype, required in rows:
            if required or x is not None:
                check_tensor(fn, name, x, dtype, shape, device=self.device)

    def _outputs(self, fn, out, rows, usage=None):
        """An op's ``out``, one row ``(dtype, shape, wanted)`` per element: allocated here when None, else of ``len(rows)`` elements
        (``usage``: what the op's message says `out` is; None: the op has none and its own unpacking raises), each one a 16-byte
        aligned tensor named ``out[i]``.  ``wanted`` is REQUIRED, OPTIONAL, UNWANTED or a message (see above)."""
        if out is None:
            torch = _torch()
            out = tuple(torch.empty(shape, dtype=dtype, device=self.device) if wanted in (REQUIRED, OPTIONAL) else None
                        for dtype, shape, wanted in rows)
        if usage is not None and len(out) != len(rows):
            raise ValueError(f"{fn}: `out` is {usage}")
        for i, (x, (dtype, shape, wanted)) in enumerate(zip(out, rows)):
            if wanted not in _WANTED:
                if x is not None:
                    raise ValueError(f"{fn}: {wanted}")
            elif x is not None or wanted is REQUIRED:
                check_tensor(fn, f"out[{i}]", x, dtype, shape, align=16, device=self.device)
        return out

    def _record_planes(self, fn, shape, planes):
        """planes that become words of a record: ``[T, N..]`` (u8, f32, i32) or ``[T, N.., w]`` (f32, i32; 1 <= w <= 64), checked;
        ``{name: trailing shape}``, () or (w,)"""
        torch = _torch()
        tails = {}
        for name, x in planes.items():
            if x is None or not hasattr(x, "dim") or x.dim() not in (len(shape), len(shape) + 1):
                raise ValueError(f"{fn}: plane `{name}` must be a {shape} or {shape + ('w',)} tensor")
            tail = tuple(x.shape[len(shape):])
            if tail and (x.dtype == torch.uint8 or not 1 <= tail[0] <= 64):
                raise ValueError(f"{fn}: plane `{name}`: a trailing axis needs f32 or i32 and 1 <= w <= 64")
            check_tensor(fn, f"plane `{name}`", x, (torch.uint8, torch.float32, torch.int32), shape + tail, device=self.device)
            tails[name] = tail
        return tails

    def _gather_dim(self, fn, shape, **tensors):
        """D of the f32 ``shape + (D,)`` tensors a gather launch reads, 1 <= D <= 64: the first one gives it, all are checked"""
        name, x = next(iter(tensors.items()))
        if not hasattr(x, "dim") or x.dim() != len(shape) + 1 or not 1 <= x.shape[-1] <= 64:
            raise ValueError(f"{fn}: `{name}` must be a {shape + ('D',)} tensor with 1 <= D <= 64")
        D = int(x.shape[-1])
        for name, x in tensors.items():
            check_tensor(fn, name, x, _torch().float32, shape + (D,), device=self.device)
        return D

    # ---- entry points ---------------------------------------------------------------------
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
        shape, T, N = _lead("gae", "rewards", rewards)
        _unit_interval("gae", gamma=gamma, lambda_=lambda_)
        self._planes("gae", shape, (("rewards", rewards, f32, True), ("truncations", truncations, u8, True), ("vf_pred", vf_pred, f32, False),
                                    ("vf_next", vf_next, f32, False), ("terminations", terminations, u8, False)))
        adv, vt = self._outputs("gae", out, [(f32, shape, REQUIRED)] * 2)
        self._launch("phx_gae", _abi.PhxGaeIO(
            T=T, N=N, gamma=gamma, lambda_=lambda_, reward=_ptr(rewards), vf_pred=_ptr(vf_pred), vf_next=_ptr(vf_next),
            terminated=_ptr(terminations), truncated=_ptr(truncations), advantage=_ptr(adv), value_target=_ptr(vt)))
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
        shape, T, N = _lead("gae_masked", "rewards", rewards)
        _unit_interval("gae_masked", gamma=gamma, lambda_=lambda_)
        self._planes("gae_masked", shape, (("rewards", rewards, f32, True), ("truncations", truncations, u8, True),
                                           ("vf_pred", vf_pred, f32, False), ("vf_next", vf_next, f32, False),
                                           ("terminations", terminations, u8, False), ("acted", acted, u8, False),
                                           ("reward_valid", reward_valid, u8, False)))
        adv, vt, rs = self._outputs("gae_masked", out, [(f32, shape, REQUIRED)] * 3)
        self._launch("phx_gae_masked", _abi.PhxGaeMaskedIO(
            T=T, N=N, gamma=gamma, lambda_=lambda_, reward=_ptr(rewards), vf_pred=_ptr(vf_pred), vf_next=_ptr(vf_next),
            terminated=_ptr(terminations), truncated=_ptr(truncations), acted=_ptr(acted), reward_valid=_ptr(reward_valid),
            advantage=_ptr(adv), value_target=_ptr(vt), reward_sum=_ptr(rs)))
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
        shape, T, N = _lead("vtrace", "rewards", rewards)
        _unit_interval("vtrace", gamma=gamma, lambda_=lambda_)
        clips = [float(np.float32(x)) for x in (clip_rho_threshold, clip_c_threshold, clip_pg_rho_threshold)]      # (as the struct holds them)
        if not all(np.isfinite(x) and x > 0.0 for x in clips):
            raise ValueError(f"vtrace: clip_rho_threshold = {clip_rho_threshold}, clip_c_threshold = {clip_c_threshold} and "
                             f"clip_pg_rho_threshold = {clip_pg_rho_threshold} must be finite and > 0")
        self._planes("vtrace", shape, (("rewards", rewards, f32, True), ("truncations", truncations, u8, True), ("vf_pred", vf_pred, f32, True),
                                       ("behaviour_logp", behaviour_logp, f32, True), ("target_logp", target_logp, f32, True),
                                       ("vf_next", vf_next, f32, False), ("terminations", terminations, u8, False)))
        vs, pg = self._outputs("vtrace", out, [(f32, shape, REQUIRED)] * 2)
        self._launch("phx_vtrace", _abi.PhxVtraceIO(
            T=T, N=N, gamma=gamma, lambda_=lambda_, rho_bar=clips[0], c_bar=clips[1], pg_rho_bar=clips[2], reward=_ptr(rewards),
            vf_pred=_ptr(vf_pred), vf_next=_ptr(vf_next), behaviour_logp=_ptr(behaviour_logp), target_logp=_ptr(target_logp),
            terminated=_ptr(terminations), truncated=_ptr(truncations), vs=_ptr(vs), pg_advantage=_ptr(pg)))
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
        shape, T, N = _lead("traj_next", "truncations", truncations)
        self._planes("traj_next", shape, (("truncations", truncations, u8, True), ("terminations", terminations, u8, False),
                                          ("acted", acted, u8, False), ("new_obs_valid", new_obs_valid, u8, False)))
        if (obs is None) != (new_obs is None):
            raise ValueError("traj_next: `obs` and `new_obs` come together (both for `next_obs`, neither without it)")
        gather = obs is not None
        D = self._gather_dim("traj_next", shape, obs=obs, new_obs=new_obs) if gather else 0
        nr, nte, ntr, nob = self._outputs(
            "traj_next", out, ((i32, shape, REQUIRED), (u8, shape, REQUIRED), (u8, shape, REQUIRED),
                               (f32, shape + (D,), REQUIRED if gather else "`out[3]` (next_obs) needs `obs` and `new_obs`")),
            "(next_row, next_terminated, next_truncated, next_obs or None)")
        self._launch("phx_traj_next", _abi.PhxTrajNextIO(
            T=T, D=D, N=N, truncated=_ptr(truncations), terminated=_ptr(terminations), acted=_ptr(acted), new_obs_valid=_ptr(new_obs_valid),
            obs=_ptr(obs), new_obs=_ptr(new_obs), next_row=_ptr(nr), next_terminated=_ptr(nte), next_truncated=_ptr(ntr), next_obs=_ptr(nob)))
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
        shape, T, N = _lead("nstep", "rewards", rewards)
        n = _int("nstep", "n", n, 1, _abi.NSTEP_MAX_N)
        _unit_interval("nstep", as_f32=True, gamma=gamma)
        self._planes("nstep", shape, (("rewards", rewards, f32, True), ("truncations", truncations, u8, True),
                                      ("terminations", terminations, u8, False), ("acted", acted, u8, False), ("next_row", next_row, i32, False)))
        gather = next_obs is not None
        D = self._gather_dim("nstep", shape, next_obs=next_obs) if gather else 0
        if out is not None and len(out) == 7:                    # (no eighth: like a None there)
            out = tuple(out) + (None,)
        out = self._outputs(
            "nstep", out, ((f32, shape, REQUIRED), (f32, shape, REQUIRED), (i32, shape, REQUIRED), (u8, shape, REQUIRED), (u8, shape, REQUIRED),
                           (i32, shape, REQUIRED), (f32, shape + (D,), REQUIRED if gather else "`out[6]` (nstep_next_obs) needs `next_obs`"),
                           (i32, shape, UNWANTED)),
            "(nstep_rewards, nstep_discounts, nstep_last, nstep_terminateds, nstep_truncateds, nstep_next_row, nstep_next_obs or None[, succ_row])")
        res, succ = tuple(out[:7]), out[7]
        if succ is None and acted is not None:
            succ = torch.empty(shape, dtype=i32, device=self.device)
        self._launch("phx_nstep", _abi.PhxNstepIO(
            T=T, D=D, N=N, n=n, gamma=gamma, reward=_ptr(rewards), truncated=_ptr(truncations), terminated=_ptr(terminations),
            acted=_ptr(acted), next_row=_ptr(next_row), next_obs=_ptr(next_obs), succ_row=_ptr(succ), nstep_reward=_ptr(res[0]),
            nstep_discount=_ptr(res[1]), nstep_last=_ptr(res[2]), nstep_terminated=_ptr(res[3]), nstep_truncated=_ptr(res[4]),
            nstep_next_row=_ptr(res[5]), nstep_next_obs=_ptr(res[6])))
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
        shape, T, N = _lead("episode_stats", "rewards", rewards)
        _int("episode_stats", "group", group, 1, _abi.EPISODE_MAX_G, f"an int >= 1 and <= {_abi.EPISODE_MAX_G}")
        _int("episode_stats", "classes", classes, 1)
        if N % group:
            raise ValueError(f"episode_stats: group = {group} must divide the {N} input columns")
        Cn = N // int(group)
        if Cn % classes or classes >= 2 ** 31:
            raise ValueError(f"episode_stats: classes = {classes} must divide the {Cn} output columns")
        self._planes("episode_stats", shape, (("rewards", rewards, f32, True), ("truncations", truncations, u8, True),
                                              ("terminations", terminations, u8, False), ("acted", acted, u8, False),
                                              ("reward_valid", reward_valid, u8, False)))
        cr = cl = None
        if carry is not None:
            if len(carry) != 2:
                raise ValueError("episode_stats: `carry` is a (f32 [C], i32 [C]) pair of device tensors")
            cr, cl = carry
            check_tensor("episode_stats", "carry[0]", cr, f32, (Cn,), device=self.device)
            check_tensor("episode_stats", "carry[1]", cl, i32, (Cn,), device=self.device)
        nb = _abi.EPISODE_STATS_BYTES
        col, summ, eret, elen = self._outputs(
            "episode_stats", out, ((u8, (Cn, nb), REQUIRED), (u8, (int(classes), nb), OPTIONAL if summary else UNWANTED),
                                   (f32, (T, Cn), OPTIONAL if planes else UNWANTED), (i32, (T, Cn), OPTIONAL if planes else UNWANTED)),
            "(col_stats, summary or None, episode_return or None, episode_len or None)")
        self._launch("phx_episode_stats", _abi.PhxEpisodeIO(
            T=T, G=int(group), N=N, K=int(classes), reward=_ptr(rewards), truncated=_ptr(truncations), terminated=_ptr(terminations),
            acted=_ptr(acted), reward_valid=_ptr(reward_valid), carry_return=_ptr(cr), carry_len=_ptr(cl), episode_return=_ptr(eret),
            episode_len=_ptr(elen), col_stats=_ptr(col), summary=_ptr(summ)))
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
        u8, i32, i64 = torch.uint8, torch.int32, torch.int64
        shape, T, N = _lead("compact", "keep", keep)
        check_tensor("compact", "keep", keep, u8, shape, device=self.device)
        capacity = _capacity("compact", capacity, T * N)
        planes = dict(planes)
        tails = self._record_planes("compact", shape, planes)
        usage = "(start, out_row or None, out_col or None, {name: dense tensor}) with the planes' names"
        if out is not None and (len(out) != 4 or set(out[3]) != set(planes)):
            raise ValueError(f"compact: `out` is {usage}")
        start, orow, ocol = self._outputs("compact", None if out is None else out[:3],
                                          ((i64, (N + 1,), REQUIRED), (i32, (capacity,), OPTIONAL), (i32, (capacity,), OPTIONAL)), usage)
        dense = out[3] if out is not None else {k: torch.empty((capacity,) + tails[k], dtype=x.dtype, device=self.device)
                                                for k, x in planes.items()}
        for name, x in planes.items():
            check_tensor("compact", f"out[3][`{name}`]", dense[name], x.dtype, (capacity,) + tails[name], align=16, device=self.device)
        names = list(planes)
        for first in range(0, max(len(names), 1), _abi.COMPACT_MAX_PLANES):
            part = names[first:first + _abi.COMPACT_MAX_PLANES]
            io = _abi.PhxTrajCompactIO(T=T, n_planes=len(part), N=N, capacity=capacity, keep=_ptr(keep), start=_ptr(start),
                                       out_row=_ptr(orow) if first == 0 else None, out_col=_ptr(ocol) if first == 0 else None)
            for k, name in enumerate(part):
                io.plane[k] = _abi.PhxCompactPlane(src=_ptr(planes[name]), dst=_ptr(dense[name]),
                                                   elem_bytes=planes[name].element_size() * math.prod(tails[name]), reserved=0)
            self._launch("phx_traj_compact", io)
        return start, orow, ocol, dense

    def _batch_planes(self, fn, planes, keep, col_class, class_id, standardize, seed, epoch, row_words, lead_dims):
        """the arguments ``train_batch`` and ``seq_batch`` share, checked: ``(planes, shape, T, N, S, layout, row_words, std_plane)``"""
        torch = _torch()
        f32, u8 = torch.float32, torch.uint8
        planes = dict(planes)
        if len(planes) > _abi.BATCH_MAX_PLANES:
            raise ValueError(f"{fn}: {len(planes)} planes, at most {_abi.BATCH_MAX_PLANES} fit one call")
        lead = keep if keep is not None else min((x for x in planes.values() if hasattr(x, "dim")), key=lambda x: x.dim(), default=None)
        if lead is None or not hasattr(lead, "dim") or lead.dim() < 2:
            raise ValueError(f"{fn}: `keep` or a plane must give the leading shape [T, B, S] (or [T, N])")
        if keep is None and lead_dims is not None:
            shape = tuple(lead.shape[:_int(fn, "lead_dims", lead_dims, 2, lead.dim())])
        else:
            shape = tuple(lead.shape)
        shape, T, N = _rows_cols(fn, "the leading shape is", shape)
        if keep is not None:
            check_tensor(fn, "keep", keep, u8, shape, device=self.device)
        S = 1
        if col_class is not None:
            if not hasattr(col_class, "dim") or col_class.dim() != 1 or col_class.numel() < 1 or N % col_class.numel():
                raise ValueError(f"{fn}: `col_class` must be a u8 [S] tensor with S >= 1 dividing the {N} columns")
            S = col_class.numel()
            check_tensor(fn, "col_class", col_class, u8, (S,), device=self.device)
        _int(fn, "class_id", class_id, 0, 255)
        _int(fn, "seed", seed, 0, 2 ** 64 - 1, "an int in [0, 2^64)")
        _int(fn, "epoch", epoch, 0, 2 ** 64 - 1, "an int in [0, 2^64)")
        layout, off = {}, 0
        for name, tail in self._record_planes(fn, shape, planes).items():
            w = tail[0] if tail else 1
            layout[name] = (off, w, planes[name].dtype)
            off += w
        if row_words is None:
            row_words = max(16, -(-off // 16) * 16)
        if not _is_int(row_words, 4, 256) or row_words % 4 or off > row_words:
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
        u8, i32, i64 = torch.uint8, torch.int32, torch.int64
        planes, shape, T, N, S, layout, row_words, std_plane = self._batch_planes("train_batch", planes, keep, col_class, class_id, standardize,
                                                                                  seed, epoch, row_words, lead_dims)
        capacity = _capacity("train_batch", capacity, T * N)
        std = REQUIRED if std_plane >= 0 else "`out[4]` (moments) and `out[5]` (workspace) need `standardize`"
        start, records, orow, ocol, moments, workspace = self._outputs(
            "train_batch", out, ((i64, (N + 1,), REQUIRED), (i32, (capacity, row_words), REQUIRED), (i32, (capacity,), OPTIONAL),
                                 (i32, (capacity,), OPTIONAL), (u8, (_abi.BATCH_MOMENTS_BYTES,), std), (torch.float64, (N, 2), std)),
            "(start, records, out_row or None, out_col or None, moments or None, workspace or None)")
        io = _abi.PhxTrainBatchIO(T=T, N=N, capacity=capacity, n_planes=len(planes), row_words=row_words, S=S, class_id=int(class_id),
                                  std_plane=std_plane, shuffle=1 if shuffle else 0, seed=int(seed), epoch=int(epoch), keep=_ptr(keep),
                                  col_class=_ptr(col_class), start=_ptr(start), records=_ptr(records), out_row=_ptr(orow), out_col=_ptr(ocol),
                                  moments=_ptr(moments), workspace=_ptr(workspace))
        _set_batch_planes(io, planes, layout)
        self._launch("phx_train_batch", io)
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
        u8, i32, i64 = torch.uint8, torch.int32, torch.int64
        L = _int("seq_batch", "max_seq_len", max_seq_len, 1, _abi.SEQ_MAX_LEN)
        planes, shape, T, N, S, layout, row_words, std_plane = self._batch_planes("seq_batch", planes, keep, col_class, class_id, standardize,
                                                                                  seed, epoch, row_words, lead_dims)
        self._planes("seq_batch", shape, (("terminated", terminated, u8, False), ("truncated", truncated, u8, False)))
        if capacity is None:                                     # (the length cuts, and a flag per row where flags are given)
            capacity = N * -(-T // L) if terminated is None and truncated is None else T * N
        capacity = _int("seq_batch", "capacity", capacity, 0)
        std = REQUIRED if std_plane >= 0 else "`out[7]` (moments) and `out[8]` (workspace) need `standardize`"
        start, records, lens, srow, scol, orow, ocol, moments, workspace = self._outputs(
            "seq_batch", out, ((i64, (N + 1,), REQUIRED), (i32, (capacity, L, row_words), REQUIRED), (i32, (capacity,), OPTIONAL),
                               (i32, (capacity,), OPTIONAL), (i32, (capacity,), OPTIONAL), (i32, (capacity, L), OPTIONAL),
                               (i32, (capacity, L), OPTIONAL), (u8, (_abi.BATCH_MOMENTS_BYTES,), std), (torch.float64, (3, N), std)),
            "(seq_start, records, seq_lens or None, seq_row or None, seq_col or None, out_row or None, out_col or None, moments or None, "
            "workspace or None)")
        io = _abi.PhxSeqBatchIO(T=T, N=N, capacity=capacity, n_planes=len(planes), row_words=row_words, S=S, class_id=int(class_id),
                                std_plane=std_plane, shuffle=1 if shuffle else 0, seed=int(seed), epoch=int(epoch), keep=_ptr(keep),
                                col_class=_ptr(col_class), seq_start=_ptr(start), records=_ptr(records), out_row=_ptr(orow), out_col=_ptr(ocol),
                                moments=_ptr(moments), workspace=_ptr(workspace), max_seq_len=L, terminated=_ptr(terminated),
                                truncated=_ptr(truncated), seq_lens=_ptr(lens), seq_row=_ptr(srow), seq_col=_ptr(scol))
        _set_batch_planes(io, planes, layout)
        self._launch("phx_seq_batch", io)
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
        count_ptr, host_count = _count("replay_add", count, src_capacity, self.device)
        self._launch("phx_replay_add", _abi.PhxReplayAddIO(
            capacity=Cn, src_capacity=src_capacity, count=host_count, row_words=row_words, count_ptr=_ptr(count_ptr),
            src=_ptr(records) if src_capacity else None, ring=_ptr(ring), state=_ptr(state)))

    def replay_sample(self, ring, state, n, seed: int = 0, draw: int = 0, slots=None, out=None):
        """``(out, out_slot)``: n records of a ring on the current stream (phx_replay_sample, include/phantom_amd_replay.h) --
        ``out`` i32 ``[n, row_words]`` and ``out_slot`` i64 ``[n]``, the slot every record came from.  ``ring`` / ``state`` are
        ``replay_add``'s.  Without ``slots`` the slots are uniform draws with replacement from the valid ones, stream ``(seed,
        draw)``; with ``slots`` (a device i64 ``[n]`` tensor) they are the caller's, as a prioritized sampler needs.  A slot outside
        ``[0, size)`` -- every one while the ring is empty -- gives a record of zeros and -1.  ``out``: ``(out, out_slot or None)``,
        caller-owned and 16-byte aligned; allocated here when None.  The call does not synchronise."""
        torch = _torch()
        Cn, row_words = self._replay_ring("replay_sample", ring, state)
        n, seed, draw = _draws("replay_sample", n, seed, draw)
        if slots is not None:
            check_tensor("replay_sample", "slots", slots, torch.int64, (n,), align=8, device=self.device)
        rec, oslot = self._outputs("replay_sample", out, ((torch.int32, (n, row_words), REQUIRED), (torch.int64, (n,), OPTIONAL)),
                                   "(out, out_slot or None)")
        self._launch("phx_replay_sample", _abi.PhxReplaySampleIO(
            capacity=Cn, n=n, row_words=row_words, seed=seed, draw=draw, slot_in=_ptr(slots), ring=_ptr(ring), state=_ptr(state),
            out=_ptr(rec), out_slot=_ptr(oslot)))
        return rec, oslot

    def _prio_tree(self, fn, tree, pstate, ring_state, capacity):
        """the arguments the three ``prio_*`` calls share, checked: C"""
        torch = _torch()
        Cn = _int(fn, "capacity", capacity, 1, _abi.PRIO_MAX_CAPACITY, "an int in [1, 2^30]")
        words = _abi.prio_layout(Cn)[3]
        if tree is None or not hasattr(tree, "numel") or tree.numel() != words:
            raise ValueError(f"{fn}: `tree` must be an f32 [{words}] tensor, _abi.prio_layout({Cn})'s words")
        check_tensor(fn, "tree", tree, torch.float32, (words,), align=16, device=self.device)
        check_tensor(fn, "pstate", pstate, torch.uint8, (_abi.PRIO_STATE_BYTES,), align=16, device=self.device)
        check_tensor(fn, "ring_state", ring_state, torch.int64, (4,), align=8, device=self.device)
        return Cn

    def prio_add(self, tree, pstate, ring_state, capacity, src_capacity, count=None):
        """Give the records the NEXT ``replay_add`` of the same batch will write the largest priority seen so far, on the current
        stream (phx_prio_add, include/phantom_amd_prio.h).  ``tree`` is f32 ``[_abi.prio_layout(capacity).words]`` and ``pstate`` uint8
        ``[32]`` (a record of ``_abi.PRIO_STATE_DTYPE``), both zero-filled once and 16-byte aligned on the env's device; ``ring_state``
        is the ring's i64 ``[4]`` state, read only -- the call comes BEFORE the ring's add.  ``src_capacity`` and ``count`` are the
        ring add's: the records the batch's buffer holds, and None for all of them, an int K in ``[0, src_capacity]`` or a device i64
        tensor of one element that holds K.  A K outside ``[0, src_capacity]`` changes nothing and counts in the state's ``refused``."""
        Cn = self._prio_tree("prio_add", tree, pstate, ring_state, capacity)
        src_capacity = _int("prio_add", "src_capacity", src_capacity, 0)
        count_ptr, host_count = _count("prio_add", count, src_capacity, self.device)
        self._launch("phx_prio_add", _abi.PhxPrioAddIO(
            capacity=Cn, src_capacity=src_capacity, count=host_count, count_ptr=_ptr(count_ptr), ring_state=_ptr(ring_state), tree=_ptr(tree),
            state=_ptr(pstate)))

    def prio_update(self, tree, pstate, ring_state, capacity, slots, priorities):
        """Set the priorities of sampled slots on the current stream (phx_prio_update, include/phantom_amd_prio.h): ``slots`` i64
        ``[n]`` (a sample's ``.slots``) and ``priorities`` f32 ``[n]``, already raised to alpha, on the env's device; ``tree`` /
        ``pstate`` / ``ring_state`` are ``prio_add``'s.  A slot outside the records held is ignored and counted in the state's
        ``ignored``; a slot named more than once gets the largest of its priorities; NaN, zero and negatives become 2^-40."""
        torch = _torch()
        Cn = self._prio_tree("prio_update", tree, pstate, ring_state, capacity)
        if slots is None or not hasattr(slots, "dim") or slots.dim() != 1 or slots.numel() < 1:
            raise ValueError("prio_update: `slots` must be a device i64 [n] tensor with n >= 1")
        n = int(slots.numel())
        check_tensor("prio_update", "slots", slots, torch.int64, (n,), align=8, device=self.device)
        check_tensor("prio_update", "priorities", priorities, torch.float32, (n,), device=self.device)
        self._launch("phx_prio_update", _abi.PhxPrioUpdateIO(
            capacity=Cn, n=n, slot_in=_ptr(slots), priority=_ptr(priorities), ring_state=_ptr(ring_state), tree=_ptr(tree), state=_ptr(pstate)))

    def prio_sample(self, tree, pstate, ring_state, capacity, n, seed: int = 0, draw: int = 0, out=None):
        """``(out_slot, out_priority)``: n slots drawn with replacement, each with probability priority / total, on the current
        stream (phx_prio_sample, include/phantom_amd_prio.h) -- i64 ``[n]`` and f32 ``[n]``, the slot and its leaf; -1 and +0.0 while
        nothing is held.  ``tree`` / ``pstate`` / ``ring_state`` are ``prio_add``'s (``pstate`` is checked, not read), the stream of
        draws is ``(seed, draw)``.  ``replay_sample(slots=out_slot)`` gathers the records.  ``out``: the two tensors, caller-owned and
        16-byte aligned; allocated here when None.  The call does not synchronise."""
        torch = _torch()
        Cn = self._prio_tree("prio_sample", tree, pstate, ring_state, capacity)
        n, seed, draw = _draws("prio_sample", n, seed, draw)
        oslot, oprio = self._outputs("prio_sample", out, ((torch.int64, (n,), REQUIRED), (torch.float32, (n,), REQUIRED)), "(out_slot, out_priority)")
        self._launch("phx_prio_sample", _abi.PhxPrioSampleIO(
            capacity=Cn, n=n, seed=seed, draw=draw, ring_state=_ptr(ring_state), tree=_ptr(tree), out_slot=_ptr(oslot), out_priority=_ptr(oprio)))
        return oslot, oprio

    def _filter_planes(self, fn, obs, state, keep, col_class, n_classes):
        """the arguments ``filter_update`` and ``filter_apply`` share, checked: ``(T, N, D, n_classes)``"""
        torch = _torch()
        if obs is None or not hasattr(obs, "dim") or obs.dim() < 3 or not 1 <= obs.shape[-1] <= _abi.FILTER_MAX_DIM:
            raise ValueError(f"{fn}: `obs` must be a [T, B, S, D] (or [T, N, D]) tensor with 1 <= D <= {_abi.FILTER_MAX_DIM}")
        shape, T, N = _rows_cols(fn, "`obs` has the leading shape", tuple(obs.shape[:-1]))
        D = int(obs.shape[-1])
        n_classes = _int(fn, "n_classes", n_classes, 1, _abi.FILTER_MAX_CLASSES)
        check_tensor(fn, "obs", obs, torch.float32, shape + (D,), align=16, device=self.device)
        check_tensor(fn, "state", state, torch.uint8, (n_classes, _abi.FILTER_STATE_BYTES), align=16, device=self.device)
        self._planes(fn, shape, (("keep", keep, torch.uint8, False),))
        if col_class is not None:
            check_tensor(fn, "col_class", col_class, torch.int32, (N,), device=self.device)
        return T, N, D, n_classes

    def filter_update(self, obs, state, keep=None, col_class=None, n_classes: int = 1, workspace=None):
        """Fold a time-major fragment's observations into a running mean / M2 per class and feature, on the current stream
        (phx_filter_update, include/phantom_amd_filter.h): five launches, no atomics, every f64 add in the header's fixed order, so the
        state is reproducible bit for bit.  ``obs`` is f32 ``[T, B, S, D]`` (or ``[T, N, D]``), D <= 16, 16-byte aligned, on the env's
        device; ``keep`` u8 of its leading shape (!= 0: the element counts; None: all do); ``col_class`` i32 ``[N]``, every column's
        class (None: all class 0; a value outside ``[0, n_classes)`` leaves the column out); ``state`` uint8 ``[n_classes, 272]``,
        records of ``_abi.FILTER_STATE_DTYPE`` (count, updates, mean[16], m2[16]), zero-filled once and 16-byte aligned, updated in
        place.  A class without a kept element keeps its bytes.  Kept values must be finite.  ``workspace``: f64
        ``[_abi.filter_workspace_bytes(N, D) // 8]`` scratch, 16-byte aligned; allocated here when None.  The call does not
        synchronise and returns ``state``."""
        torch = _torch()
        T, N, D, n_classes = self._filter_planes("filter_update", obs, state, keep, col_class, n_classes)
        words = _abi.filter_workspace_bytes(N, D) // 8
        if workspace is None:
            workspace = torch.empty((words,), dtype=torch.float64, device=self.device)
        check_tensor("filter_update", "workspace", workspace, torch.float64, (words,), align=16, device=self.device)
        self._launch("phx_filter_update", _abi.PhxFilterUpdateIO(
            T=T, D=D, N=N, n_classes=n_classes, obs=_ptr(obs), keep=_ptr(keep), col_class=_ptr(col_class), state=_ptr(state),
            workspace=_ptr(workspace)))
        return state

    def filter_apply(self, obs, state, keep=None, col_class=None, n_classes: int = 1, clip: float = 0.0, out=None):
        """``out``: a time-major plane normalised with a filter's state as it stands, in ONE launch on the current stream
        (phx_filter_apply, include/phantom_amd_filter.h).  ``obs`` / ``state`` / ``keep`` / ``col_class`` / ``n_classes`` are
        ``filter_update``'s; the state is read only.  A kept element of a class's column leaves as ``(x - mean_f) / den_f`` with
        ``mean_f = (float)mean`` and ``den_f = (float)sqrt(m2 / (count - 1)) + 1e-8f`` (count 1: ``sqrt(mean * mean)``), clamped to
        ``[-clip, clip]`` when ``clip > 0``; a class that has seen nothing copies its elements bit for bit; every other element is
        +0.0.  ``out``: f32 of ``obs``'s shape, 16-byte aligned -- ``obs`` itself for in place, any other overlap is refused;
        allocated here when None.  The call does not synchronise."""
        torch = _torch()
        T, N, D, n_classes = self._filter_planes("filter_apply", obs, state, keep, col_class, n_classes)
        clip32 = float(np.float32(clip)) if isinstance(clip, (int, float, np.floating, np.integer)) and not isinstance(clip, bool) else float("nan")
        if not clip32 >= 0.0:
            raise ValueError(f"filter_apply: clip = {clip!r} must be a number >= 0 (0: none)")
        out, = self._outputs("filter_apply", None if out is None else (out,), ((torch.float32, tuple(obs.shape), REQUIRED),))
        nbytes = obs.numel() * 4
        if out.data_ptr() != obs.data_ptr() and out.data_ptr() < obs.data_ptr() + nbytes and obs.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("filter_apply: `out` overlaps `obs` in part (pass `obs` itself for in place)")
        self._launch("phx_filter_apply", _abi.PhxFilterApplyIO(
            T=T, D=D, N=N, n_classes=n_classes, clip=clip32, obs=_ptr(obs), keep=_ptr(keep), col_class=_ptr(col_class), state=_ptr(state),
            out=_ptr(out)))
        return out
