"""Bulk exits of a device rollout fragment (VERDICT r3 Missing #4 / Next #2).

The reference builds, per env instance and per step, a ``Step`` of five dicts and collects them in a ``Rollout``
(phantom/utils/rllib/rollout.py:300-408, containers phantom/utils/rollout.py); RLlib's samplers build per-(env, agent)
trajectories and concatenate them into ``SampleBatch`` columns.  Here the whole fragment ``[T, B, S, ..]`` is already
on the device: ``FragmentBatch`` brings it to the host ONCE (transposed on the device to ``[B, S, T, ..]`` so that an
agent's steps are contiguous, one pinned copy per column) and offers

* ``to_sample_batches()`` -- per-policy column dicts with RLlib's ``SampleBatch`` column names (``obs, new_obs, actions,
  rewards, terminateds, truncateds, eps_id, agent_index, t``): numpy reshapes of the host arrays, no python object per
  (env, agent, step);
* ``rollouts()`` -- the reference's own containers (``Rollout`` / ``Step`` / ``AgentStep`` with the reference's field
  names and helper methods), built LAZILY from the same arrays: a ``Step`` of dicts exists only while somebody looks at it.

Conventions (rollout.py:361-408): step ``i`` of an episode holds the observations the policies acted on (those returned
by ``reset`` or by step ``i - 1``), the actions taken, and the rewards / terminations / truncations / infos that
``env.step`` returned.  The trajectory planes store an agent's done flag OR-ed with ``"__all__"`` (device.Trajectory);
``"__all__"`` is recovered as the AND over the strategic agents (env.py:297-301).
"""
from collections import Counter
from collections.abc import Sequence
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterable, List, Mapping, Optional, Tuple

import numpy as np

from .batch import DeviceBatch, DeviceSeqBatch  # noqa: F401  (sample(batcher=...)'s results: records on the device, next to the two host forms)

DEFAULT_POLICY_ID = "default_policy"          # ray.rllib.policy.sample_batch.DEFAULT_POLICY_ID


@dataclass(frozen=True)
class AgentStep:
    """One agent's view of one step (phantom/utils/rollout.py:22-32).  The reference's ``Rollout.steps_for_agent`` passes
    terminations and truncations as two positional values into this seven-field record (a TypeError there); here ``done``
    is their OR."""
    i: int
    observation: Optional[Any]
    reward: Optional[float]
    done: bool
    info: Optional[Dict[str, Any]]
    action: Optional[Any]
    stage: Optional[Any] = None


@dataclass(frozen=True)
class Step:
    """One step of one episode (phantom/utils/rollout.py:35-47)."""
    i: int
    observations: Dict[Any, Any]
    rewards: Dict[Any, float]
    terminations: Dict[Any, bool]
    truncations: Dict[Any, bool]
    infos: Dict[Any, Dict[str, Any]]
    actions: Dict[Any, Any]
    messages: Optional[List[Any]] = None
    stage: Optional[Any] = None


class _Steps(Sequence):
    """``Rollout.steps`` over the arrays of a FragmentBatch: episode rows [t0, t0 + n) of env instance b."""

    def __init__(self, frag: "FragmentBatch", b: int, t0: int, n: int):
        self._f, self._b, self._t0, self._n = frag, b, t0, n

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._f.step(self._b, self._t0 + i, i)


class Rollout:
    """One episode of one env instance (phantom/utils/rollout.py:50-57): same fields, same helper methods; ``steps`` is a
    lazy sequence (or any list of ``Step``)."""

    def __init__(self, rollout_id: int, repeat_id: int, env_config: Mapping[str, Any], rollout_params: Dict[str, Any],
                 steps: Sequence, metrics: Dict[str, np.ndarray]):
        self.rollout_id, self.repeat_id = rollout_id, repeat_id
        self.env_config, self.rollout_params = env_config, rollout_params
        self.steps, self.metrics = steps, metrics

    def _column(self, field: str, agent_id, drop_nones: bool, stages, none_values: bool = False) -> list:
        out = []
        for step in self.steps:
            if stages is not None and step.stage not in stages:
                continue
            d = getattr(step, field)
            if agent_id in d and not (none_values and drop_nones and d[agent_id] is None):
                out.append(d[agent_id])
            elif not drop_nones:
                out.append(None)
        return out

    def observations_for_agent(self, agent_id, drop_nones: bool = False, stages: Optional[Iterable] = None) -> list:
        return self._column("observations", agent_id, drop_nones, stages)

    def rewards_for_agent(self, agent_id, drop_nones: bool = False, stages: Optional[Iterable] = None) -> list:
        return self._column("rewards", agent_id, drop_nones, stages, none_values=True)

    def terminations_for_agent(self, agent_id, drop_nones: bool = False, stages: Optional[Iterable] = None) -> list:
        return self._column("terminations", agent_id, drop_nones, stages)

    def truncations_for_agent(self, agent_id, drop_nones: bool = False, stages: Optional[Iterable] = None) -> list:
        return self._column("truncations", agent_id, drop_nones, stages)

    def infos_for_agent(self, agent_id, drop_nones: bool = False, stages: Optional[Iterable] = None) -> list:
        return self._column("infos", agent_id, drop_nones, stages)

    def actions_for_agent(self, agent_id, drop_nones: bool = False, stages: Optional[Iterable] = None) -> list:
        return self._column("actions", agent_id, drop_nones, stages)

    def steps_for_agent(self, agent_id, stages: Optional[Iterable] = None) -> List[AgentStep]:
        out = []
        for step in self.steps:
            if stages is not None and step.stage not in stages:
                continue
            term, trunc = step.terminations.get(agent_id), step.truncations.get(agent_id)
            done = None if term is None and trunc is None else bool(term) or bool(trunc)
            out.append(AgentStep(step.i, step.observations.get(agent_id), step.rewards.get(agent_id), done,
                                 step.infos.get(agent_id), step.actions.get(agent_id), step.stage))
        return out

    @staticmethod
    def _hashable(a):
        return a.tobytes() if isinstance(a, np.ndarray) else a

    def count_actions(self, stages: Optional[Iterable] = None) -> List[Tuple[Any, int]]:
        vals = [a for step in self.steps if stages is None or step.stage in stages for a in step.actions.values()]
        return self._count(vals)

    def count_agent_actions(self, agent_id, stages: Optional[Iterable] = None) -> List[Tuple[Any, int]]:
        return self._count([step.actions.get(agent_id) for step in self.steps if stages is None or step.stage in stages])

    def _count(self, vals) -> List[Tuple[Any, int]]:
        # (the reference counts the action objects themselves; numpy arrays are not hashable, so equal arrays are grouped by value)
        first, cnt = {}, Counter()
        for v in vals:
            k = self._hashable(v)
            first.setdefault(k, v)
            cnt[k] += 1
        return [(first[k], n) for k, n in cnt.most_common()]

    def __getitem__(self, index: int):
        return self.steps[index]

    def __repr__(self):
        return f"Rollout(rollout_id={self.rollout_id}, repeat_id={self.repeat_id}, steps={len(self.steps)})"


NSTEP_COLUMNS = ("nstep_rewards", "nstep_discounts", "nstep_new_obs", "nstep_terminateds", "nstep_truncateds")


class FragmentBatch:
    """A rollout fragment on the host, agent-major: every array is ``[B, S, T, ..]`` (env instance, strategic agent, step).

    ``obs``       f32 [B, S, T, D]  what the policy saw before step t        ``new_obs``   f32 [B, S, T, D]  what step t returned
    ``actions``   f32 [B, S, T]                                             ``rewards``   f32 [B, S, T]
    ``terminateds`` / ``truncateds``  bool [B, S, T]  (agent flag OR ``"__all__"``)
    ``obs_valid`` / ``new_obs_valid`` u8 [B, S, T] or None (FSM / Stackelberg envs: key present in the dict),
    ``reward_valid`` u8 [B, S, T] or None (0 absent / 1 value / 2 present-but-None, fsm.py:378)
    ``t``         i32 [B, T] step inside the episode (0-based)              ``eps_id``  i64 [B, T] episode counter * B + b
    ``stage``     i32 [B, T] or None: the stage the step ran in (``previous_stage`` after it, rollout.py:389-391)
    an exploring policy's fragment (PhantomEnv.sample(explore=True)), else None:
    ``raw_actions`` f32 [B, S, T] the Gaussian draw z (``actions`` stays what the env took: clip(out_scale z + out_bias))
    ``action_logp`` f32 [B, S, T] log N(z; mean, exp(log_std))              ``dist_inputs`` f32 [B, S, T, 2] (mean, log_std)
    a fragment sampled with a critic (PhantomEnv.sample(value_fn=...)), else None -- RLlib's columns of the same names:
    ``vf_preds`` f32 [B, S, T] V(obs)       ``advantages`` / ``value_targets`` f32 [B, S, T] (DeviceEnv.gae / gae_masked)
    ``trajectory_rewards`` f32 [B, S, T] or None (FSM / Stackelberg fragments of PhantomEnv.sample): at the rows where the agent
    acted, the sum of the rewards that arrived until its next observation (DeviceEnv.gae_masked); ``rewards`` stays step-aligned
    ``trajectory_next_row`` i32 [B, S, T], ``trajectory_new_obs`` f32 [B, S, T, D], ``trajectory_terminateds`` / ``trajectory_truncateds``
    bool [B, S, T], or None (FSM / Stackelberg fragments of PhantomEnv.sample; DeviceEnv.traj_next): at the rows where the agent acted,
    the fragment row whose ``new_obs`` it holds when its transition ends (-1: none, it still holds ``obs``), that observation, and the done
    flags of the step that ended the transition; -1 / +0.0 / False elsewhere.  ``new_obs`` / ``terminateds`` / ``truncateds`` stay
    step-aligned.  A kept row is a COMPLETE transition iff it carries a flag or ``trajectory_next_row >= 0``; the one row that can be
    incomplete is the (env instance, agent)'s last trajectory row of the fragment -- its answer lies in the next fragment
    an off-policy learner's fragment (PhantomEnv.sample(target_logp_fn=...)), else None -- ``advantages`` / ``value_targets`` are None then:
    ``target_logp`` f32 [B, S, T] the learner's log-density of the recorded draws
    ``vtrace_vs`` / ``vtrace_pg_advantages`` f32 [B, S, T] V-trace value targets and policy-gradient advantages (DeviceEnv.vtrace)
    a replay learner's fragment (PhantomEnv.sample(n_step=n)), else None -- DeviceEnv.nstep over the agent's own transitions:
    ``nstep_rewards`` f32 [B, S, T] the discounted sum of the rewards of the (up to n) transitions folded at the row
    ``nstep_discounts`` f32 [B, S, T] gamma to the number of transitions folded: what to multiply Q(``nstep_new_obs``) with
    ``nstep_new_obs`` f32 [B, S, T, D], ``nstep_terminateds`` / ``nstep_truncateds`` bool [B, S, T] the next observation and the done
    flags of the last transition folded; +0.0 / False at rows where the agent did not act.  The one-step fields stay as they are
    """

    COLUMNS = ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")

    def __init__(self, agent_ids, obs, new_obs, actions, rewards, terminateds, truncateds, t, eps_id,
                 obs_valid=None, new_obs_valid=None, reward_valid=None, stage=None, stage_ids=None,
                 action_shape=(1,), never_finishes_alone: bool = True, done_valid=None, raw_actions=None, action_logp=None,
                 dist_inputs=None, vf_preds=None, advantages=None, value_targets=None, trajectory_rewards=None, target_logp=None,
                 vtrace_vs=None, vtrace_pg_advantages=None, trajectory_next_row=None, trajectory_new_obs=None,
                 trajectory_terminateds=None, trajectory_truncateds=None, nstep_rewards=None, nstep_discounts=None, nstep_new_obs=None,
                 nstep_terminateds=None, nstep_truncateds=None):
        self.agent_ids = list(agent_ids)
        self.obs, self.new_obs, self.actions, self.rewards = obs, new_obs, actions, rewards
        self.terminateds, self.truncateds, self.t, self.eps_id = terminateds, truncateds, t, eps_id
        self.obs_valid, self.new_obs_valid, self.reward_valid = obs_valid, new_obs_valid, reward_valid
        self.stage, self.stage_ids = stage, stage_ids
        self.done_valid = done_valid                 # u8 [B, S, T] or None (None: every strategic agent has done flags in every step)
        self.action_shape = tuple(action_shape)
        self.never_finishes_alone = never_finishes_alone
        self.raw_actions, self.action_logp, self.dist_inputs = raw_actions, action_logp, dist_inputs
        self.vf_preds, self.advantages, self.value_targets = vf_preds, advantages, value_targets
        self.trajectory_rewards = trajectory_rewards
        self.trajectory_next_row, self.trajectory_new_obs = trajectory_next_row, trajectory_new_obs
        self.trajectory_terminateds, self.trajectory_truncateds = trajectory_terminateds, trajectory_truncateds
        self.target_logp, self.vtrace_vs, self.vtrace_pg_advantages = target_logp, vtrace_vs, vtrace_pg_advantages
        self.nstep_rewards, self.nstep_discounts, self.nstep_new_obs = nstep_rewards, nstep_discounts, nstep_new_obs
        self.nstep_terminateds, self.nstep_truncateds = nstep_terminateds, nstep_truncateds
        self.B, self.S, self.T = obs.shape[0], obs.shape[1], obs.shape[2]

    # ---- RLlib-shaped exit -------------------------------------------------------------------------------------------
    def to_sample_batches(self, policy_mapping_fn: Optional[Callable[[Any], str]] = None) -> Dict[str, Dict[str, np.ndarray]]:
        """{policy_id: {column: array}} with ``SampleBatch``'s column names.  Rows are ordered (env instance, agent, step):
        an agent's episode is a contiguous run, as in RLlib's per-agent trajectories.  ``policy_mapping_fn(agent_id)``
        (default: everything under ``"default_policy"``).  Agents of one policy that are consecutive in agent order come
        out as reshaped VIEWS of the host arrays (no copy); envs whose dicts omit keys (FSM / Stackelberg) drop the rows of
        absent observations (boolean mask: a copy).  An exploring fragment's ``actions`` column is the raw draw z (what RLlib's
        sampler records), next to ``action_logp``, ``action_prob`` = exp(action_logp) and ``action_dist_inputs``; a fragment with
        ``vf_preds`` / ``advantages`` / ``value_targets`` / ``target_logp`` / ``vtrace_vs`` / ``vtrace_pg_advantages`` has the columns
        of those names; a fragment with ``trajectory_rewards``
        takes its ``rewards`` column from them (an action's reward is what arrived until the agent's next observation), and one with
        ``trajectory_new_obs`` / ``trajectory_terminateds`` / ``trajectory_truncateds`` its ``new_obs`` / ``terminateds`` / ``truncateds``
        columns from those (the agent's next observation and the flags of the step that ended its transition), plus a
        ``trajectory_next_row`` column: a row is a complete transition iff it carries a flag or ``trajectory_next_row >= 0`` (only an
        agent's last row of the fragment can be incomplete).  A fragment with ``nstep_rewards`` / ``nstep_discounts`` / ``nstep_new_obs`` /
        ``nstep_terminateds`` / ``nstep_truncateds`` has the columns of those names next to the one-step ones."""
        fn = policy_mapping_fn or (lambda aid: DEFAULT_POLICY_ID)
        groups: Dict[str, List[int]] = {}
        for s, aid in enumerate(self.agent_ids):
            groups.setdefault(fn(aid), []).append(s)
        B, T = self.B, self.T
        out = {}
        for pid, idx in groups.items():
            n = len(idx)
            contiguous = idx == list(range(idx[0], idx[0] + n))
            sel = (lambda a: a[:, idx[0]:idx[0] + n]) if contiguous else (lambda a: a[:, idx])
            cols = {
                "obs": sel(self.obs).reshape(B * n * T, -1),
                "new_obs": sel(self.new_obs).reshape(B * n * T, -1),
                "actions": sel(self.actions).reshape((B * n * T,) + self.action_shape),
                "rewards": sel(self.rewards).reshape(-1),
                "terminateds": sel(self.terminateds).reshape(-1),
                "truncateds": sel(self.truncateds).reshape(-1),
                "eps_id": np.broadcast_to(self.eps_id[:, None, :], (B, n, T)).reshape(-1),
                "agent_index": np.broadcast_to(np.asarray(idx, dtype=np.int32)[None, :, None], (B, n, T)).reshape(-1),
                "t": np.broadcast_to(self.t[:, None, :], (B, n, T)).reshape(-1),
                "env_id": np.broadcast_to(np.arange(B, dtype=np.int32)[:, None, None], (B, n, T)).reshape(-1),
            }
            if self.raw_actions is not None:
                cols["actions"] = sel(self.raw_actions).reshape((B * n * T,) + self.action_shape)
                cols["action_logp"] = sel(self.action_logp).reshape(-1)
                cols["action_prob"] = np.exp(cols["action_logp"])
                cols["action_dist_inputs"] = sel(self.dist_inputs).reshape(B * n * T, -1)
            if self.trajectory_rewards is not None:
                cols["rewards"] = sel(self.trajectory_rewards).reshape(-1)
            if self.trajectory_new_obs is not None:
                cols["new_obs"] = sel(self.trajectory_new_obs).reshape(B * n * T, -1)
            if self.trajectory_terminateds is not None:
                cols["terminateds"] = sel(self.trajectory_terminateds).reshape(-1)
            if self.trajectory_truncateds is not None:
                cols["truncateds"] = sel(self.trajectory_truncateds).reshape(-1)
            if self.trajectory_next_row is not None:
                cols["trajectory_next_row"] = sel(self.trajectory_next_row).reshape(-1)
            for name in ("vf_preds", "advantages", "value_targets", "target_logp", "vtrace_vs", "vtrace_pg_advantages"):
                if getattr(self, name) is not None:
                    cols[name] = sel(getattr(self, name)).reshape(-1)
            for name in NSTEP_COLUMNS:
                if getattr(self, name) is not None:
                    x = sel(getattr(self, name))
                    cols[name] = x.reshape(B * n * T, -1) if name == "nstep_new_obs" else x.reshape(-1)
            if self.obs_valid is not None:
                keep = sel(self.obs_valid).reshape(-1).astype(bool)
                cols = {k: v[keep] for k, v in cols.items()}
            out[pid] = cols
        return out

    # ---- the reference's containers ------------------------------------------------------------------------------------
    def episodes(self) -> List[Tuple[int, int]]:
        """(first row, length) of every episode piece of the fragment (all env instances run in lock-step)."""
        t = self.t[0]
        starts = [0] + [k for k in range(1, self.T) if t[k] != t[k - 1] + 1]
        return [(a, (starts[i + 1] if i + 1 < len(starts) else self.T) - a) for i, a in enumerate(starts)]

    def step(self, b: int, row: int, i: Optional[int] = None) -> Step:
        """the reference's ``Step`` for env instance b, fragment row ``row`` (dicts built here, on demand)."""
        ids = self.agent_ids
        ov = self.obs_valid[b, :, row] if self.obs_valid is not None else None
        nv = self.new_obs_valid[b, :, row] if self.new_obs_valid is not None else None
        rv = self.reward_valid[b, :, row] if self.reward_valid is not None else None
        term, trunc = self.terminateds[b, :, row], self.truncateds[b, :, row]
        all_t, all_u = bool(term.all()), bool(trunc.all())
        own = (lambda flag, allf: False if (allf and self.never_finishes_alone) else bool(flag))
        obs = {a: self.obs[b, s, row] for s, a in enumerate(ids) if ov is None or ov[s]}
        acts = {a: np.asarray(self.actions[b, s, row], dtype=np.float32).reshape(self.action_shape)
                for s, a in enumerate(ids) if a in obs}
        rew = {a: (None if rv is not None and rv[s] == 2 else float(self.rewards[b, s, row]))
               for s, a in enumerate(ids) if (rv[s] != 0 if rv is not None else True)}
        # done flags: every strategic agent that was live when the step began (env.py:285-292, fsm.py:333-340: the loop runs over the
        # strategic agents, not over the observing ones); infos: the agents that got an observation (env.py:279-283)
        dv = self.done_valid[b, :, row] if self.done_valid is not None else None
        terms = {ids[s]: own(term[s], all_t) for s in range(len(ids)) if dv is None or dv[s]}
        truncs = {ids[s]: own(trunc[s], all_u) for s in range(len(ids)) if dv is None or dv[s]}
        terms["__all__"], truncs["__all__"] = all_t, all_u
        infos = {ids[s]: {} for s in range(len(ids)) if nv is None or nv[s]}
        st = None
        if self.stage is not None:
            k = int(self.stage[b, row])
            st = self.stage_ids[k] if self.stage_ids is not None else k
        return Step(int(self.t[b, row]) if i is None else i, obs, rew, terms, truncs, infos, acts, None, st)

    def rollouts(self, rollout_ids: Optional[Sequence] = None, repeat_ids: Optional[Sequence] = None,
                 env_configs: Optional[Sequence] = None, rollout_params: Optional[Sequence] = None,
                 metrics: Optional[Sequence] = None) -> List[Rollout]:
        """One ``Rollout`` per (episode piece, env instance), episode-major; the per-instance attributes default to the
        instance index / 0 / {}."""
        out = []
        for t0, n in self.episodes():
            for b in range(self.B):
                out.append(Rollout(rollout_ids[b] if rollout_ids is not None else b,
                                   repeat_ids[b] if repeat_ids is not None else 0,
                                   env_configs[b] if env_configs is not None else {},
                                   rollout_params[b] if rollout_params is not None else {},
                                   _Steps(self, b, t0, n),
                                   metrics[b] if metrics is not None else {}))
        return out


class CompactFragment:
    """The rows of an FSM / Stackelberg fragment where an agent acted, and nothing else: what ``PhantomEnv.sample(compact=True)``
    returns.  The hole rows were dropped on the device (``DeviceEnv.compact``, include/phantom_amd_compact.h), so every array here is
    already in ``to_sample_batches()``'s row order -- (env instance, agent, step) -- and K rows long.

    ``agent_ids``; ``B``, ``S``, ``T`` as in ``FragmentBatch``; ``K`` the number of kept rows
    ``col_start`` i64 [B * S + 1]: the rows of (env instance b, agent s) are ``[col_start[b * S + s], col_start[b * S + s + 1])``
    ``row``       i32 [K] the fragment row (step) of every kept row
    ``t``         i32 [B, T], ``eps_id`` i64 [B, T] as in ``FragmentBatch``
    ``columns``   {name: [K, ..] host array} under ``to_sample_batches()``'s column names: ``obs``, ``new_obs`` (the agent's NEXT
                  observation), ``actions``, ``rewards`` (the transition's), ``terminateds`` / ``truncateds`` (bool, the transition's),
                  ``trajectory_next_row`` (a FRAGMENT row, as in ``FragmentBatch``), with a critic ``vf_preds`` / ``advantages`` /
                  ``value_targets``, with ``n_step`` ``nstep_rewards`` / ``nstep_discounts`` / ``nstep_new_obs`` / ``nstep_terminateds`` /
                  ``nstep_truncateds`` (the flags bool)

    The arrays of a fragment that ``sample(compact=True)`` returned are views of host buffers the env keeps: they hold until the
    env's next ``sample(compact=True)`` call.  There is no ``rollouts()`` / ``step()`` here -- the step-aligned planes never left the
    device: use ``compact=False`` for the reference's containers."""

    ORDER = ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")

    def __init__(self, agent_ids, B: int, S: int, T: int, col_start, row, t, eps_id, columns):
        self.agent_ids = list(agent_ids)
        self.B, self.S, self.T = int(B), int(S), int(T)
        self.col_start, self.row, self.t, self.eps_id = col_start, row, t, eps_id
        self.K = int(col_start[-1])
        self.columns = dict(columns)
        if len(self.agent_ids) != self.S or col_start.shape != (self.B * self.S + 1,) or row.shape != (self.K,):
            raise ValueError("CompactFragment: col_start is [B * S + 1], row is [K = col_start[-1]] and there is one agent id per S")
        for k, v in self.columns.items():
            if v.shape[0] != self.K:
                raise ValueError(f"CompactFragment: column `{k}` has {v.shape[0]} rows, expected K = {self.K}")

    @classmethod
    def from_time_major(cls, agent_ids, keep, columns, t, eps_id, action_shape=(1,)):
        """from TIME-major host arrays, by the numpy restatement of the compaction: ``keep`` u8 / bool [T, B, S], every column
        [T, B, S, ..] under its ``to_sample_batches()`` name (``terminateds`` / ``truncateds`` become bool, ``actions`` take
        ``action_shape``), ``t`` / ``eps_id`` [B, T]"""
        keep = np.asarray(keep)
        T, B, S = keep.shape
        km = np.moveaxis(keep, 0, 2) != 0                                 # [B, S, T]
        col_start = np.zeros(B * S + 1, dtype=np.int64)
        np.cumsum(km.reshape(B * S, T).sum(axis=1), out=col_start[1:])
        row = np.broadcast_to(np.arange(T, dtype=np.int32), (B, S, T))[km]
        cols = {}
        for k, v in columns.items():
            c = np.moveaxis(np.asarray(v), 0, 2)[km]
            if k in ("terminateds", "truncateds"):
                c = c.astype(bool)
            elif k == "actions":
                c = c.reshape((len(c),) + tuple(action_shape))
            elif k in ("obs", "new_obs"):
                c = c.reshape(len(c), int(np.prod(c.shape[1:])))
            cols[k] = c
        return cls(agent_ids, B, S, T, col_start, row, t, eps_id, cols)

    def to_sample_batches(self, policy_mapping_fn: Optional[Callable[[Any], str]] = None) -> Dict[str, Dict[str, np.ndarray]]:
        """what ``FragmentBatch.to_sample_batches`` returns for the same fragment, key for key and array for array.  With every agent
        under one policy the columns are ``self.columns``' arrays themselves (no copy); a policy that owns a subset of the agents
        takes its agents' ranges from ``col_start`` (one indexed copy per column).  ``eps_id``, ``t``, ``env_id`` and ``agent_index``
        are derived here from ``row`` and ``col_start``."""
        fn = policy_mapping_fn or (lambda aid: DEFAULT_POLICY_ID)
        groups: Dict[str, List[int]] = {}
        for s, aid in enumerate(self.agent_ids):
            groups.setdefault(fn(aid), []).append(s)
        B, S = self.B, self.S
        counts = np.diff(self.col_start)
        col = np.repeat(np.arange(B * S, dtype=np.int32), counts)         # the column of every kept row
        env_id, agent_index = col // S, col % S
        derived = {"eps_id": self.eps_id[env_id, self.row], "agent_index": agent_index, "t": self.t[env_id, self.row], "env_id": env_id}
        names = list(self.ORDER) + list(derived) + [k for k in self.columns if k not in self.ORDER]
        out = {}
        for pid, idx in groups.items():
            if idx == list(range(S)):
                sel = lambda a: a
            else:
                cols_of = (np.arange(B)[:, None] * S + np.asarray(idx)[None, :]).reshape(-1)
                first, n = self.col_start[cols_of], counts[cols_of]
                rows = np.repeat(first - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))
                sel = lambda a: a[rows]
            out[pid] = {k: sel(self.columns[k] if k in self.columns else derived[k]) for k in names if k in self.columns or k in derived}
        return out


def fragment_from_arrays(agent_ids, first_obs, new_obs, actions, rewards, terminated, truncated, num_steps: int, step0,
                         reset_obs: Optional[Dict[int, np.ndarray]] = None, obs_valid=None, reward_valid=None,
                         first_obs_valid=None, stage=None, stage_ids=None, episode0: int = 0,
                         never_finishes_alone: bool = True) -> FragmentBatch:
    """FragmentBatch from TIME-major host arrays (an oracle rollout, a golden): ``new_obs`` [T, B, S, D], the others
    [T, B, S]; ``first_obs`` [B, S, D] = what the policies saw before row 0; ``step0`` = the env's step counter before
    row 0 (int); ``reset_obs[row]`` [B, S, D] = the observation ``env.reset()`` returned before row ``row`` (needed where an
    episode starts inside the fragment)."""
    T, B, S = actions.shape
    tm = lambda a: np.ascontiguousarray(np.moveaxis(a, 0, 2))            # [T, B, S, ..] -> [B, S, T, ..]
    nob = tm(new_obs)
    obs = np.empty_like(nob)
    obs[:, :, 0] = first_obs
    obs[:, :, 1:] = nob[:, :, :-1]
    t = (int(step0) + np.arange(T)) % num_steps
    ep = episode0 + (int(step0) + np.arange(T)) // num_steps
    nv = tm(obs_valid) if obs_valid is not None else None
    ov = None
    if nv is not None:
        ov = np.empty_like(nv)
        ov[:, :, 0] = first_obs_valid if first_obs_valid is not None else 1
        ov[:, :, 1:] = nv[:, :, :-1]
    for row in range(1, T):
        if t[row] == 0:
            if reset_obs is None or row not in reset_obs:
                raise ValueError(f"an episode starts at fragment row {row}: its reset observation is needed (reset_obs[{row}])")
            obs[:, :, row] = reset_obs[row]
            if ov is not None:
                ov[:, :, row] = 1
    return FragmentBatch(agent_ids, obs, nob, tm(actions), tm(rewards).astype(np.float32), tm(terminated).astype(bool),
                         tm(truncated).astype(bool), np.broadcast_to(t.astype(np.int32), (B, T)).copy(),
                         (ep[None, :] * B + np.arange(B)[:, None]).astype(np.int64), ov, nv,
                         tm(reward_valid) if reward_valid is not None else None,
                         np.ascontiguousarray(stage.T) if stage is not None else None, stage_ids,
                         never_finishes_alone=never_finishes_alone)
