"""Episode returns and lengths across rollout fragments, under RLlib's names (episode_reward_mean / min / max, episode_len_mean,
episodes_this_iter, policy_reward_mean): ``EpisodeStats`` keeps a carry per (env instance, agent) and per env instance on the device,
so that an episode one ``PhantomEnv.sample()`` call cuts is finished by the next, and folds what each call closed into running
totals on the host -- without a host wait per call (DeviceEnv.episode_stats, include/phantom_amd_episodes.h)."""
import numpy as np

from . import _abi

_NAN = float("nan")


class _Totals:
    """running totals of struct phx_episode_stats records, one per class: the integer fields and min / max exact, the f64 sums added
    in the order the records arrive"""

    def __init__(self, n):
        self.n = n
        self.clear()

    def clear(self):
        n = self.n
        self.count, self.len_sum = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.ret_sum, self.ret_sumsq = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self.ret_min, self.ret_max = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
        self.len_min, self.len_max = np.full(n, np.iinfo(np.int32).max, np.int32), np.full(n, -1, np.int32)

    def add(self, rec):
        """``rec``: a record array [n] of _abi.EPISODE_STATS_DTYPE (a call's summary)"""
        self.count += rec["count"]; self.len_sum += rec["len_sum"]
        self.ret_sum = self.ret_sum + rec["ret_sum"]; self.ret_sumsq = self.ret_sumsq + rec["ret_sumsq"]
        self.ret_min, self.ret_max = np.minimum(self.ret_min, rec["ret_min"]), np.maximum(self.ret_max, rec["ret_max"])
        self.len_min, self.len_max = np.minimum(self.len_min, rec["len_min"]), np.maximum(self.len_max, rec["len_max"])


def _stats(count, ret_sum, ret_min, ret_max, len_sum):
    """(mean, min, max, len_mean) of combined totals: the means in f64, NaN where nothing closed (as RLlib reports)"""
    if count == 0:
        return _NAN, _NAN, _NAN, _NAN
    return float(ret_sum) / count, float(ret_min), float(ret_max), float(len_sum) / count


class EpisodeStats:
    """``st = EpisodeStats(env)``; ``env.sample(T, episode_stats=st)`` any number of times; ``st.result()``.

    For the env's B instances and S strategic agents it holds two carries on the device -- per agent ``[B * S]`` and per env
    instance ``[B]``, each a (return so far f32, length so far i32; -1: no episode open) pair starting at (+0.0, -1) -- and running
    host totals per agent and for the env level.  ``update`` makes two ``DeviceEnv.episode_stats`` calls on a fragment's time-major
    planes: ``group=1, classes=S`` (an agent's episode: its own present rewards, the steps it acted in, closed by its own flags) and
    ``group=S, classes=1`` (the env's episode, RLlib's: every agent's rewards, the steps in which anybody acted, closed in the row
    where all agents carry a flag), and copies the two summaries, (S + 1) * 48 bytes, to pinned memory asynchronously; they are folded
    into the totals when ``result()`` is called (or, without waiting, by a later ``update`` once their copy has completed)."""

    def __init__(self, env, policy_mapping_fn=None):
        self.agent_ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
        self.B, self.S = int(env.batch_size), int(env.spec.n_strategic)
        self.policy_mapping_fn = policy_mapping_fn
        self.agents, self.envs = _Totals(self.S), _Totals(1)
        self._dev = None                                   # the DeviceEnv the device buffers live on (made at the first update)
        self._pending, self._free = [], []                 # (pinned u8 [S + 1, 48], event) pairs in flight / to reuse

    # ---- device side ---------------------------------------------------------------------------------------------------------------
    def _buffers(self, dev):
        import torch
        if self._dev is not dev:
            B, S, nb = self.B, self.S, _abi.EPISODE_STATS_BYTES
            e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev.device)
            self._dev = dev
            self._carry_agent = (e((B * S,), torch.float32), e((B * S,), torch.int32))
            self._carry_env = (e((B,), torch.float32), e((B,), torch.int32))
            self._col_agent, self._col_env = e((B * S, nb), torch.uint8), e((B, nb), torch.uint8)
            self._summary = e((S + 1, nb), torch.uint8)      # rows [0, S): per agent; row S: the env level
            self.drop_open()

    def drop_open(self):
        """forget the episodes that are open: both carries back to (+0.0, -1).  After an ``env.reset()`` that abandons running episodes"""
        if self._dev is not None:
            for ret, ln in (self._carry_agent, self._carry_env):
                ret.zero_()
                ln.fill_(-1)

    def update(self, dev, rewards, truncations, terminations=None, acted=None, reward_valid=None):
        """the episodes a fragment closes: ``[T, B, S]`` time-major device planes as ``dev``'s rollouts wrote them (``acted`` /
        ``reward_valid`` None on a plain env).  Two launches each for the agent and the env level and one asynchronous copy; no wait"""
        import torch
        if tuple(rewards.shape[1:]) != (self.B, self.S):
            raise ValueError(f"EpisodeStats.update: `rewards` has shape {tuple(rewards.shape)}, expected [T, {self.B}, {self.S}]")
        self._buffers(dev)
        S = self.S
        dev.episode_stats(rewards, truncations, terminations, acted, reward_valid, group=1, classes=S, carry=self._carry_agent,
                          out=(self._col_agent, self._summary[:S], None, None))
        dev.episode_stats(rewards, truncations, terminations, acted, reward_valid, group=S, classes=1, carry=self._carry_env,
                          out=(self._col_env, self._summary[S:], None, None))
        self._fold(wait=False)
        if self._free:
            pin, ev = self._free.pop()
        else:
            pin, ev = torch.empty(tuple(self._summary.shape), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()
        with torch.cuda.device(dev.device):
            pin.copy_(self._summary, non_blocking=True)
            ev.record(torch.cuda.current_stream(dev.device))
        self._pending.append((pin, ev))

    # ---- host side -----------------------------------------------------------------------------------------------------------------
    def _fold(self, wait):
        """the summaries whose copy has arrived (wait=True: all of them) into the totals, in call order"""
        while self._pending:
            pin, ev = self._pending[0]
            if wait:
                ev.synchronize()
            elif not ev.query():
                break
            self.add_summaries(pin.numpy().reshape(-1).view(_abi.EPISODE_STATS_DTYPE))
            self._free.append(self._pending.pop(0))

    def add_summaries(self, rec):
        """fold one call's summaries: a record array [S + 1] of _abi.EPISODE_STATS_DTYPE, rows [0, S) per agent, row S the env level"""
        rec = np.asarray(rec)
        if rec.shape != (self.S + 1,):
            raise ValueError(f"EpisodeStats.add_summaries: {rec.shape} records, expected {self.S + 1}")
        self.agents.add(rec[:self.S])
        self.envs.add(rec[self.S:])

    def result(self, reset: bool = True, policy_mapping_fn=None):
        """RLlib's numbers over everything folded since the last reset: ``episodes_this_iter``, ``episode_reward_mean`` / ``_min`` /
        ``_max`` and ``episode_len_mean`` (the env's episodes); ``agent_reward_mean`` / ``_min`` / ``_max`` and
        ``agent_episode_len_mean``, dicts keyed by agent id (an agent's own episodes); with a ``policy_mapping_fn`` (here or at
        construction) ``policy_reward_mean`` / ``_min`` / ``_max`` keyed by policy id, the episodes of a policy's agents taken
        together as RLlib groups them.  A mean is ret_sum / count in f64; where nothing closed every number is NaN.  ``reset=True``
        clears the totals, never the carries: an episode that is open goes on"""
        self._fold(wait=True)
        e, a = self.envs, self.agents
        mean, lo, hi, ln = _stats(int(e.count[0]), e.ret_sum[0], e.ret_min[0], e.ret_max[0], int(e.len_sum[0]))
        out = {"episodes_this_iter": int(e.count[0]), "episode_reward_mean": mean, "episode_reward_min": lo, "episode_reward_max": hi,
               "episode_len_mean": ln}
        per = [_stats(int(a.count[s]), a.ret_sum[s], a.ret_min[s], a.ret_max[s], int(a.len_sum[s])) for s in range(self.S)]
        for i, name in enumerate(("agent_reward_mean", "agent_reward_min", "agent_reward_max", "agent_episode_len_mean")):
            out[name] = {aid: per[s][i] for s, aid in enumerate(self.agent_ids)}
        fn = policy_mapping_fn or self.policy_mapping_fn
        if fn is not None:
            groups = {}
            for s, aid in enumerate(self.agent_ids):
                groups.setdefault(fn(aid), []).append(s)
            pol = {}
            for pid, members in groups.items():          # (the f64 sums in agent order)
                count = sum(int(a.count[s]) for s in members)
                ret_sum = 0.0
                for s in members:
                    ret_sum = ret_sum + float(a.ret_sum[s])
                pol[pid] = _stats(count, ret_sum, min(a.ret_min[s] for s in members), max(a.ret_max[s] for s in members),
                                  sum(int(a.len_sum[s]) for s in members))
            for i, name in enumerate(("policy_reward_mean", "policy_reward_min", "policy_reward_max")):
                out[name] = {pid: v[i] for pid, v in pol.items()}
        if reset:
            self.agents.clear()
            self.envs.clear()
        return out
