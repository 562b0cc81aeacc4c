"""RLlib's ``observation_filter="MeanStdFilter"`` on the device: ``ObsFilter`` keeps a running count, mean and M2 of every observation
feature per policy in 272 device bytes per policy, folds a ``PhantomEnv.sample()`` fragment into them with one
``DeviceEnv.filter_update`` call and normalises the fragment's observation planes with ``DeviceEnv.filter_apply``
(include/phantom_amd_filter.h).  Every sum is taken in a fixed order, so the statistics -- and the normalised columns -- are
reproducible bit for bit.  Nothing waits for the device but ``stats()``."""
import numpy as np

from . import _abi
from .batch import DEFAULT_POLICY_ID


class ObsFilter:
    """``f = ObsFilter(env)``; ``env.sample(T, obs_filter=f, batcher=...)`` any number of times.

    ``policy_mapping_fn(agent_id)`` splits the strategic agents into policies as ``TrainBatcher`` does (default: one,
    ``"default_policy"``; at most 16); a policy is a CLASS of the fragment's columns and has its own statistics.  ``clip``: the
    normalised values are clamped to ``[-clip, clip]`` (RLlib's ``clip``); None: no clamp -- the form a device policy needs, see
    ``fold``.  A policy that has seen nothing is the identity, clamp included.

    ``sample(obs_filter=f)`` applies, then updates: both observation planes of a call are normalised with the statistics as they
    stood when the call began -- the ones a folded device policy acted under during that call -- and only then are the call's raw
    ``obs`` rows folded in.  The first call with a fresh filter therefore returns raw observations."""

    def __init__(self, env, policy_mapping_fn=None, clip=10.0):
        if clip is not None:
            if isinstance(clip, bool) or not isinstance(clip, (int, float, np.floating, np.integer)) or not float(np.float32(clip)) > 0.0 \
                    or not np.isfinite(np.float32(clip)):
                raise ValueError(f"ObsFilter: clip = {clip!r} must be None or a finite number > 0")
        self.clip = None if clip is None else float(np.float32(clip))
        self.agent_ids = [env.spec.agent_ids[a] for a in env.spec.strategic_idx]
        self.B, self.S, self.D = int(env.batch_size), int(env.spec.n_strategic), int(env.spec.obs_dim)
        if not 1 <= self.D <= _abi.FILTER_MAX_DIM:
            raise ValueError(f"ObsFilter: observations of {self.D} features, the filter serves 1 .. {_abi.FILTER_MAX_DIM}")
        fn = policy_mapping_fn or (lambda aid: DEFAULT_POLICY_ID)
        self.policies = {}                                   # policy id -> its agents' indices, in agent order
        for s, aid in enumerate(self.agent_ids):
            self.policies.setdefault(fn(aid), []).append(s)
        if len(self.policies) > _abi.FILTER_MAX_CLASSES:
            raise ValueError(f"ObsFilter: {len(self.policies)} policies, one filter holds at most {_abi.FILTER_MAX_CLASSES}")
        self.n_classes = len(self.policies)
        self.agent_class = np.zeros(self.S, np.int32)
        for c, idx in enumerate(self.policies.values()):
            self.agent_class[idx] = c
        self._host = np.zeros(self.n_classes, _abi.FILTER_STATE_DTYPE)       # the state while no device holds it, and stats()'s copy
        self._dev = self._state = self._class_dev = self._workspace = None

    # ---- device side ---------------------------------------------------------------------------------------------------------------
    def _buffers(self, dev):
        import torch
        if self._dev is not dev:
            if self._dev is not None:
                self._download()
            self._dev = dev
            self._state = torch.from_numpy(self._host.view(np.uint8).reshape(self.n_classes, _abi.FILTER_STATE_BYTES).copy()).to(dev.device)
            self._class_dev = torch.from_numpy(np.tile(self.agent_class, self.B)).to(dev.device)
            self._workspace = torch.empty((_abi.filter_workspace_bytes(self.B * self.S, self.D) // 8,), dtype=torch.float64, device=dev.device)

    def _check(self, fn, obs):
        if not hasattr(obs, "shape") or tuple(obs.shape[1:]) != (self.B, self.S, self.D):
            raise ValueError(f"ObsFilter.{fn}: `obs` has shape {tuple(getattr(obs, 'shape', ()))}, expected [T, {self.B}, {self.S}, {self.D}]")

    def update(self, dev, obs, keep=None):
        """fold the kept elements of a time-major device plane ``obs`` f32 ``[T, B, S, D]`` into the statistics (``keep`` u8
        ``[T, B, S]``: who acted; None on a plain env).  One ``dev.filter_update`` call, five launches; no wait"""
        self._check("update", obs)
        self._buffers(dev)
        dev.filter_update(obs, self._state, keep, None if self.n_classes == 1 else self._class_dev, self.n_classes, self._workspace)

    def apply(self, dev, obs, keep=None, out=None):
        """``obs`` normalised with the statistics as they stand: ``(x - mean) / (std + 1e-8)`` in f32, clamped to ``clip``, +0.0 where
        ``keep`` is 0.  ``out``: ``obs`` itself for in place, another 16-byte aligned tensor of its shape, or None (allocated).  One
        launch; no wait"""
        self._check("apply", obs)
        self._buffers(dev)
        return dev.filter_apply(obs, self._state, keep, None if self.n_classes == 1 else self._class_dev, self.n_classes,
                                0.0 if self.clip is None else self.clip, out)

    def _download(self):
        if self._dev is not None:
            self._host = self._state.cpu().numpy().reshape(-1).view(_abi.FILTER_STATE_DTYPE).copy()      # (the one synchronising copy)
        return self._host

    # ---- host side -----------------------------------------------------------------------------------------------------------------
    def state(self):
        """a host copy of the device state: a record array ``[n_classes]`` of ``_abi.FILTER_STATE_DTYPE``, policies in ``policies`` order"""
        return self._download().copy()

    def stats(self):
        """``{policy_id: (count, mean f64 [D], var f64 [D])}`` after one small synchronising copy: ``var = m2 / (count - 1)``, RLlib's
        ``mean * mean`` for a count of 1 and zeros for a policy that has seen nothing"""
        st, D, out = self._download(), self.D, {}
        for c, pid in enumerate(self.policies):
            count = int(st["count"][c])
            mean = st["mean"][c, :D].copy()
            var = np.zeros(D) if count == 0 else (mean * mean if count == 1 else st["m2"][c, :D] / np.float64(count - 1))
            out[pid] = (count, mean, var)
        return out

    def set_stats(self, stats):
        """restore a checkpoint: ``{policy_id: (count, mean [D], var [D])}`` as ``stats()`` returns it, for every policy of the filter;
        ``m2 = var * (count - 1)`` (a count of 1 keeps its mean alone, 0 clears the policy) and ``updates`` becomes 0 or 1"""
        if set(stats) != set(self.policies):
            raise ValueError(f"ObsFilter.set_stats: policies {sorted(map(str, stats))}, the filter has {sorted(map(str, self.policies))}")
        new = np.zeros(self.n_classes, _abi.FILTER_STATE_DTYPE)
        for c, pid in enumerate(self.policies):
            count, mean, var = stats[pid]
            mean, var = np.asarray(mean, np.float64).reshape(-1), np.asarray(var, np.float64).reshape(-1)
            if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 0:
                raise ValueError(f"ObsFilter.set_stats: count = {count!r} of policy {pid!r} must be an int >= 0")
            if mean.shape != (self.D,) or var.shape != (self.D,) or not (np.isfinite(mean).all() and np.isfinite(var).all() and (var >= 0).all()):
                raise ValueError(f"ObsFilter.set_stats: policy {pid!r} needs finite mean and var >= 0 of {self.D} features")
            if count == 0:
                continue
            new["count"][c], new["updates"][c] = int(count), 1
            new["mean"][c, :self.D] = mean
            if count > 1:
                new["m2"][c, :self.D] = var * np.float64(count - 1)
        self._host = new
        if self._dev is not None:
            import torch
            self._state.copy_(torch.from_numpy(new.view(np.uint8).reshape(self.n_classes, _abi.FILTER_STATE_BYTES).copy()))

    def table(self, policy_id=None):
        """``(mean_f, den_f)``, f32 ``[D]`` each, of one policy exactly as ``apply`` forms them from the state (one synchronising copy):
        ``(float)mean`` and ``(float)sqrt(var) + 1e-8f``; (+0.0, 1.0) for a policy that has seen nothing"""
        c = self._class_of(policy_id)
        st, D = self._download(), self.D
        count = int(st["count"][c])
        if count == 0:
            return np.zeros(D, np.float32), np.ones(D, np.float32)
        mean = st["mean"][c, :D].astype(np.float64)
        var = mean * mean if count == 1 else st["m2"][c, :D].astype(np.float64) / np.float64(count - 1)
        return mean.astype(np.float32), np.sqrt(var).astype(np.float32) + np.float32(1e-8)

    def _class_of(self, policy_id):
        if policy_id is None:
            if self.n_classes != 1:
                raise ValueError(f"ObsFilter: the filter has {self.n_classes} policies, name one of {list(self.policies)}")
            return 0
        if policy_id not in self.policies:
            raise ValueError(f"ObsFilter: no policy {policy_id!r}, the filter has {list(self.policies)}")
        return list(self.policies).index(policy_id)

    def fold(self, weights, biases, policy_id=None):
        """``(W0', b0')`` as f32 numpy arrays: the filter of one policy folded into the first layer of an ``MLPPolicy``, so that the
        fused rollout kernels act on RAW observations exactly as the network would on normalised ones, with no kernel change:
        ``pol.update([W0'] + weights[1:], [b0'] + biases[1:])``.  ``weights`` / ``biases``: the policy's lists (layer 0 is read) or
        layer 0's ``[H, D]`` / ``[H]`` arrays themselves.

        From the host snapshot's ``mean_f`` / ``den_f`` (``table()``: exactly what ``apply`` divides by),
        ``W'[j][i] = (float)((double)W[j][i] / (double)den_f[i])`` and ``b'[j] = (float)((double)b[j] - sum)``, where ``sum`` runs over
        i ascending from +0.0 of ``((double)W[j][i] * (double)mean_f[i]) / (double)den_f[i]``.  A clamp cannot be folded into a linear
        layer: a filter with ``clip`` set raises ValueError -- build the filter of a device policy with ``clip=None``."""
        if self.clip is not None:
            raise ValueError(f"ObsFilter.fold: the filter clamps to clip = {self.clip}, which no first layer can express; build it with clip=None")
        W = weights[0] if isinstance(weights, (list, tuple)) else weights
        b = biases[0] if isinstance(biases, (list, tuple)) else biases
        W = np.ascontiguousarray(W.detach().cpu().numpy() if hasattr(W, "detach") else W, np.float32)
        b = np.ascontiguousarray(b.detach().cpu().numpy() if hasattr(b, "detach") else b, np.float32).reshape(-1)
        if W.ndim != 2 or W.shape[1] != self.D or b.shape != (W.shape[0],):
            raise ValueError(f"ObsFilter.fold: layer 0 has weight {W.shape} and bias {b.shape}, expected [H, {self.D}] and [H]")
        mean_f, den_f = self.table(policy_id)
        Wd, m, den = W.astype(np.float64), mean_f.astype(np.float64), den_f.astype(np.float64)
        terms = (Wd * m[None, :]) / den[None, :]
        s = np.zeros(W.shape[0], np.float64)
        for i in range(self.D):                              # (ascending i, from +0.0: the definition's order)
            s = s + terms[:, i]
        return (Wd / den[None, :]).astype(np.float32), (b.astype(np.float64) - s).astype(np.float32)
