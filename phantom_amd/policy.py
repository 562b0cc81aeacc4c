"""A policy evaluated on the device inside the fused rollout (``phx_rollout_io.policy``, ABI 10).

The reference's collection loop calls a policy for every agent and step (utils/rllib/rollout.py:300-363).  ``MLPPolicy`` is the
network the library can evaluate itself (up to RLlib's default model, two hidden layers of 256 tanh units):
``DeviceEnv.rollout(T, policy=pol)`` is ONE launch for T on-policy steps.  Its arithmetic is defined in include/phantom_amd.h (f32, fused multiply-adds term by term in ascending order);
``__call__`` evaluates the same network with torch ops (the same function up to the order of the additions).

A STOCHASTIC policy -- a head of two rows (mean, log_std), RLlib's DiagGaussian for a Box action space, or one row and a state-independent
``log_std`` (RLlib's free_log_std) -- also explores: ``DeviceEnv.rollout(T, policy=pol, noise=...)`` draws z = mean + exp(log_std) noise and
records z, its log-probability and (mean, log_std) (phx_policy_explore; the arithmetic is defined in include/phantom_amd.h)."""
import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _abi

ACTIVATIONS = {"relu": _abi.ACT_RELU, "hard_tanh": _abi.ACT_HARD_TANH, "tanh": _abi.ACT_TANH}


def width_ok(w: int) -> bool:
    """a hidden width the device serves: 1 .. 64, or a multiple of 32 up to 256"""
    return 1 <= w <= _abi.POLICY_MAX_WIDTH or (1 <= w <= _abi.POLICY_WIDE_MAX and w % _abi.POLICY_WIDE_STEP == 0)


class MLPPolicy:
    """``weights`` / ``biases``: torch.nn.Linear's own layouts -- [H0, D], ([H1, H0],) [1, H_last] and [H0], ([H1],) [1]; one or two
    hidden layers of 1 .. 64 units or a multiple of 32 up to 256; ``activation`` "relu", "hard_tanh" (clip to [-1, 1]) or "tanh" (the
    header's PHX_ACT_TANH, within 4e-7 of tanh).  The scalar output y becomes the action
    ``clip(out_scale * y + out_bias, out_lo, out_hi)`` (ShopAgent's action space is Box(0, 100): out_lo >= 0).
    The output layer has one row, or two: (mean, log_std), RLlib's DiagGaussian head; ``log_std`` (a float) gives a one-row head a
    state-independent log-std (RLlib's free_log_std).  Either makes the policy ``stochastic``; deterministic rollouts use the mean row
    (RLlib's deterministic_sample)."""

    def __init__(self, weights: Sequence, biases: Sequence, activation: str = "relu", out_scale: float = 1.0, out_bias: float = 0.0,
                 out_lo: float = 0.0, out_hi: float = 100.0, log_std: Optional[float] = None):
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(ACTIVATIONS)}")
        self.weights = [np.ascontiguousarray(_np(w), np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(_np(b), np.float32).reshape(-1) for b in biases]
        n = len(self.weights)
        if n not in (2, 3) or len(self.biases) != n:
            raise ValueError("MLPPolicy: one or two hidden layers (2 or 3 weight matrices and as many biases)")
        for l in range(n):
            w, b = self.weights[l], self.biases[l]
            if w.ndim != 2 or b.shape != (w.shape[0],) or (l > 0 and w.shape[1] != self.weights[l - 1].shape[0]):
                raise ValueError(f"MLPPolicy: layer {l} has weight {w.shape} and bias {b.shape}")
            if l < n - 1 and not width_ok(w.shape[0]):
                raise ValueError(f"MLPPolicy: hidden width {w.shape[0]}: 1 .. {_abi.POLICY_MAX_WIDTH}, or a multiple of "
                                 f"{_abi.POLICY_WIDE_STEP} up to {_abi.POLICY_WIDE_MAX}")
            if not (np.isfinite(w).all() and np.isfinite(b).all()):
                raise ValueError("MLPPolicy: weights must be finite")
        if self.weights[-1].shape[0] not in (1, 2):
            raise ValueError("MLPPolicy: the output layer has one unit (the agent's scalar action) or two (mean, log_std)")
        if log_std is not None and (self.weights[-1].shape[0] == 2 or not np.isfinite(np.float32(log_std))):
            raise ValueError("MLPPolicy: `log_std` is a finite float for a one-row head (a two-row head has its own log-std row)")
        self.log_std = None if log_std is None else float(np.float32(log_std))
        if not 0.0 <= out_lo <= out_hi:
            raise ValueError("MLPPolicy: 0 <= out_lo <= out_hi")
        self.activation = activation
        self.out_scale, self.out_bias, self.out_lo, self.out_hi = float(out_scale), float(out_bias), float(out_lo), float(out_hi)
        self._dev = {}
        self._free = {}                  # device -> f32 [1]: the free log-std (b_log_std of a one-row head)

    @property
    def obs_dim(self) -> int:
        return int(self.weights[0].shape[1])

    @property
    def stochastic(self) -> bool:
        """a log-std to explore with: a two-row head or a ``log_std``"""
        return self.weights[-1].shape[0] == 2 or self.log_std is not None

    @classmethod
    def from_torch(cls, module, **kw) -> "MLPPolicy":
        """from a torch.nn.Sequential: Linear, activation, Linear[, activation, Linear] in that order -- ReLU, Hardtanh(-1, 1) or Tanh,
        the same one between every pair of Linears.  Any other layer, mixed activations, two Linears in a row or a Hardtanh with other
        bounds raise ValueError.  The last Linear has one output, or two: RLlib's action head for a Box action space, (mean, log_std),
        which makes the policy stochastic (``log_std=`` in ``kw`` gives a one-output head RLlib's free_log_std instead)."""
        import torch
        kinds = {torch.nn.ReLU: "relu", torch.nn.Tanh: "tanh", torch.nn.Hardtanh: "hard_tanh"}
        layers = list(module.children()) if len(list(module.children())) else [module]
        lin, acts = [], []
        for i, m in enumerate(layers):
            want_linear = i % 2 == 0
            if want_linear:
                if type(m) is not torch.nn.Linear:
                    raise ValueError(f"MLPPolicy.from_torch: layer {i} is {type(m).__name__}, a Linear is expected there")
                if m.bias is None:
                    raise ValueError(f"MLPPolicy.from_torch: layer {i} has no bias")
                lin.append(m)
                continue
            kind = kinds.get(type(m))
            if kind is None:
                raise ValueError(f"MLPPolicy.from_torch: layer {i} is {type(m).__name__}: ReLU, Hardtanh(-1, 1) or Tanh expected "
                                 "between Linears")
            if kind == "hard_tanh" and (float(m.min_val) != -1.0 or float(m.max_val) != 1.0):
                raise ValueError(f"MLPPolicy.from_torch: layer {i} is Hardtanh({m.min_val}, {m.max_val}); only Hardtanh(-1, 1)")
            acts.append(kind)
        if not lin or len(layers) % 2 == 0:
            raise ValueError("MLPPolicy.from_torch: the module must end with a Linear")
        if len(set(acts)) > 1:
            raise ValueError(f"MLPPolicy.from_torch: mixed activations {acts}; one kind between every pair of Linears")
        if not acts:
            raise ValueError("MLPPolicy.from_torch: at least one hidden layer (Linear, activation, Linear)")
        return cls([m.weight.detach() for m in lin], [m.bias.detach() for m in lin], activation=acts[0], **kw)

    def update(self, weights: Sequence, biases: Sequence, log_std: Optional[float] = None) -> None:
        """new parameter values of the same shapes (a learner's update; a two-row head's log-std row with the rest, ``log_std`` for a
        policy built with one): the device copies are refreshed in place, cached argument blocks stay valid"""
        import torch
        if log_std is not None and self.log_std is None:
            raise ValueError("MLPPolicy.update: `log_std` is for a policy built with one")
        new = []
        for l, (w, b) in enumerate(zip(weights, biases)):
            w, b = np.ascontiguousarray(_np(w), np.float32), np.ascontiguousarray(_np(b), np.float32).reshape(-1)
            if w.shape != self.weights[l].shape or b.shape != self.biases[l].shape:
                raise ValueError("MLPPolicy.update: shapes differ from the policy's")
            new.append((w, b))
        for l, (w, b) in enumerate(new):
            self.weights[l], self.biases[l] = w, b
            for dev, (ws, bs, _) in self._dev.items():
                ws[l].copy_(torch.from_numpy(w)); bs[l].copy_(torch.from_numpy(b))
        if log_std is not None:
            self.log_std = float(np.float32(log_std))
            for ls in self._free.values():
                ls.fill_(self.log_std)

    def on(self, device):
        """(device weight tensors, device bias tensors, the phx_policy_mlp argument) for ``device``"""
        import torch
        key = str(device)
        if key not in self._dev:
            ws = [torch.from_numpy(w).to(device).contiguous() for w in self.weights]
            bs = [torch.from_numpy(b).to(device).contiguous() for b in self.biases]
            self._dev[key] = (ws, bs, self._c_struct([w.data_ptr() for w in ws], [b.data_ptr() for b in bs]))
        return self._dev[key]

    def _c_struct(self, wptrs, bptrs) -> "_abi.PhxPolicyMLP":
        p = _abi.PhxPolicyMLP()
        n = len(self.weights)
        p.n_hidden = n - 1
        p.width[0] = self.weights[0].shape[0]
        p.width[1] = self.weights[1].shape[0] if n == 3 else 0
        p.activation = ACTIVATIONS[self.activation]
        p.out_scale, p.out_bias, p.out_lo, p.out_hi = self.out_scale, self.out_bias, self.out_lo, self.out_hi
        for l in range(3):
            p.w[l] = wptrs[l] if l < n else None
            p.b[l] = bptrs[l] if l < n else None
        return p

    def explore_struct(self, device, noise, raw_action, logp, dist_inputs) -> "_abi.PhxPolicyExplore":
        """the phx_policy_explore argument for tensors on ``device``: ``noise`` the standard-normal draws, the three output planes; the
        log-std row and bias are the device copies of the head's second row (or the free log-std).  ValueError for a policy without a
        log-std."""
        import torch
        if not self.stochastic:
            raise ValueError("MLPPolicy: `noise` needs a stochastic policy (a (mean, log_std) head or log_std=)")
        ws, bs, _ = self.on(device)
        x = _abi.PhxPolicyExplore()
        x.noise, x.raw_action, x.logp, x.dist_inputs = (t.data_ptr() for t in (noise, raw_action, logp, dist_inputs))
        if self.log_std is None:
            x.w_log_std = ws[-1][1].data_ptr()
            x.b_log_std = bs[-1][1:].data_ptr()
        else:
            key = str(device)
            if key not in self._free:
                self._free[key] = torch.full((1,), self.log_std, dtype=torch.float32, device=device)
            x.w_log_std = None
            x.b_log_std = self._free[key].data_ptr()
        return x

    def distribution(self, obs):
        """(mean, log_std) of the action distribution on a torch tensor [..., D] with torch ops -- RLlib's action_dist_inputs, unclamped
        (the device clamps the log-std to [-20, 20] before it draws)"""
        import torch
        if not self.stochastic:
            raise ValueError("MLPPolicy.distribution: a deterministic policy (one-row head, no log_std)")
        out = self._head(obs)
        if self.log_std is None:
            return out[..., 0], out[..., 1]
        return out[..., 0], torch.full_like(out[..., 0], self.log_std)

    def host_struct(self) -> "_abi.PhxPolicyMLP":
        """the same argument over the HOST copies of the weights (the CPU restatement's tests)"""
        return self._c_struct([w.ctypes.data for w in self.weights], [b.ctypes.data for b in self.biases])

    def __call__(self, obs):
        """the network on a torch tensor [..., D] with torch ops (same function up to the order of the additions -- and, for tanh,
        torch.tanh against the header's approximation, within 4e-7); a two-row head's mean row"""
        import torch
        y = self._head(obs)[..., 0]
        return torch.clamp(y * self.out_scale + self.out_bias, self.out_lo, self.out_hi)

    def _head(self, obs):
        """the output layer's rows [..., 1 or 2] on a torch tensor [..., D]"""
        import torch
        ws, bs, _ = self.on(obs.device)
        h = obs
        for l in range(len(ws) - 1):
            h = torch.nn.functional.linear(h, ws[l], bs[l])
            if self.activation == "hard_tanh":
                h = torch.clamp(h, -1.0, 1.0)
            elif self.activation == "tanh":
                h = torch.tanh(h)
            else:
                h = torch.relu(h)
        return torch.nn.functional.linear(h, ws[-1], bs[-1])


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
