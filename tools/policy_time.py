"""On-policy rollouts with the policy evaluated on the device (phx_rollout_io.policy): time per step at the bench shape.
    python tools/policy_time.py [--wide | --explore]      (--wide: only the rows of RLlib-sized networks on phx_sc_rollout_policy_mfma_kernel;
    --explore: SC64, B = 4096, T = 100, deterministic against exploring (a (mean, log_std) head and torch.randn noise) on both kernels)
The wide rows report the f32 work of the network (2 * (3 W0 + W0 W1 + W1) FLOP per (env, shop) and step) against the 157 TF f32 matrix peak."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phantom_amd as ph
from helpers import supply_chain_env


def ev(fn, n):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def pol(widths, seed=0, act="relu"):
    rng = np.random.default_rng(seed)
    dims = [3] + list(widths) + [1]
    ws = [rng.normal(0, 1 / np.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0, .3, (dims[l + 1],)).astype(np.float32) for l in range(len(dims) - 1)]
    return ph.MLPPolicy(ws, bs, activation=act, out_scale=60.0, out_bias=45.0)


WIDE = "--wide" in sys.argv
if "--explore" in sys.argv:
    S, K, B, T = 9, 6, 4096, 100
    for widths, act in (((32,), "relu"), ((64, 64), "relu"), ((256, 256), "tanh")):
        env = supply_chain_env(S, [K] * S, 100, B, seed=1, exogenous="device")
        d = env._device(); env.reset()
        det, sto = pol(widths, act=act), pol(widths, act=act)
        sto = ph.MLPPolicy(sto.weights[:-1] + [np.concatenate([sto.weights[-1], 0.1 * sto.weights[-1]])],
                           sto.biases[:-1] + [np.concatenate([sto.biases[-1], [-0.5]]).astype(np.float32)],
                           activation=act, out_scale=60.0, out_bias=45.0)
        tr, trx = d.alloc_trajectory(T), d.alloc_trajectory(T, explore=True)
        noise = torch.randn((T, B, S), device=d.device, generator=torch.Generator(device=d.device).manual_seed(0))
        us = ev(lambda: d.rollout(T, out=tr, policy=det), 5); k0 = d.last_kernel()
        usx = ev(lambda: d.rollout(T, out=trx, policy=sto, noise=noise), 5); k1 = d.last_kernel()
        print(f"SC64 B=4096    policy 3-{'-'.join(map(str, widths))}-1 {act:4s} deterministic {us / T:8.3f} us/step [{k0}]  exploring "
              f"{usx / T:8.3f} us/step [{k1}]  ratio {usx / us:.3f}", flush=True)
        del env, d, tr, trx
    sys.exit(0)
for name, S, K, B in () if WIDE else (("SC64 B=4096", 9, 6, 4096), ("SC64 B=65536", 9, 6, 65536), ("SC256 B=8192", 51, 4, 8192)):
    env = supply_chain_env(S, [K] * S, 100, B, seed=1, exogenous="device")
    d = env._device(); env.reset()
    T = 100
    tr = d.alloc_trajectory(T)
    for widths in ((8,), (16,), (32,), (64,), (8, 8), (32, 32), (64, 64)):
        p = pol(widths)
        us = ev(lambda: d.rollout(T, out=tr, policy=p), 5)
        by = 22 * S * B * T
        print(f"{name:14s} policy 3-{'-'.join(map(str, widths))}-1  {us / T:8.3f} us/step  {by / us / 1e3 / 8000:.3f} of 8 TB/s  {(1 + S + S * K) * B * T / us * 1e6:.3e} agent-steps/s  [{d.last_kernel()}]", flush=True)
    del env, d, tr

# RLlib-sized networks: tanh, 128 and 256 units (always the MFMA kernel); 3-64-64-1 ReLU on both kernels (variant "policy_mfma")
for name, S, K, B in (("SC64 B=4096", 9, 6, 4096), ("SC64 B=65536", 9, 6, 65536)):
    for widths, act, variant in (((256, 256), "tanh", "auto"), ((128, 128), "tanh", "auto"), ((64, 64), "relu", "auto"), ((64, 64), "relu", "policy_mfma")):
        env = supply_chain_env(S, [K] * S, 100, B, seed=1, exogenous="device", variants={"rollout": variant})
        d = env._device(); env.reset()
        T = 100
        tr = d.alloc_trajectory(T)
        p = pol(widths, act=act)
        us = ev(lambda: d.rollout(T, out=tr, policy=p), 5)
        w = [3] + list(widths) + [1]
        flop = 2 * sum(w[l] * w[l + 1] for l in range(len(w) - 1)) * S * B
        print(f"{name:14s} policy 3-{'-'.join(map(str, widths))}-1 {act:4s} {variant:11s} {us / T:8.3f} us/step  {flop / (us / T) / 1e6:7.2f} TF/s = "
              f"{flop / (us / T) / 1e6 / 157.3:.3f} of the f32 matrix peak  [{d.last_kernel()}]", flush=True)
        del env, d, tr
