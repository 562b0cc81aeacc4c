"""Designed digital-ads markets at the widths where phx_ads_fused.hip changes its workgroup: one env and its replayed inputs per
(case, N), shared by tests/test_ads_wide_cpu.py (the cases contain what they claim, on the oracle) and tests/test_gpu_ads_wide.py
(the device against the oracle).  Every env has tracking off and exogenous="device": the static schedule, hence the fused kernel.

The launcher takes NT = 64, 128, 256, 512, 1024 threads for N <= NT advertisers, one thread per advertiser, and folds the auction
over the waves of 64 through LDS.  WIDTHS are the two sides of every threshold: a last wave of one lane (65, 129, 257, 513), a last
wave missing one lane (1023), the full block.

  march          equal constant budgets, every action 1.25: every bid is the advertiser's whole `left`, all top bids tie, the first
                 in acting order wins, pays everything and terminates -- the winner of auction k is advertiser k, across every wave
                 boundary; all-terminated on row 2N - 1, the rollout resets itself and goes on.  First and second price (the runner-up
                 ties: the same cost).
  reverse        budgets 1 + i / 1024, rising: the winners run N - 1, N - 2, ..., 0, starting in the partial last wave.
  second         second price, budgets rising, every action 1 / 64: no bid reaches `left`, so advertiser N - 1 wins every auction and
                 pays advertiser N - 2's bid (the last lane of the wave before, where N - 1 is a wave's only lane); nobody terminates.
                 (With actions of 1.25 the winner would pay all but 1 / 1024 of its budget and lose the next auction.)
  scattered      budgets a fixed permutation of 1 + (i % 97) / 64, B envs with their own actions from {0, 0.5, 1} and 20 % continuous
                 values, episodes cut by num_steps inside the fragment.  Per (auction k, env b) -- see `_mode`:
                   focus   only one wave bids (wave k, cycling): every wave holds a winner, the one-lane wave included
                   none    every action 0: no bid
                   single  one advertiser bids
                   tie     advertiser 0 (budget 2, action 0.5) and advertiser N - 1 (budget 1, action 1) bid the same f32 1.0 from
                           the first and the last wave: the lower index wins
                   else    everybody draws: ~10 % zeros; the highest budgets tie on the grid across waves
  sampled        scattered, every third advertiser with a UniformFloatSampler budget of its own (clipped and unclipped in turn; f64
                 and python-float arithmetic): ~N / 3 columns redrawn at every reset inside the kernel
  dropped        scattered on connection rates (0.9, 0.8, 0.85), num_steps 6: 2N + 1 connections resampled at every reset
  *-drawn        the envs of scattered / sampled / dropped with neither actions nor draws replayed: the device's own policy
"""
import numpy as np

import phantom_amd as ph

WIDTHS = (64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)
THEMES = ("sport", "travel", "science", "tech")
MARCH_ACTION = 1.25
SCATTER_T, SCATTER_B = 40, 3
RATES = (0.9, 0.8, 0.85)


def nt_of(N):
    """threads of the workgroup ads_launch takes for N advertisers"""
    return next(nt for nt in (64, 128, 256, 512, 1024) if N <= nt)


def ads_env(budgets, num_steps, batch, strategy="first", rates=(1.0, 1.0, 1.0), seed=1, env_offset=0):
    """a DigitalAdsEnv of len(budgets) advertisers (the themes in four equal runs); budgets[i] a float or a sampler"""
    N = len(budgets)
    counts = {th: N // 4 + (1 if k < N % 4 else 0) for k, th in enumerate(THEMES)}
    st = {f"ADV_{i + 1}": ph.AdvertiserAgent.Supertype(budget=b) for i, b in enumerate(budgets)}
    env = ph.DigitalAdsEnv(num_steps=int(num_steps), num_agents_theme={th: n for th, n in counts.items() if n}, agent_supertypes=st,
                           strategy=strategy, connection_rates=rates, batch_size=batch, exogenous="device", seed=seed,
                           env_offset=env_offset)
    env.network.resolver.enable_tracking = False
    return env


# ---- the marches ------------------------------------------------------------------------------------------------------------------------
def march_batch(N):
    return 1 if N >= 513 else 2


def march(N, strategy="first"):
    """(env, T, actions): auction k on row 2k + 1, won by advertiser k; all terminated on row 2N - 1"""
    T, B = 2 * N + 6, march_batch(N)
    return ads_env([1.0] * N, T + 5, B, strategy, seed=5), T, np.full((T, B, N), MARCH_ACTION, np.float32)


def rising_budgets(N):
    return [1.0 + i / 1024.0 for i in range(N)]


def reverse_march(N):
    """(env, T, actions): auction k won by advertiser N - 1 - k"""
    T, B = 2 * N + 6, march_batch(N)
    return ads_env(rising_budgets(N), T + 5, B, "first", seed=6), T, np.full((T, B, N), MARCH_ACTION, np.float32)


SECOND_ACTION = 1.0 / 64.0


def second_rising(N):
    """(env, T, actions): advertiser N - 1 wins every auction at advertiser N - 2's bid"""
    T, B = SCATTER_T, SCATTER_B
    return ads_env(rising_budgets(N), T + 5, B, "second", seed=7), T, np.full((T, B, N), SECOND_ACTION, np.float32)


# ---- the scattered family -----------------------------------------------------------------------------------------------------------
def scattered_budgets(N):
    """a fixed permutation of 1 + (i % 97) / 64 with budget 2 on advertiser 0 and budget 1 on advertiser N - 1 (the tie pair; N = 64
    has no budget 2: one wave, nothing to tie across)"""
    v = [int(x) for x in np.random.default_rng(97).permutation(N)]
    for pos, want in ((0, 64), (N - 1, 0)):
        if want not in v:
            continue
        at = v.index(want)
        v[pos], v[at] = v[at], v[pos]
    return [1.0 + (x % 97) / 64.0 for x in v]


def sampled_budgets(N):
    """scattered_budgets with a sampler of its own on every third advertiser (never the tie pair), clipped and unclipped in turn"""
    out = scattered_budgets(N)
    for k, i in enumerate(range(1, N - 1, 3)):
        out[i] = ph.UniformFloatSampler(0.8, 2.7, 1.0, 2.5) if k % 2 else ph.UniformFloatSampler(1.0, 2.5)
    return out


def auction_rows(T, num_steps):
    """rows of a fragment from reset on which the advertisers act, while no episode ends by all_terminated: the stages alternate from
    the publisher's, and every num_steps rows the reset returns to it"""
    return [t for t in range(T) if (t % num_steps) % 2 == 1]


def _mode(k, b):
    if (k + b) % 3 == 0:
        return "focus"
    return {0: "none", 1: "single", 2: "tie", 3: "tie"}.get((5 * k + 3 * b) % 11, "scatter")


def focus_wave(k, b, N):
    return (k + 7 * (b // 3)) % ((N + 63) // 64)


def scattered_inputs(N, T, B, num_steps, seed):
    """(actions [T, B, N] f32, exo [T, B, 2] u8: the publisher's user 1 | 2 and its click draw)"""
    rng = np.random.default_rng([seed, N])
    grid = rng.choice(np.float32([0.0, 0.5, 1.0]), (T, B, N), p=[0.125, 0.4375, 0.4375])
    acts = np.where(rng.random((T, B, N)) < 0.2, rng.uniform(0.0, 1.0, (T, B, N)).astype(np.float32), grid).astype(np.float32)
    wave = np.arange(N) // 64
    for k, t in enumerate(auction_rows(T, num_steps)):
        for b in range(B):
            m = _mode(k, b)
            if m == "focus":
                on = wave == focus_wave(k, b, N)
                acts[t, b, on & (acts[t, b] == 0)] = 0.5
                acts[t, b, ~on] = 0.0
            elif m != "scatter":
                acts[t, b] = 0.0
                if m == "single":
                    acts[t, b, N // 2] = 0.75
                elif m == "tie":
                    acts[t, b, 0], acts[t, b, N - 1] = 0.5, 1.0
    exo = np.stack([rng.integers(1, 3, (T, B)), rng.integers(0, 2, (T, B))], axis=-1).astype(np.uint8)
    return acts, exo


SCATTER = {                                              # family -> (budgets, num_steps, connection rates, env seed)
    "scattered": (scattered_budgets, 7, (1.0, 1.0, 1.0), 11),
    "sampled": (sampled_budgets, 7, (1.0, 1.0, 1.0), 12),
    "dropped": (scattered_budgets, 6, RATES, 13),
}


def scatter(family, N, strategy="first", B=SCATTER_B, T=SCATTER_T, drawn=False):
    """(env, T, actions, exo); drawn: neither replayed.  `dropped` replays the actions only: users and clicks are the device's"""
    budgets, num_steps, rates, seed = SCATTER[family]
    env = ads_env(budgets(N), num_steps, B, strategy, rates, seed=seed, env_offset=3)
    if drawn:
        return env, T, None, None
    acts, exo = scattered_inputs(N, T, B, num_steps, seed)
    return env, T, acts, (None if family == "dropped" else exo)
