#!/usr/bin/env python
"""Build-container only: the reference's digital-ads market at the widths where the fused kernel folds its auction over several
waves (N = 130, 300, 1024 advertisers: workgroups of 256, 512 and 1024 threads), recorded by gen_goldens_ads.run_ads the way
gen_goldens_live.py records its random markets.

    python tests/golden/gen_goldens_ads_wide.py

writes ads_wide.npz (data only, no reference source), keys "<case>.<name>".  Budgets are a permutation of 1 + (i % 97) / 64 as python
floats and four actions in five come from the grid {0, 0.5, 1}: the highest bids tie and the winners spread over the waves.
tests/test_ads_wide_cpu.py replays the records on the oracle, tests/test_gpu_ads_wide.py on the device's step kernel."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
sys.dont_write_bytecode = True

# name -> (N, T, num_steps, seed, strategy, rates)
CASES = {
    "n130_first": (130, 40, 12, 130, "first", None),
    "n130_second_rates": (130, 40, 10, 131, "second", (0.9, 0.8, 0.85)),
    "n300_second": (300, 40, 14, 300, "second", None),
    "n1024_first": (1024, 24, 12, 1024, "first", None),
}


def budgets(N, seed):
    return [1.0 + (int(x) % 97) / 64.0 for x in np.random.RandomState(seed).permutation(N)]


def themes(gga, N):
    return [gga.THEMES[(4 * i) // N] for i in range(N)]


def main():
    import gen_goldens_ads as gga
    out = {}
    for name, (N, T, num_steps, seed, strategy, rates) in CASES.items():
        g = gga.run_ads(None, themes(gga, N), budgets(N, seed), num_steps, T, seed=seed, strategy=strategy, rates=rates, p_uniform=0.2)
        winners = [int(np.flatnonzero(w)[0]) for w in g["step_wins"] if w.any()]
        print(f"{name}: N={N} T={T} winners {min(winners)}..{max(winners)} in waves {sorted({w // 64 for w in winners})} "
              f"terminated={int(g['terminated'].sum())} resets={int(g['reset_before'].sum())}", flush=True)
        out.update({f"{name}.{k}": np.asarray(v) for k, v in g.items()})
    path = os.path.join(HERE, "ads_wide.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes; live_ads.npz:", os.path.getsize(os.path.join(HERE, "live_ads.npz")))


if __name__ == "__main__":
    main()
