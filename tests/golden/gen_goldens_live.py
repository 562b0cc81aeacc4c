#!/usr/bin/env python
"""Build-container only: record the reference's side of the random differential cases that
tests/test_oracle_vs_live_reference.py replays against the CPU oracle.

    python tests/golden/gen_goldens_live.py

writes (data only, no reference source):
  live_fuzz.npz   traces of ref_fuzz.py cases 0-23 and 700-723 (supply chains, FSM tables, Stackelberg markets), every
                  case checked against the oracle while it is recorded; keys "c<case>.<name>"
  live_ads.npz    gen_goldens_ads.run_ads results of the random digital-ads markets (seeds 9000 + case, cases 0-11 and
                  500-511) and of the auction-tie cases (seeds 19000 + case, cases 0-7); keys "<group><case>.<name>"
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
sys.dont_write_bytecode = True

FUZZ_CASES = list(range(0, 24)) + list(range(700, 724))
ADS_CASES = list(range(0, 12)) + list(range(500, 512))
TIE_CASES = list(range(8))


def ads_case(gga, case):
    """random digital-ads markets: budgets of all three numpy kinds, both auction strategies, connectivity < 1, actions above 1"""
    rng = np.random.RandomState(9000 + case)
    n = int(rng.randint(1, 9))
    themes = sorted(rng.choice(gga.THEMES, n).tolist(), key=gga.THEMES.index)
    budgets = []
    for _ in range(n):
        r = rng.rand()
        if r < 0.4:
            budgets.append(float(rng.choice([0.5, 0.75, 1.0, 1.3, 2.0, 3.1])))
        elif r < 0.7:
            lo = float(rng.uniform(0.3, 1.0))
            budgets.append(("clipped", lo, lo + 1.0, lo + 0.1, lo + 0.9))
        else:
            budgets.append(("uniform", 0.4, float(rng.uniform(0.5, 2.5))))
    rates = None if rng.rand() < 0.5 else tuple(float(x) for x in rng.choice([1.0, 0.9, 0.7, 0.5], 3))
    return gga.run_ads(None, themes, budgets, int(rng.randint(2, 16)), int(rng.randint(8, 60)), seed=case,
                       strategy=("second" if rng.rand() < 0.5 else "first"), rates=rates,
                       act_hi=float(rng.choice([1.0, 1.2, 2.0])))


def tie_case(gga, case):
    """equal budgets and grid actions: many equal bids, decided by the stable sort's arrival order"""
    rng = np.random.RandomState(19000 + case)
    k = int(rng.randint(2, 21))
    themes = sorted(rng.choice(gga.THEMES, k).tolist(), key=gga.THEMES.index)
    budgets = [[1.0] * k, [float(rng.choice([1.0, 2.0])) for _ in range(k)], [("clipped", 0.5, 1.5, 1.0, 1.0)] * k][case % 3]
    return gga.run_ads(None, themes, budgets, int(rng.randint(4, 30)), int(rng.randint(20, 90)), seed=case,
                       strategy=("second" if case % 2 else "first"), p_uniform=0.3)


def main():
    import gen_goldens_ads as gga
    import ref_fuzz
    out = {}
    for case in FUZZ_CASES:
        desc, trace = ref_fuzz.run_case(case)
        out.update({f"c{case}.{k}": v for k, v in trace.items()})
        print("fuzz", case, desc, flush=True)
    np.savez_compressed(os.path.join(HERE, "live_fuzz.npz"), **out)
    out = {}
    for group, fn, cases in (("ads", ads_case, ADS_CASES), ("tie", tie_case, TIE_CASES)):
        for case in cases:
            out.update({f"{group}{case}.{k}": np.asarray(v) for k, v in fn(gga, case).items()})
    np.savez_compressed(os.path.join(HERE, "live_ads.npz"), **out)


if __name__ == "__main__":
    main()
