"""CPU: the C oracle against the reference on random cases (tests/golden/ref_fuzz.py and the random digital-ads markets
of tests/golden/gen_goldens_live.py).  What the reference returned for every case is recorded in tests/golden/live_fuzz.npz
and live_ads.npz (gen_goldens_live.py, run where the reference's source tree is present); the cases are rebuilt here on
the phantom_amd side and replayed on the oracle against those records."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)


def _records(fname, prefix):
    with np.load(os.path.join(GOLDEN, fname)) as z:
        keys = [k for k in z.files if k.startswith(prefix + ".")]
        assert keys, f"{fname}: no record {prefix}"
        return {k[len(prefix) + 1:]: z[k] for k in keys}


@pytest.mark.parametrize("first", [0, 700])
def test_oracle_matches_live_reference_on_random_cases(first):
    import ref_fuzz
    for case in range(first, first + 24):
        ref_fuzz.run_case(case, _records("live_fuzz.npz", f"c{case}"))


@pytest.mark.parametrize("first", [0, 500])
def test_oracle_matches_live_reference_ads_market(first):
    """random digital-ads markets run by the reference's own example module (gen_goldens_ads.run_ads):
    budgets of all three numpy kinds, both auction strategies, connectivity < 1, actions above 1."""
    from oracle import OracleEnv
    from test_oracle_vs_goldens import replay_ads
    for case in range(first, first + 12):
        replay_ads(_records("live_ads.npz", f"ads{case}"), lambda spec: OracleEnv(spec))


def test_oracle_matches_live_reference_ads_auction_ties():
    """equal budgets and grid actions: many equal bids, so the winner / second bid are decided by the
    stable sort's arrival order (digital_ads_market.py:498-516)."""
    from oracle import OracleEnv
    from test_oracle_vs_goldens import replay_ads
    for case in range(8):
        g = _records("live_ads.npz", f"tie{case}")
        assert (g["step_wins"].sum() > 0)
        replay_ads(g, lambda spec: OracleEnv(spec))
