"""The edge-value networks of tests/policy_edges.py on both device-policy kernels: the tanh thresholds, the ReLU / hard-tanh boundaries
(v_med3_f32), signed zeros, subnormal MFMA and VALU operands, +inf pre-activations (NaN is out of scope: see policy_edges.py) and sums
whose value depends on the order of their roundings.  Every network: the device's on-policy rows, last_obs and state == the oracle's, and
its actions == tests/policy_ref.py's, bit for bit; the family tells the definition from every perturbation it targets."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import policy_edges as pe
import policy_ref as pr
from device_runner import DeviceRunner
from helpers import f32_bits, supply_chain_env
from oracle import OracleEnv

pytestmark = pytest.mark.gpu
STATE = ("shop.stock", "shop.sales", "shop.missed_sales", "shop.delivered_stock", "env.step", "env.tick")


@pytest.mark.parametrize("cid,act,widths,j,kern,fam", pe.cases(), ids=[c[0] for c in pe.cases()])
def test_edge_family_on_the_device(cid, act, widths, j, kern, fam):
    nets, targets = pe.families(act, widths, j)[fam]
    env = supply_chain_env(9, [6] * 9, 7, 4, seed=3)
    o, d = OracleEnv(env.spec, threads=4), DeviceRunner(env.spec)
    x0, _ = o.reset(); d.reset()
    hit = {t: False for t in targets}
    for n, pol in enumerate(nets):
        rd, ro = d.rollout(16, policy=pol), o.rollout(16, policy=pol)
        assert d.dev.last_kernel() == kern, d.dev.last_kernel()
        assert (d.err == 0).all()
        for k in ("obs", "actions", "rewards", "last_obs"):
            np.testing.assert_array_equal(f32_bits(rd[k]), f32_bits(ro[k]), err_msg=f"{cid} net {n}: {k}")
        np.testing.assert_array_equal(rd["truncated"], ro["truncated"], err_msg=f"{cid} net {n}")
        for f in STATE:
            np.testing.assert_array_equal(d.get_i32(f), o.get_i32(f), err_msg=f"{cid} net {n}: {f}")
        x = pe.prev_obs(x0, rd)
        np.testing.assert_array_equal(f32_bits(rd["actions"].reshape(-1)), f32_bits(pr.action(pol, x)), err_msg=f"{cid} net {n}")
        for t in targets:
            hit[t] = hit[t] or pe.sensitive(pol, x, t)
        x0 = rd["last_obs"]
    assert all(hit.values()), f"{cid}: the perturbations {[t for t, h in hit.items() if not h]} change no action"
