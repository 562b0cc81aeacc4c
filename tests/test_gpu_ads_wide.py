"""phx_ads_fused.hip at every workgroup size it launches, against the oracle, bit for bit: the designed markets of
tests/ads_wide_cases.py (tests/test_ads_wide_cpu.py asserts on the oracle that they contain what they claim) and the reference's
own records at N = 130, 300, 1024 (tests/golden/ads_wide.npz).  Rollouts go through test_gpu_fences._rollout: every plane fenced and
poisoned, so a lane >= N of a partial last wave that writes anything is caught.  No tolerance anywhere.

phx_ads_kernel<NT, ...>             NT = 64    128        256          512          1024
  step                 <false, true>  64         65         129, 130     257, 300     513, 1024       (N)
  replayed rollout     <true, true>   64         65, 128    129, 256     257, 512     513, 1023, 1024
  device-drawn rollout <true, false>  64         65, 128    129, 256     257, 512     513, 1023, 1024
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ads_wide_cases as aw
from device_runner import DeviceRunner
from fuzz_cases import cmp
from helpers import f32_bits, f64_bits
from oracle import OracleEnv
from test_ads_wide_cpu import SCATTER_RUNS, wide_records
from test_gpu_fences import _rollout
from test_oracle_vs_goldens import replay_ads

pytestmark = pytest.mark.gpu
ROLLOUT, STEP = "phx_ads_kernel[rollout]", "phx_ads_kernel[step]"
I32_STATE = ("adv.left_tag", "adv.bid_tag", "adv.step_clicks", "adv.step_wins", "adv.user", "adv.total_clicks", "adv.total_requests",
             "adv.total_wins")                                    # what fuzz_cases.ads_case's state() compares
SPARE = {65: 2, 1023: 2}                                          # planes with two rows more than the call fills


def _state(o, d, what=""):
    """adv.left / adv.bid with their kinds, the counters, the connections of this episode and the budgets drawn for it"""
    for f in ("adv.left", "adv.bid") + (("env.sampler",) if o.spec.n_samplers else ()):
        np.testing.assert_array_equal(f64_bits(d.get_f64(f)), f64_bits(o.get_f64(f)), err_msg=f"{what}{f}")
    for f in I32_STATE:
        np.testing.assert_array_equal(d.get_i32(f), o.get_i32(f), err_msg=f"{what}{f}")
    if o.spec.n_conn:
        np.testing.assert_array_equal(d.get_u8("net.conn_on"), o.get_u8("net.conn_on"), err_msg=f"{what}net.conn_on")


def _run(env, T, N, acts=None, exo=None):
    assert env.spec.n_strategic == N
    o, d, frags, ro, first = _rollout(env, T, ROLLOUT, masked=True, spare=SPARE.get(N, 0), acts=acts, exo=exo,
                                      state=I32_STATE + ("env.stage", "env.step"))
    assert d.dev.uses_fused
    _state(o, d)
    return ro


# ---- rollouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", aw.WIDTHS)
@pytest.mark.parametrize("case", ["march first", "march second", "reverse"])
def test_march(case, N):
    """the winner of auction k is advertiser k (reverse: N - 1 - k): the tie-break and the winner's record cross every wave boundary;
    nterm == N on row 2N - 1 ends the episode, the kernel resets and goes on"""
    env, T, acts = aw.reverse_march(N) if case == "reverse" else aw.march(N, case.split()[1])
    ro = _run(env, T, N, acts)
    assert np.flatnonzero((ro["terminated"] != 0).all(axis=(1, 2))).tolist() == [2 * N - 1]


@pytest.mark.parametrize("N", aw.WIDTHS)
def test_second_price_cost_from_the_wave_before(N):
    env, T, acts = aw.second_rising(N)
    _run(env, T, N, acts)


@pytest.mark.parametrize("N", aw.WIDTHS)
@pytest.mark.parametrize("family,strategy", SCATTER_RUNS)
def test_scattered(family, strategy, N):
    """replayed actions (scattered, sampled: the publisher's draws too): winners in every wave, ties across waves, auctions of one
    bidder and of none, resets inside the fragment with N / 3 budgets (sampled) and 2N + 1 connections (dropped) redrawn"""
    env, T, acts, exo = aw.scatter(family, N, strategy)
    _run(env, T, N, acts, exo)


@pytest.mark.parametrize("N", aw.WIDTHS)
@pytest.mark.parametrize("family", list(aw.SCATTER))
def test_device_drawn(family, N):
    """nothing replayed: the instantiation without a load on the step's path"""
    env, T, _, _ = aw.scatter(family, N, "second" if family == "sampled" else "first", drawn=True)
    _run(env, T, N)


# ---- the step kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n130_first", "n130_second_rates", "n300_second", "n1024_first"])
def test_step_kernel_matches_the_reference(name):
    made = []

    def make(spec):
        made.append(DeviceRunner(spec))
        assert made[-1].dev.uses_fused
        return made[-1]
    replay_ads(wide_records()[name], make, tracking=False)
    assert made[0].dev.last_kernel() == STEP, made[0].dev.last_kernel()


@pytest.mark.parametrize("N", [64, 65, 129, 257, 513, 1024])
def test_step_kernel_scattered(N):
    """the scattered market step by step, B = 9 (xcd_block's remainder branch), 24 steps: action_valid masks on half of the steps, the
    publisher's draws replayed on half, every env reset when its episode ends"""
    B, T = 9, 24
    env, _, acts, exo = aw.scatter("scattered", N, "second", B=B, T=T)
    o, d = OracleEnv(env.spec, threads=4), DeviceRunner(env.spec)
    assert d.dev.uses_fused
    o.reset(); d.reset()
    rng = np.random.default_rng(N)
    resets = wins = 0
    for t in range(T):
        valid = (rng.random((B, N)) < 0.9).astype(np.uint8) if t % 4 < 2 else None
        x = exo[t] if t % 2 else None
        o.step(acts[t], valid, x); d.step(acts[t], valid, x)
        assert d.dev.last_kernel() == STEP, d.dev.last_kernel()
        cmp(o, d, (N, t))
        assert (o.err == 0).all()
        _state(o, d, f"step {t}: ")
        wins += int(o.get_i32("adv.step_wins").sum())
        done = ((o.all_truncated != 0) | (o.all_terminated != 0)).astype(np.uint8)
        if done.any():
            (oo, ov), (do, dv) = o.reset(done), d.reset(done)
            m = done.astype(bool)
            assert np.array_equal(dv[m], ov[m]) and np.array_equal(f32_bits(do[m]), f32_bits(oo[m])), (N, t, "reset")
            resets += 1
    assert resets == 3 and wins > B
