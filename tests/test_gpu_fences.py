"""Every kernel that writes caller-owned device memory, run into FENCED, POISONED buffers (tests/fenced.py): no byte outside a plane
is written, no element inside is left unwritten (where the ABI specifies it), the planes equal the oracle's bit for bit, the replayed
inputs are untouched.  Shapes sit on the kernels' edges: plane byte counts that are no multiple of 16 wherever the kernel takes such a
shape, no multiple of 64 where it demands pairs in multiples of 16 (B S = 192 of the FSM store-wave case is one: its plan needs it).

kernel (phx_last_kernel) -> case
  phx_sc_rollout_sw_kernel                       test_store_wave_rollout, test_store_wave_fragment_list, test_spare_rows_stay_untouched[sw ...]
  phx_sc_rollout_sw_kernel[replay]               test_store_wave_replay
  phx_sc_rollout_sw_kernel[fsm]                  test_store_wave_fsm (one fragment, a list)
  phx_sc_rollout_fast_kernel[pairs]              test_time_parallel_rollout[...-36-...] (TP_EDGE), [4-4-64-50-21-32-...], test_time_parallel_sparse_flag_planes[joined]
  phx_sc_rollout_fast_kernel[whole_envs]         test_time_parallel_rollout[...-0-...] (TP_EDGE), [4-4-64-50-21-whole_envs-...], test_time_parallel_sparse_flag_planes[odd tail ...]
  phx_zero_fill_kernel[flag planes]              test_time_parallel_sparse_flag_planes (the fill starts at T B S >= 2^23: the module's only large cases)
  phx_sc_rollout_kernel                          test_general_rollout, test_time_parallel_rollout[9-6-7-5-11-...] (see there)
  phx_sc_rollout_kernel[if an action ...]        test_action_that_rounds_below_zero
  phx_sc_rollout_fsm_lean_kernel                 test_fsm_rollout_kernels[lean]
  phx_sc_rollout_fsmfast_kernel[pairs]           test_fsm_rollout_kernels[fsmfast pairs]
  phx_sc_rollout_fsmfast_kernel[whole_envs]      test_fsm_rollout_kernels[fsmfast whole_envs]
  phx_sc_rollout_fsm_kernel                      test_fsm_rollout_kernels[general]
  phx_sc_rollout_fsm_kernel[rules]               test_fsm_rule_rollout, test_spare_rows_stay_untouched[rules]
  phx_sc_rollout_policy_kernel                   test_policy_rollout[8-relu], [24x16-hard_tanh]
  phx_sc_rollout_policy_mfma_kernel              test_policy_rollout[96-relu], [32x32-relu policy_mfma]
  phx_sc_rollout_policy_explore_kernel           test_policy_rollout[... explore]
  phx_sc_rollout_policy_mfma_explore_kernel      test_policy_rollout[... explore]
  phx_stk_rollout_kernel                         test_market_rollout
  phx_ads_kernel[rollout]                        test_ads_rollout
  phx_generic_step_kernel[T-step loop]           test_engine_rollout[dynamic], [dynamic tracked]
  phx_sched_step_kernel[T-step loop]             test_engine_rollout[compiled], [compiled tracked]
  phx_sc_step_kernel, phx_sc_step_wide_kernel    test_step_outputs[sc ...], [wide ...]
  phx_stk_step_fast_kernel, phx_stk_step_kernel  test_step_outputs[market packed], [market degree 9]
  phx_ads_kernel[step]                           test_step_outputs[ads]
  phx_generic_step_kernel, phx_sched_step_kernel test_step_outputs[dynamic ...], [compiled ...]
  phx_step_begin + phx_step_end                  test_step_begin_leaves_the_outputs_alone_and_step_end_writes_them
  phx_reset / phx_mt_draw / phx_pack_flags / phx_unpack_flags / phx_get_state: the tests of those names at the end
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phantom_amd as ph
from phantom_amd import _abi
from device_runner import DeviceRunner
from fenced import assert_fences, assert_poison, assert_written, fenced, fenced_trajectory, repoison
from helpers import ads_env_from_golden, f32_bits, f64_bits, golden, market_env, supply_chain_env
from oracle import LOG_DTYPE, OracleEnv

pytestmark = pytest.mark.gpu
SC_STATE = ("shop.stock", "shop.sales", "shop.missed_sales", "shop.delivered_stock", "env.step", "env.tick")
SW = "phx_sc_rollout_sw_kernel"
FSM_LOOP = "phx_sc_rollout_fsm_lean_kernel[if off-chain]"
BELOW_ZERO = "phx_sc_rollout_kernel[if an action rounds below zero]"


def _np(x):
    return None if x is None else x.cpu().numpy()


def _dev_copy(d, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(d.dev.device)


def _same_bytes(a, b, what):
    assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), f"the call changed its input `{what}`"


def _exempt(tr, ro, lo, hi, masked):
    """what assert_written skips in rows [lo, hi) of the oracle's rollout: observations where obs_valid == 0 and rewards where
    reward_valid != 1 (``masked``), message records past the step's count"""
    m = {}
    if masked:
        m["observations"], m["rewards"] = ro["obs_valid"][lo:hi] == 0, ro["reward_valid"][lo:hi] != 1
    if tr.msg_count is not None:
        m["msg_log"] = np.arange(ro["msg_log"].shape[2])[None, None, :] >= ro["msg_count"][lo:hi][..., None]
    return m


def _compare(tr, ro, lo, hi, exempt, what):
    """rows [0, hi - lo) of a fragment against rows [lo, hi) of the oracle's rollout, bit for bit, outside ``exempt``"""
    n = hi - lo
    row = lambda x: _np(x)[:n]
    if tr.obs_valid is not None:
        np.testing.assert_array_equal(row(tr.obs_valid), ro["obs_valid"][lo:hi], err_msg=f"{what}obs_valid")
        np.testing.assert_array_equal(row(tr.reward_valid), ro["reward_valid"][lo:hi], err_msg=f"{what}reward_valid")
    everything = np.ones(ro["truncated"][lo:hi].shape, bool)
    mo, mr = ~exempt.get("observations", ~everything), ~exempt.get("rewards", ~everything)
    np.testing.assert_array_equal(f32_bits(row(tr.observations))[mo], f32_bits(ro["obs"][lo:hi])[mo], err_msg=f"{what}observations")
    np.testing.assert_array_equal(f32_bits(row(tr.rewards))[mr], f32_bits(ro["rewards"][lo:hi])[mr], err_msg=f"{what}rewards")
    np.testing.assert_array_equal(f32_bits(row(tr.actions)), f32_bits(ro["actions"][lo:hi]), err_msg=f"{what}actions")
    np.testing.assert_array_equal(row(tr.truncations), ro["truncated"][lo:hi], err_msg=f"{what}truncations")
    if tr.terminations is not None:
        np.testing.assert_array_equal(row(tr.terminations), ro["terminated"][lo:hi], err_msg=f"{what}terminations")
    if tr.msg_count is not None:
        np.testing.assert_array_equal(row(tr.msg_count), ro["msg_count"][lo:hi], err_msg=f"{what}msg_count")
        live = ~exempt["msg_log"]
        got = np.ascontiguousarray(row(tr.msg_log)).view(LOG_DTYPE)[..., 0]
        assert (got[live] == ro["msg_log"][lo:hi][live]).all(), f"{what}msg_log"


def _rollout(env, T, kernel, *, k=1, spare=0, acts=None, exo=None, masked=False, state=SC_STATE, threads=4, policy=None, noise=None,
             record=False, after_reset=None, hints=None, **traj_kw):
    """ONE phx_rollout of ``k`` fragments of ``T`` rows into fenced planes of ``T + spare`` rows each, from reset: the kernel's name, the
    fences, the poison (rows >= T and the earlier fragments' last_obs keep it), the oracle's planes and state, the inputs' bytes.
    Returns (oracle env, DeviceRunner, fragments, the oracle's rows, the reset observation)."""
    o, d = OracleEnv(env.spec, threads=threads), DeviceRunner(env.spec)
    o.reset(); d.reset()
    if after_reset is not None:
        after_reset(o, d)
    dev = d.dev
    first = _np(dev.obs).copy()
    frags = [fenced_trajectory(dev, T + spare, explore=noise is not None, record_messages=record, **traj_kw) for _ in range(k)]
    inputs = {"actions": _dev_copy(d, acts, np.float32), "exo": _dev_copy(d, exo, np.uint8), "noise": _dev_copy(d, noise, np.float32)}
    before = {n: x.clone() for n, x in inputs.items() if x is not None}
    hints = hints or {}
    if k == 1:
        kw = dict(policy=policy, noise=inputs["noise"]) if policy is not None else {}
        dev.rollout(T, inputs["actions"], inputs["exo"], out=frags[0][0], **hints, **kw)
    else:
        got = dev.rollout_fragments(T, [f[0] for f in frags], inputs["actions"], inputs["exo"], **hints)
        assert all(g.last_obs is None for g in got[:-1])
    torch.cuda.synchronize()
    assert dev.last_kernel() == kernel, dev.last_kernel()
    if noise is not None:                    # the oracle has no noise input: it replays the device's action plane (as test_gpu_policy_explore does)
        ro = o.rollout(T, _np(frags[0][0].actions)[:T], exo)
    else:
        ro = o.rollout(k * T, acts, exo, record_messages=record, policy=policy)
    for i, (tr, wholes, check) in enumerate(frags):
        what = f"fragment {i}: " if k > 1 else ""
        exempt = _exempt(tr, ro, i * T, (i + 1) * T, masked)
        check(rows=T, masks=exempt, last_obs=i == k - 1, what=what)
        _compare(tr, ro, i * T, (i + 1) * T, exempt, what)
    np.testing.assert_array_equal(f32_bits(_np(frags[-1][0].last_obs)), f32_bits(ro["last_obs"]), err_msg="last_obs")
    for f in state:
        np.testing.assert_array_equal(d.get_i32(f), o.get_i32(f), err_msg=f)
    assert (_np(dev.err) == 0).all()
    for n, x in before.items():
        _same_bytes(inputs[n], x, n)
    return o, d, frags, ro, first


# ---- the store-wave kernel ------------------------------------------------------------------------------------------------------------
# (3, 2, 48): 144 pairs; T = 41: u8 planes of 5904 bytes = 16 mod 64.  (9, 6, 64) T = 57: 32 832 bytes = 0 mod 64 but 57 rows = 3 chunks + 9.
SW_SHAPES = [(3, 2, 48, 22, 41, 48), (9, 6, 64, 23, 57, 0), (51, 4, 128, 20, 44, 0)]


def _sw_env(S, K, B, ns, block=0, **kw):
    return supply_chain_env(S, [K] * S, ns, B, seed=11 + S, env_offset=5, variants={"rollout": "store_waves", **({"block": block} if block else {})}, **kw)


@pytest.mark.parametrize("S,K,B,ns,T,block", SW_SHAPES)
@pytest.mark.parametrize("terminations", [True, False], ids=["", "no terminations plane"])
def test_store_wave_rollout(S, K, B, ns, T, block, terminations):
    _rollout(_sw_env(S, K, B, ns, block), T, SW, terminations=terminations)


@pytest.mark.parametrize("what,vouch", [("actions", False), ("actions", True), ("exo", True), ("both", True)])
def test_store_wave_replay(what, vouch):
    """replayed actions (above 100, 1e9, +inf, halves, in (-0.5, 0): none rounds below zero) and / or order sizes; the caller vouches for
    the order sizes always (the kernel takes no others) and for the actions in the `vouch` cases (no pre-scan launch then)"""
    S, K, B, ns, T, block = SW_SHAPES[0]
    rng = np.random.default_rng(41)
    acts = exo = None
    if what in ("actions", "both"):
        acts = rng.uniform(0, 130, (T, B, S)).astype(np.float32)
        for p, v in ((0.1, 0.5), (0.1, 2.5), (0.05, -0.4), (0.02, 1e9), (0.01, np.inf)):
            acts[rng.random((T, B, S)) < p] = v
    if what in ("exo", "both"):
        exo = rng.integers(0, 5, (T, B, S * K)).astype(np.uint8)
    kernel = SW + "[replay]" + ("+" + BELOW_ZERO if acts is not None and not vouch else "")
    _rollout(_sw_env(S, K, B, ns, block), T, kernel, acts=acts, exo=exo,
             hints=dict(actions_in_domain=vouch and acts is not None, exo_in_domain=exo is not None))


@pytest.mark.parametrize("S,K,B,ns,Tf,k,block", [(3, 2, 48, 22, 23, 3, 48), (9, 6, 64, 21, 5, 8, 0)])
def test_store_wave_fragment_list(S, K, B, ns, Tf, k, block):
    """k fragments from one launch, every fragment's planes fenced on their own (the store waves switch base pointers at the fragments'
    first rows); only the last fragment's last_obs is written"""
    _rollout(_sw_env(S, K, B, ns, block), Tf, SW, k=k)


@pytest.mark.parametrize("k,T", [(1, 41), (3, 17)], ids=["one fragment", "fragment list"])
def test_store_wave_fsm(k, T):
    """the FSM instantiation at the smallest shape of tests/test_gpu_fsm_sw.py (3 shops x 64 envs, 48-pair workgroups): validity planes as
    closed forms of the step counters; every element of every plane is the oracle's (no mask: the kernel writes silent rows too)"""
    env = supply_chain_env(3, [2] * 3, 16, 64, fsm=True, seed=10, env_offset=13, variants={"rollout": "store_waves", "block": 48})
    _rollout(env, T, SW + "[fsm]+" + FSM_LOOP, k=k, state=SC_STATE + ("env.stage", "env.prev_stage"))


# ---- the time-parallel kernel and the flag planes' zero fill -------------------------------------------------------------------------------
TP_PAIRS, TP_WHOLE = (4, 4, 64, 50, 21, 32, "phx_sc_rollout_fast_kernel[pairs]"), (4, 4, 64, 50, 21, "whole_envs", "phx_sc_rollout_fast_kernel[whole_envs]")
TP_ODD, TP_ODD_WHOLE = (9, 6, 7, 5, 11, 0, "phx_sc_rollout_kernel"), (9, 6, 7, 5, 11, "whole_envs", "phx_sc_rollout_kernel")
# the smallest shapes the kernel takes whose planes end off a 16-byte boundary: 36 pairs per row, T = 21: u8 planes of 756 bytes = 4 mod 16,
# one workgroup of 36 pairs (whole envs: 12 envs of 3 shops / 4 envs of 9 shops) -- the DENSE flag stores (no zero fill below 2^23 bytes)
TP_EDGE = [(3, 2, 12, 50, 21, 0, "phx_sc_rollout_fast_kernel[whole_envs]"), (3, 2, 12, 50, 21, 36, "phx_sc_rollout_fast_kernel[pairs]"),
           (9, 6, 4, 50, 21, 0, "phx_sc_rollout_fast_kernel[whole_envs]"), (9, 6, 4, 50, 21, 36, "phx_sc_rollout_fast_kernel[pairs]")]


@pytest.mark.parametrize("S,K,B,ns,T,block,kernel,flags",
                         [c + (f,) for c in (TP_PAIRS, TP_WHOLE) for f in ("separate", "joined", "no terminations plane")] +
                         [c + (f,) for c in (TP_ODD, TP_ODD_WHOLE) for f in ("separate", "no terminations plane")] +
                         [c + (f,) for c in TP_EDGE for f in ("separate", "no terminations plane", "separate, spare rows", "no terminations plane, spare rows")])
def test_time_parallel_rollout(S, K, B, ns, T, block, kernel, flags):
    """variants rollout=time_parallel.  (4, 4, 64, 50) T = 21: T B S = 5376 = 21 x 256, the size at which alloc_trajectory joins the flag
    planes.  (9, 6, 7, 5) T = 11: T B S = 693, odd -- the plan of the time-parallel kernel refuses the shape (63 pairs are no multiple of 4,
    and episodes of 5 steps are shorter than its 20-row chunk), so phx_rollout hands it to phx_sc_rollout_kernel whatever block is asked for;
    that kernel cannot leave the `terminations` plane out: without it the call is refused before any launch and writes nothing.
    The kernel's own edge: (3, 2, 12, 50) and (9, 6, 4, 50), T = 21 (TP_EDGE), also into planes with three spare rows.
    (No joined block at 693 or 756 bytes per plane: its second half would start off a 16-byte boundary, which phx_rollout refuses; alloc_trajectory
    joins the planes at multiples of 256 only.)"""
    env = supply_chain_env(S, [K] * S, ns, B, seed=3 + S, env_offset=2, variants={"rollout": "time_parallel", **({"block": block} if block else {})})
    kw = dict(joined_flags=True) if flags == "joined" else dict(terminations=flags.startswith("separate"), spare=3 if flags.endswith("spare rows") else 0)
    if kernel == "phx_sc_rollout_kernel" and flags == "no terminations plane":
        from phantom_amd.device import DeviceError
        d = DeviceRunner(env.spec); d.reset()
        tr, wholes, check = fenced_trajectory(d.dev, T, terminations=False)
        with pytest.raises(DeviceError, match="`terminated` is required"):
            d.dev.rollout(T, out=tr)
        torch.cuda.synchronize()
        for name, (w, n0) in wholes.items():                     # refused before any launch: nothing was written
            assert_poison(w, name)
        return
    _rollout(env, T, kernel, **kw)


@pytest.mark.parametrize("S,K,B,ns,T,block,flags,kernel", [
    (3, 2, 12, 50, 233017, "whole_envs", "separate", "phx_sc_rollout_fast_kernel[whole_envs]"),
    (3, 2, 12, 50, 233017, "whole_envs", "no terminations plane", "phx_sc_rollout_fast_kernel[whole_envs]"),
    (4, 4, 64, 50, 32768, 32, "joined", "phx_sc_rollout_fast_kernel[pairs]")], ids=["odd tail", "odd tail, no terminations plane", "joined"])
def test_time_parallel_sparse_flag_planes(S, K, B, ns, T, block, flags, kernel):
    """phx_zero_fill_kernel[flag planes] runs from T B S >= 2^23 flag bytes on: the smallest shapes that reach it (the only cases of this
    module above a few thousand env-steps).  `odd tail`: T B S = 8 388 612 = 4 mod 16, zero_fill's byte tail, once per plane; `joined`:
    T B S = 2^23 and terminations directly behind truncations: ONE fill of 2^24 bytes whose end is the block's fence."""
    env = supply_chain_env(S, [K] * S, ns, B, seed=5, variants={"rollout": "time_parallel", "block": block})
    assert T * B * S >= 1 << 23 and (T * B * S) % 16 == (0 if flags == "joined" else 4)
    kw = dict(joined_flags=True) if flags == "joined" else dict(terminations=flags == "separate")
    _rollout(env, T, "phx_zero_fill_kernel[flag planes]+" + kernel, **kw)


@pytest.mark.parametrize("family", ["sw", "sw replay", "sw fragment list", "sw fsm", "time_parallel pairs", "time_parallel whole_envs", "rules"])
def test_spare_rows_stay_untouched(family):
    """planes with three rows more than the call fills (check_tensor's AtLeast(T)): rows >= T keep the poison, in every fragment.  (The other
    families take their spare rows in their own cases: `spare` there.)"""
    if family.startswith("sw") and family != "sw fsm":
        S, K, B, ns, T, block = SW_SHAPES[0]
        exo = np.random.default_rng(1).integers(0, 5, (T, B, S * K)).astype(np.uint8) if family == "sw replay" else None
        k, T = (3, 23) if family == "sw fragment list" else (1, T)
        _rollout(_sw_env(S, K, B, ns, block), T, SW + ("[replay]" if exo is not None else ""), k=k, spare=3, exo=exo, hints=dict(exo_in_domain=exo is not None))
    elif family == "sw fsm":
        env = supply_chain_env(3, [2] * 3, 16, 64, fsm=True, seed=10, env_offset=13, variants={"rollout": "store_waves", "block": 48})
        _rollout(env, 41, SW + "[fsm]+" + FSM_LOOP, spare=3, state=SC_STATE + ("env.stage", "env.prev_stage"))
    elif family.startswith("time_parallel"):
        S, K, B, ns, T, block, kernel = TP_PAIRS if family.endswith("pairs") else TP_WHOLE
        env = supply_chain_env(S, [K] * S, ns, B, seed=3 + S, env_offset=2, variants={"rollout": "time_parallel", "block": block})
        _rollout(env, T, kernel, spare=3)
    else:
        handler = ph.state_rules([ph.StageRule("shop.stock", "<", 300, "RESTOCK")])(lambda env: None)
        handler._phx_skip_check = True
        env = supply_chain_env(9, [6] * 9, 9, 7, fsm=True, seed=5, restock_handler=handler)
        env._rules_checked = True
        _rollout(env, 11, "phx_sc_rollout_fsm_kernel[rules]", spare=3, masked=True, state=SC_STATE + ("env.stage",))


# ---- round 1's kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spare", [0, 3])
@pytest.mark.parametrize("variants", [{"rollout": "general"}, {}], ids=["general", "ragged"])
def test_general_rollout(variants, spare):
    """3 shops with 2, 7 and 1 customers, B = 5: 15 pairs, u8 planes of 105 bytes, f32 planes of 420"""
    env = supply_chain_env(3, [2, 7, 1], 4, 5, seed=2, env_offset=1, variants=variants)
    _rollout(env, 7, "phx_sc_rollout_kernel", spare=spare)


def test_action_that_rounds_below_zero():
    """tests/test_gpu_round5.py's case: the pre-scan finds a negative StockRequest, the store-wave launch returns at entry and round 1's
    kernel writes the planes behind the same call"""
    S, K, B, T = 9, 6, 64, 50
    env = supply_chain_env(S, [K] * S, 30, B, seed=3, variants={"rollout": "store_waves"})
    acts = np.random.default_rng(7).uniform(0, 100, (T, B, S)).astype(np.float32)
    acts[T // 2, B // 3, 4] = -7.3
    acts[3, 1, 0] = -0.51
    _rollout(env, T, SW + "[replay]+" + BELOW_ZERO, acts=acts)


# ---- FSM supply chains ------------------------------------------------------------------------------------------------------------------
FSM_STATE = SC_STATE + ("env.stage",)


@pytest.mark.parametrize("S,ks,B,ns,T,variants,kernel,spare", [
    (3, [2, 3, 1], 5, 12, 13, {"rollout": "lean"}, "phx_sc_rollout_fsm_kernel", 0),          # (ragged customer counts: the general loop whatever is asked)
    (3, [2, 3, 1], 5, 12, 13, {"rollout": "general"}, "phx_sc_rollout_fsm_kernel", 3),
    (9, [6] * 9, 7, 9, 11, {"rollout": "lean"}, "phx_sc_rollout_fsm_lean_kernel", 0),
    (9, [6] * 9, 7, 9, 11, {"rollout": "lean", "block": "whole_envs"}, "phx_sc_rollout_fsm_lean_kernel", 3),
    (9, [6] * 9, 7, 9, 11, {"rollout": "time_parallel"}, "phx_sc_rollout_fsm_lean_kernel", 0),   # (episodes shorter than the time-parallel kernel's chunk)
    (9, [6] * 9, 7, 9, 11, {"rollout": "general"}, "phx_sc_rollout_fsm_kernel", 0),
    (9, [6] * 9, 12, 100, 11, {"rollout": "time_parallel", "block": 12}, "phx_sc_rollout_fsmfast_kernel[pairs]+" + FSM_LOOP, 0),
    (9, [6] * 9, 12, 100, 11, {"rollout": "time_parallel", "block": "whole_envs"}, "phx_sc_rollout_fsmfast_kernel[whole_envs]+" + FSM_LOOP, 3),
], ids=["ragged lean", "ragged general", "lean", "lean whole_envs", "short episodes", "general", "fsmfast pairs", "fsmfast whole_envs"])
def test_fsm_rollout_kernels(S, ks, B, ns, T, variants, kernel, spare):
    """every plane is the oracle's everywhere (tests/test_gpu_round3.py compares these kernels without a mask: they write silent rows too).
    The time-parallel FSM kernel needs uniform customer counts and episodes of >= 20 steps: it runs at the SC64 shape with B = 12
    (108 pairs; u8 planes of 1188 bytes = 4 mod 16)."""
    env = supply_chain_env(S, ks, ns, B, fsm=True, seed=5 + S, env_offset=77, variants=variants)
    _rollout(env, T, kernel, spare=spare, state=FSM_STATE)


@pytest.mark.parametrize("S,ks,B,ns,T,thr", [(3, [2, 3, 1], 5, 12, 13, 60), (9, [6] * 9, 7, 9, 11, 300)])
def test_fsm_rule_rollout(S, ks, B, ns, T, thr):
    handler = ph.state_rules([ph.StageRule("shop.stock", "<", thr, "RESTOCK")])(lambda env: None)
    handler._phx_skip_check = True
    env = supply_chain_env(S, ks, ns, B, fsm=True, seed=5, restock_handler=handler)
    env._rules_checked = True                                  # (the lambda is a placeholder: the spec is what is under test)
    _rollout(env, T, "phx_sc_rollout_fsm_kernel[rules]", masked=True, state=FSM_STATE)


# ---- device policies -------------------------------------------------------------------------------------------------------------------
NETS = [((8,), "relu", "auto", ""), ((24, 16), "hard_tanh", "auto", ""), ((96,), "relu", "auto", "mfma_"), ((32, 32), "relu", "policy_mfma", "mfma_")]


@pytest.mark.parametrize("explore", [False, True], ids=["", "explore"])
@pytest.mark.parametrize("S,B,spare", [(9, 61, 0), (65, 3, 2)])
@pytest.mark.parametrize("widths,act,variant,mfma", NETS, ids=["8-relu", "24x16-hard_tanh", "96-relu", "32x32-relu policy_mfma"])
def test_policy_rollout(widths, act, variant, mfma, S, B, spare, explore):
    """T = 12 on-policy steps over two episode ends; exploring: raw_actions, action_logp and dist_inputs are fenced too and equal the
    restatement of the header's definition (tests/policy_explore_ref.py) on the noise, the env's planes equal the oracle replaying the
    device's actions"""
    from test_gpu_policy import _policy as det_policy
    from test_gpu_policy_explore import _check_against_restatement, _policy as gauss_policy
    T, ns = 12, 5
    env = supply_chain_env(S, [1 + s % 6 for s in range(S)], ns, B, seed=3 + S, env_offset=5, variants={"rollout": variant})
    kernel = f"phx_sc_rollout_policy_{mfma}{'explore_' if explore else ''}kernel"
    if not explore:
        _rollout(env, T, kernel, policy=det_policy(widths, act, seed=S + len(widths)), spare=spare)
        return
    pol = gauss_policy(widths, act, seed=S + len(widths))
    noise = np.random.default_rng(S).standard_normal((T, B, S)).astype(np.float32)
    o, d, frags, ro, first = _rollout(env, T, kernel, policy=pol, noise=noise, spare=spare)
    tr = frags[0][0]
    r = dict(obs=_np(tr.observations)[:T], actions=_np(tr.actions)[:T], truncated=_np(tr.truncations)[:T], raw=_np(tr.raw_actions)[:T],
             logp=_np(tr.action_logp)[:T], dist=_np(tr.dist_inputs)[:T])
    _check_against_restatement(pol, first, r, noise)


# ---- the market, the ads market, the message-passing engine -----------------------------------------------------------------------------
@pytest.mark.parametrize("spare", [0, 2])
def test_market_rollout(spare):
    """8 sellers, 24 buyers, B = 5: 160 pairs per row, over an episode end"""
    env = market_env(8, 24, 4, 10, 5, seed=9, exogenous="device")
    _rollout(env, 7, "phx_stk_rollout_kernel", spare=spare, state=("seller.tx", "buyer.bought"))


@pytest.mark.parametrize("spare", [0, 2])
def test_ads_rollout(spare):
    """the five advertisers of golden `ads_sampled` (budgets drawn on the device at every reset), B = 5: 25 pairs per row"""
    env = ads_env_from_golden(golden("ads_sampled"), batch=5, tracking=False, seed=3)
    _rollout(env, 7, "phx_ads_kernel[rollout]", spare=spare, masked=True, state=("env.stage", "adv.step_clicks", "adv.step_wins"))


@pytest.mark.parametrize("how,kernel,tracked,spare", [
    ("dynamic", "phx_generic_step_kernel[T-step loop]", False, 0), ("dynamic", "phx_generic_step_kernel[T-step loop]", True, 2),
    ("compiled", "phx_sched_step_kernel[T-step loop]", False, 2), ("compiled", "phx_sched_step_kernel[T-step loop]", True, 0)],
    ids=["dynamic", "dynamic tracked", "compiled", "compiled tracked"])
def test_engine_rollout(how, kernel, tracked, spare):
    """5 shops x 3 customers, B = 7 (35 pairs), T = 11 over an episode end of 9 steps, on the engine's dynamic kernel and on its compiled
    schedule; tracked: msg_log / msg_count of every step are fenced, records up to the count are the oracle's in order"""
    kw = dict(force_generic=True) if how == "compiled" else dict(variants={"step": "generic_dynamic"})
    env = supply_chain_env(5, [3] * 5, 9, 7, seed=4, env_offset=3, tracking=tracked, **kw)
    _rollout(env, 11, kernel, masked=True, record=tracked, spare=spare)


# ---- the step kernels, through the C ABI with every output fenced on its own ---------------------------------------------------------------
STEP_OUT = dict(obs=torch.float32, obs_valid=torch.uint8, reward=torch.float64, reward_valid=torch.uint8, terminated=torch.uint8,
                truncated=torch.uint8, done_valid=torch.uint8, all_terminated=torch.uint8, all_truncated=torch.uint8, err=torch.int32)


class FencedStep:
    """a phx_step_io whose outputs are fenced buffers of their own (DeviceEnv's own step buffers stay where they are: reset() uses them)"""

    def __init__(self, dev):
        self.dev, B, S, D = dev, dev.B, max(dev.S, 1), dev.D
        shapes = {"obs": (B, S, D), "all_terminated": (B,), "all_truncated": (B,), "err": (B,)}
        dt = dict(STEP_OUT)
        if dev.spec.trace_cap > 0:
            shapes.update(msg_log=(B, dev.spec.trace_cap, 16), msg_count=(B,)); dt.update(msg_log=torch.uint8, msg_count=torch.int32)
        self.planes, self.wholes = {}, {}
        for n in dt:
            self.planes[n], self.wholes[n] = fenced(shapes.get(n, (B, S)), dt[n], dev.device)
        self.io = _abi.PhxStepIO()
        for n, p in self.planes.items():
            setattr(self.io, n, p.data_ptr())

    def call(self, entry, actions=None, next_stage=None):
        for w in self.wholes.values():
            repoison(w)
        self.planes["err"].zero_()                              # (err is the caller's: the kernels only ever store a non-zero code)
        self.io.actions = None if actions is None else actions.data_ptr()
        self.io.next_stage = None if next_stage is None else next_stage.data_ptr()
        rc = getattr(self.dev.lib, entry)(self.dev.handle, C.byref(self.io), self.dev._stream())
        assert rc == 0, self.dev._err()
        torch.cuda.synchronize()

    def fences(self, what):
        for n, w in self.wholes.items():
            assert_fences(w, self.planes[n].shape[0], f"{what}: {n}")

    def check(self, o, what, masked_flags, msgs=True):
        """fences, poison and the oracle's values of every output.  ``masked_flags``: terminated / truncated where done_valid == 1 only (the
        market and the ads market, as their golden replays compare them)"""
        self.fences(what)
        g = {n: _np(p) for n, p in self.planes.items()}
        for n in ("obs_valid", "reward_valid", "done_valid", "all_terminated", "all_truncated", "err"):
            np.testing.assert_array_equal(g[n], getattr(o, n), err_msg=f"{what}: {n}")
        ov, rv, dv = o.obs_valid == 1, o.reward_valid == 1, (o.done_valid == 1) | (not masked_flags)
        assert_written(self.planes["obs"], f"{what}: obs", ~ov); assert_written(self.planes["reward"], f"{what}: reward", ~rv)
        np.testing.assert_array_equal(f32_bits(g["obs"])[ov], f32_bits(o.obs)[ov], err_msg=f"{what}: obs")
        np.testing.assert_array_equal(f64_bits(g["reward"])[rv], f64_bits(o.reward)[rv], err_msg=f"{what}: reward")
        for n in ("terminated", "truncated"):
            assert_written(self.planes[n], f"{what}: {n}", ~dv)
            np.testing.assert_array_equal(g[n][dv], getattr(o, n)[dv], err_msg=f"{what}: {n}")
        if "msg_count" in g and msgs:
            self.check_msgs(o, what)

    def check_msgs(self, o, what):
        """msg_count, and the records up to it in the oracle's order"""
        g = {n: _np(self.planes[n]) for n in ("msg_log", "msg_count")}
        np.testing.assert_array_equal(g["msg_count"], o.msg_count, err_msg=f"{what}: msg_count")
        live = np.arange(o.msg_log.shape[1])[None, :] < o.msg_count[:, None]
        assert_written(self.planes["msg_log"].view(torch.int64), f"{what}: msg_log", ~live)
        assert (np.ascontiguousarray(g["msg_log"]).view(LOG_DTYPE)[..., 0][live] == o.msg_log[live]).all(), f"{what}: msg_log"


def _sc(S, ks, B, **kw):
    return lambda: supply_chain_env(S, ks, 3, B, seed=9 + S, env_offset=3, **kw)


STEP_CASES = [
    ("sc 9x7", _sc(9, [6] * 9, 7, variants={"step": "fused"}), "phx_sc_step_kernel", 100.0, False),             # 63 bytes per u8 plane
    ("sc ragged 3x5", _sc(3, [2, 7, 1], 5), "phx_sc_step_kernel", 100.0, False),                                # 15
    ("sc fsm 9x7", _sc(9, [6] * 9, 7, fsm=True), "phx_sc_step_kernel", 100.0, False),
    ("wide 9x300", _sc(9, [6] * 9, 300, variants={"step": "wide"}), "phx_sc_step_wide_kernel", 100.0, False),   # 2700 bytes = 12 mod 16, 3 workgroups
    ("wide 1x3000", _sc(1, [3], 3000, variants={"step": "wide"}), "phx_sc_step_wide_kernel", 100.0, False),     # 3000 = 8 mod 16
    ("market packed", lambda: market_env(8, 24, 4, 3, 5, seed=9), "phx_stk_step_fast_kernel", 1.0, True),       # 160 bytes per u8 plane
    ("market degree 9", lambda: market_env(16, 7, 9, 3, 5, seed=9), "phx_stk_step_kernel", 1.0, True),          # 115
    ("ads", lambda: ads_env_from_golden(golden("ads_sampled"), batch=5, tracking=False, seed=3), "phx_ads_kernel[step]", 1.0, True),
    ("dynamic 9x7", _sc(9, [6] * 9, 7, variants={"step": "generic_dynamic"}), "phx_generic_step_kernel", 100.0, False),
    ("dynamic ragged tracked", _sc(3, [2, 7, 1], 5, tracking=True, variants={"step": "generic_dynamic"}), "phx_generic_step_kernel", 100.0, False),
    ("compiled 9x7", _sc(9, [6] * 9, 7, force_generic=True), "phx_sched_step_kernel", 100.0, False),
    ("compiled ragged tracked", _sc(3, [2, 7, 1], 5, tracking=True, force_generic=True), "phx_sched_step_kernel", 100.0, False),
    ("compiled fsm 9x7", _sc(9, [6] * 9, 7, fsm=True, force_generic=True), "phx_sched_step_kernel", 100.0, False),
]


@pytest.mark.parametrize("name,make,kernel,amax,masked_flags", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_outputs(name, make, kernel, amax, masked_flags):
    """three phx_step calls from reset (the third one ends the supply chains' and the markets' episodes): after each, every output of
    phx_step_io -- obs, obs_valid, reward, reward_valid, terminated, truncated, done_valid, all_terminated, all_truncated, err, and with
    tracking on msg_log and msg_count -- within its fences, written, and the oracle's"""
    env = make()
    o, d = OracleEnv(env.spec, threads=4), DeviceRunner(env.spec)
    o.reset(); d.reset()
    fs = FencedStep(d.dev)
    rng = np.random.default_rng(len(name))
    for t in range(3):
        a = rng.uniform(0, amax, (d.B, max(d.S, 1))).astype(np.float32)
        act = _dev_copy(d, a, np.float32); keep = act.clone()
        fs.call("phx_step", act)
        assert d.dev.last_kernel() == kernel, d.dev.last_kernel()
        o.step(a, None, None)
        fs.check(o, f"step {t}", masked_flags)
        _same_bytes(act, keep, "actions")


@pytest.mark.parametrize("tracked", [False, True], ids=["", "tracked"])
def test_step_begin_leaves_the_outputs_alone_and_step_end_writes_them(tracked):
    """phx_step_begin + phx_step_end around a host-side stage handler (always the engine's dynamic kernel): the first half writes no
    output (err aside: the caller's) but, with tracking on, the step's msg_log / msg_count; the second half writes every output and
    leaves msg_log / msg_count alone"""
    env = supply_chain_env(3, [2, 7, 1], 3, 5, fsm=True, seed=4, tracking=tracked)
    o, d = OracleEnv(env.spec, threads=2), DeviceRunner(env.spec)
    o.reset(); d.reset()
    fs = FencedStep(d.dev)
    msgs = ("msg_log", "msg_count") if tracked else ()
    rng = np.random.default_rng(3)
    for t in range(3):
        a = rng.uniform(0, 100, (d.B, d.S)).astype(np.float32)
        act = _dev_copy(d, a, np.float32)
        fs.call("phx_step_begin", act)
        assert d.dev.last_kernel() == "phx_generic_step_kernel", d.dev.last_kernel()
        fs.fences(f"begin {t}")
        for n, p in fs.planes.items():
            if n != "err" and n not in msgs:
                assert_poison(p, f"begin {t}: {n}")
        o.step_begin(a)
        if tracked:
            fs.check_msgs(o, f"begin {t}")
        np.testing.assert_array_equal(d.get_i32("shop.stock"), o.get_i32("shop.stock"))
        err = _np(fs.planes["err"]).copy()
        fs.call("phx_step_end", act)                              # (phx_step_io.actions stays set, as DeviceEnv.step_end leaves it)
        assert d.dev.last_kernel() == "phx_generic_step_kernel", d.dev.last_kernel()
        o.step_end()
        assert (err == 0).all()
        fs.check(o, f"end {t}", False, msgs=False)
        for n in msgs:
            assert_poison(fs.planes[n], f"end {t}: {n}")


# ---- the rest of the ABI's device outputs ---------------------------------------------------------------------------------------------------
def test_reset_with_a_mask_writes_the_masked_envs_rows_only():
    S, B = 9, 7
    env = supply_chain_env(S, [6] * S, 5, B, fsm=True, seed=2)
    o, d = OracleEnv(env.spec, threads=2), DeviceRunner(env.spec)
    o.reset(); d.reset()
    a = np.random.default_rng(0).uniform(0, 100, (B, S)).astype(np.float32)
    for _ in range(2):
        o.step(a, None, None); d.step(a, None, None)
    dev = d.dev
    obs, w_obs = fenced((B, S, dev.D), torch.float32, dev.device)
    valid, w_valid = fenced((B, S), torch.uint8, dev.device)
    mask = np.array([1, 0, 1, 0, 0, 1, 0], np.uint8)
    m = _dev_copy(d, mask, np.uint8)
    dev._check(dev.lib.phx_reset(dev.handle, m.data_ptr(), None, None, obs.data_ptr(), valid.data_ptr(), dev._stream()), "phx_reset")
    torch.cuda.synchronize()
    ro, rv = o.reset(mask)
    assert_fences(w_obs, B, "obs"); assert_fences(w_valid, B, "obs_valid")
    on = mask.astype(bool)
    assert_poison(obs[torch.from_numpy(~on)], "obs rows of envs outside the mask"); assert_poison(valid[torch.from_numpy(~on)], "obs_valid rows of envs outside the mask")
    np.testing.assert_array_equal(_np(valid)[on], rv[on])
    assert_written(valid[torch.from_numpy(on)], "obs_valid")
    sel = rv[on].astype(bool)
    assert_written(obs[torch.from_numpy(on)], "obs", ~sel)
    np.testing.assert_array_equal(f32_bits(_np(obs)[on])[sel], f32_bits(ro[on])[sel])
    np.testing.assert_array_equal(_np(m), mask)
    for f in ("shop.stock", "env.step", "env.stage"):
        np.testing.assert_array_equal(d.get_i32(f), o.get_i32(f), err_msg=f)


def test_mt_draw():
    """T = 7, B = 5, five customers: 175 bytes between the fences, numpy's own streams"""
    T, B, ks = 7, 5, [2, 2, 1]
    env = supply_chain_env(3, ks, 4, B, exogenous="mt19937", seed=3)
    d = DeviceRunner(env.spec); d.reset()
    seeds = [11, 2 ** 31 + 5, 0, 77, 123456789]
    d.dev.mt_seed(seeds)
    assert d.n_exo == 5
    out, whole = fenced((T, B, d.n_exo), torch.uint8, d.dev.device)
    d.dev.mt_draw(T, out=out)
    torch.cuda.synchronize()
    assert_fences(whole, T, "exo"); assert_written(out, "exo")
    for b, s in enumerate(seeds):
        want = np.random.RandomState(s).randint(5, size=T * 5).astype(np.uint8).reshape(T, 5)
        np.testing.assert_array_equal(_np(out)[:, b], want, err_msg=f"instance {b}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100_003])
def test_pack_and_unpack_flags(n):
    """the destination is exactly ceil(n / 64) words / n bytes between fences"""
    d = DeviceRunner(supply_chain_env(3, [2] * 3, 5, 4, seed=1).spec)
    dev = d.dev
    rng = np.random.default_rng(n)
    x = rng.integers(0, 2, n).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    x[-1] = 7
    src = _dev_copy(d, x, np.uint8); keep = src.clone()
    words = (n + 63) // 64
    packed, w_packed = fenced((words * 8,), torch.uint8, dev.device)
    dev.pack_flags(src, packed)
    torch.cuda.synchronize()
    assert_fences(w_packed, words * 8, "packed")
    want = np.packbits(np.pad(x != 0, (0, words * 64 - n)), bitorder="little")
    np.testing.assert_array_equal(_np(packed), want)
    _same_bytes(src, keep, "plane")
    back, w_back = fenced((n,), torch.uint8, dev.device)
    keep = packed.clone()
    dev.unpack_flags(packed, n, out=back)
    torch.cuda.synchronize()
    assert_fences(w_back, n, "unpacked"); assert_written(back, "unpacked")
    np.testing.assert_array_equal(_np(back), (x != 0).astype(np.uint8))
    _same_bytes(packed, keep, "packed")


@pytest.mark.parametrize("field,dtype", [("shop.stock", torch.int32), ("env.step", torch.int32)])
def test_get_state_into_a_device_buffer_of_the_fields_size(field, dtype):
    S, B = 9, 7                                                   # shop.stock: 252 bytes, env.step: 28
    env = supply_chain_env(S, [6] * S, 5, B, seed=2)
    o, d = OracleEnv(env.spec, threads=2), DeviceRunner(env.spec)
    o.reset(); d.reset()
    a = np.random.default_rng(0).uniform(0, 100, (B, S)).astype(np.float32)
    o.step(a, None, None); d.step(a, None, None)
    dev = d.dev
    n = dev.field(field).numel()
    dst, whole = fenced((n,), dtype, dev.device)
    nb = n * dst.element_size()
    assert dev.lib.phx_get_state(dev.handle, field.encode(), dst.data_ptr(), nb, dev._stream()) == nb
    torch.cuda.synchronize()
    assert_fences(whole, n, field); assert_written(dst, field)
    np.testing.assert_array_equal(_np(dst).reshape(B, -1), o.get_i32(field))
    assert dev.lib.phx_get_state(dev.handle, field.encode(), dst.data_ptr(), nb - 4, dev._stream()) < 0      # a smaller buffer is refused
