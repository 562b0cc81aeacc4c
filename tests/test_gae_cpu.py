"""CPU: the definition of phx_gae (include/phantom_amd_gae.h) as tests/gae_ref.py restates it, against RLlib's formula in f64
within a computed forward error bound; its special cases; the symbol and the two headers; FragmentBatch's critic columns."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gae_ref
from helpers import f32_bits
from phantom_amd import _abi
from phantom_amd.rollout import FragmentBatch


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_restatement_against_rllibs_formula_in_f64(gamma, lam):
    """|f32 definition - f64 formula| <= 2 E_t, E_t the first-order forward bound computed in f64 from the f64 values
    (gae_ref.gae_f64); the factor 2 covers the second-order terms.  value_target: one more 2^-24 |vt|."""
    rng = np.random.default_rng(7)
    T, N = 57, 96
    case = gae_ref.random_case(rng, T, N)
    tr, te = case["truncated"], case["terminated"]
    assert tr[0].any() and te[0].any() and tr[T - 1].any() and te[T - 1].any() and (tr & te).any()
    assert (tr[1:-1] | te[1:-1]).any(axis=0).sum() > N // 2 and not (tr | te)[:-1].any(axis=0).all()      # cut and uncut columns
    adv, vt = gae_ref.gae(gamma=gamma, lam=lam, **case)
    a64, v64, e_adv, e_vt = gae_ref.gae_f64(gamma=gamma, lam=lam, **case)
    assert adv.dtype == vt.dtype == np.float32
    assert (np.abs(adv.astype(np.float64) - a64) <= 2 * e_adv).all()
    assert (np.abs(vt.astype(np.float64) - v64) <= 2 * e_vt).all()
    assert e_adv.max() < 1e-4                              # (the bound is a few ulps, not a loose number)
    # the f64 formula is RLlib's: per trajectory segment, discount_cumsum of the deltas
    n = int(np.flatnonzero((tr | te)[:-1].any(axis=0))[0])
    cuts = np.flatnonzero((tr | te)[:, n] != 0).tolist()
    t1 = cuts[0]
    g, gl = np.float64(np.float32(gamma)), np.float64(np.float32(gamma)) * np.float64(np.float32(lam))
    v = case["vf_pred"][:, n].astype(np.float64)
    last_r = 0.0 if te[t1, n] else np.float64(case["vf_next"][t1, n])
    vpred_t = np.concatenate([v[:t1 + 1], [last_r]])
    delta = case["reward"][:t1 + 1, n].astype(np.float64) + g * vpred_t[1:] - vpred_t[:-1]
    want = np.array([sum(gl ** (k - t) * delta[k] for k in range(t, t1 + 1)) for t in range(t1 + 1)])
    np.testing.assert_allclose(a64[:t1 + 1, n], want, rtol=1e-12, atol=1e-12)


def test_without_a_critic_the_advantages_are_discounted_returns():
    rng = np.random.default_rng(3)
    case = gae_ref.random_case(rng, 23, 10)
    case["vf_pred"] = None
    gamma = np.float32(0.97)
    adv, vt = gae_ref.gae(gamma=gamma, lam=1.0, **case)
    np.testing.assert_array_equal(f32_bits(adv), f32_bits(vt))
    ret = np.zeros((23, 10))
    cut = (case["truncated"] != 0) | (case["terminated"] != 0)
    cut[-1] = True
    boot = np.where(case["terminated"] != 0, 0.0, case["vf_next"].astype(np.float64))
    for t in range(22, -1, -1):
        ret[t] = case["reward"][t] + np.float64(gamma) * np.where(cut[t], boot[t], ret[t + 1] if t < 22 else 0.0)
    np.testing.assert_allclose(adv, ret, rtol=1e-5, atol=1e-5)


def test_gamma_zero_is_reward_minus_value_exactly():
    rng = np.random.default_rng(4)
    case = gae_ref.random_case(rng, 19, 12)
    adv, vt = gae_ref.gae(gamma=0.0, lam=0.5, **case)
    want = (case["reward"].astype(np.float64) - case["vf_pred"].astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(f32_bits(adv + np.float32(0)), f32_bits(want + np.float32(0)))


def test_a_column_is_unaffected_by_its_neighbours():
    rng = np.random.default_rng(5)
    case = gae_ref.random_case(rng, 31, 40)
    adv, vt = gae_ref.gae(gamma=0.99, lam=0.9, **case)
    perm = rng.permutation(40)
    adv_p, vt_p = gae_ref.gae(gamma=0.99, lam=0.9, **{k: v[:, perm] for k, v in case.items()})
    np.testing.assert_array_equal(f32_bits(adv_p), f32_bits(adv[:, perm]))
    np.testing.assert_array_equal(f32_bits(vt_p), f32_bits(vt[:, perm]))
    one, _ = gae_ref.gae(gamma=0.99, lam=0.9, **{k: v[:, 17:18] for k, v in case.items()})
    np.testing.assert_array_equal(f32_bits(one), f32_bits(adv[:, 17:18]))


def test_unread_vf_next_elements_do_not_matter():
    rng = np.random.default_rng(6)
    case = gae_ref.random_case(rng, 20, 16)
    adv, vt = gae_ref.gae(**case)
    case["vf_next"] = np.where(gae_ref.reads_vf_next(case["terminated"], case["truncated"]), case["vf_next"], np.float32(np.nan))
    adv2, vt2 = gae_ref.gae(**case)
    np.testing.assert_array_equal(f32_bits(adv2), f32_bits(adv))
    np.testing.assert_array_equal(f32_bits(vt2), f32_bits(vt))


def test_symbol_and_headers():
    lib = _abi.load_library()
    assert hasattr(lib, "phx_gae")
    assert "phx_gae" not in _abi.EXPORTS and _abi.ABI_VERSION == 10
    new = open(os.path.join(ROOT, "include", "phantom_amd_gae.h")).read()
    old = open(os.path.join(ROOT, "include", "phantom_amd.h")).read()
    assert "int phx_gae(const phx_gae_io* io, void* stream);" in new
    assert "phx_gae" not in old
    import ctypes
    assert ctypes.sizeof(_abi.PhxGaeIO) == 80 and _abi.PhxGaeIO.reward.offset == 24 and _abi.PhxGaeIO.value_target.offset == 72


def _fragment(B=3, S=2, T=5, D=3, **kw):
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(B, S, T, D)).astype(np.float32)
    f = lambda: rng.normal(size=(B, S, T)).astype(np.float32)
    z = np.zeros((B, S, T), bool)
    t = np.broadcast_to(np.arange(T, dtype=np.int32), (B, T)).copy()
    return FragmentBatch(["a", "b"], obs, obs + 1, f(), f(), z, z.copy(), t, np.zeros((B, T), np.int64), **kw)


def test_fragment_batch_critic_columns():
    B, S, T = 3, 2, 5
    planes = {k: (100 * i + np.arange(B * S * T, dtype=np.float32)).reshape(B, S, T) for i, k in enumerate(("vf_preds", "advantages", "value_targets"))}
    cols = _fragment(**planes).to_sample_batches()["default_policy"]
    for k, p in planes.items():                                # rows in (env, agent, step) order
        np.testing.assert_array_equal(cols[k], p.reshape(-1))
        assert cols[k].shape == cols["rewards"].shape
    assert FragmentBatch.COLUMNS == ("obs", "new_obs", "actions", "rewards", "terminateds", "truncateds")
    plain = _fragment()
    assert plain.vf_preds is None and plain.advantages is None and plain.value_targets is None
    assert not {"vf_preds", "advantages", "value_targets"} & set(plain.to_sample_batches()["default_policy"])
    valid = np.ones((B, S, T), np.uint8)
    valid[1, 0, 2] = valid[2, 1, 4] = 0
    masked = _fragment(obs_valid=valid, **planes).to_sample_batches()["default_policy"]
    for k, p in planes.items():
        np.testing.assert_array_equal(masked[k], p.reshape(-1)[valid.reshape(-1).astype(bool)])
    per_policy = _fragment(**planes).to_sample_batches(lambda aid: aid)
    np.testing.assert_array_equal(per_policy["b"]["advantages"], planes["advantages"][:, 1].reshape(-1))
