"""The oracle's policy path (oracle/phx_oracle.c) for every policy the device accepts -- tanh, hidden layers up to 256 units -- against
tests/policy_ref.py bit for bit, over random networks and the edge-value networks of tests/policy_edges.py; every edge family tells the
definition from the perturbations it targets; the oracle and the CPU library's phx_rollout refuse what the device refuses, with its codes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import phantom_amd as ph
import policy_edges as pe
import policy_ref as pr
from phantom_amd import _abi
from helpers import f32_bits, supply_chain_env
from oracle import OracleEnv

ROOT = os.path.dirname(HERE)


def _random(widths, act, seed):
    rng = np.random.default_rng(seed)
    dims = [3] + list(widths) + [1]
    ws = [rng.normal(0, 1.5 / np.sqrt(dims[l]), (dims[l + 1], dims[l])).astype(np.float32) for l in range(len(dims) - 1)]
    bs = [rng.normal(0, 0.3, (dims[l + 1],)).astype(np.float32) for l in range(len(dims) - 1)]
    f = {"relu": lambda c: np.maximum(c, 0), "hard_tanh": lambda c: np.clip(c, -1, 1), "tanh": np.tanh}[act]
    h = np.zeros(3)
    for l in range(len(ws) - 1):
        h = f(ws[l].astype(np.float64) @ h + bs[l])
    y0 = float((ws[-1].astype(np.float64) @ h + bs[-1])[0])          # (the action at the zero observation is 50)
    return ph.MLPPolicy(ws, bs, activation=act, out_scale=60.0, out_bias=50.0 - 60.0 * y0)


def _oracle_rows(pol, o, x0, T):
    ro = o.rollout(T, policy=pol)
    x = pe.prev_obs(x0, ro)
    want = pr.action(pol, x)
    bad = np.flatnonzero(f32_bits(want) != f32_bits(ro["actions"].reshape(-1)))
    assert bad.size == 0, f"{bad.size} actions differ; first: obs {x[bad[0]]} oracle {ro['actions'].reshape(-1)[bad[0]]!r} restatement {want[bad[0]]!r}"
    return ro, x


@pytest.mark.parametrize("widths,act", [((256, 256), "tanh"), ((256,), "tanh"), ((96, 224), "relu"), ((17, 256), "hard_tanh"),
                                        ((64, 64), "tanh"), ((1, 256), "tanh"), ((256, 1), "relu"), ((5,), "tanh")])
def test_oracle_evaluates_tanh_and_wide_policies_like_the_restatement(widths, act):
    env = supply_chain_env(5, [3, 1, 6, 2, 4], 7, 6, seed=9)
    o = OracleEnv(env.spec, threads=4)
    x0, _ = o.reset()
    pol = _random(widths, act, seed=len(widths) + widths[0])
    ro, _ = _oracle_rows(pol, o, x0, 17)
    assert ro["truncated"].any() and np.unique(ro["actions"]).size > 10


@pytest.mark.parametrize("cid,act,widths,j,kern,fam", pe.cases(), ids=[c[0] for c in pe.cases()])
def test_edge_family_oracle_and_sensitivity(cid, act, widths, j, kern, fam):
    """each network of the family: the oracle's on-policy rows == the restatement's actions, bit for bit; over the family's inputs, every
    perturbation it targets changes at least one action"""
    nets, targets = pe.families(act, widths, j)[fam]
    env = supply_chain_env(9, [6] * 9, 7, 4, seed=3)
    o = OracleEnv(env.spec, threads=4)
    x0, _ = o.reset()
    hit = {t: False for t in targets}
    for pol in nets:
        ro, x = _oracle_rows(pol, o, x0, 16)
        x0 = ro["last_obs"]
        for t in targets:
            hit[t] = hit[t] or pe.sensitive(pol, x, t)
    assert all(hit.values()), f"{cid}: the perturbations {[t for t, h in hit.items() if not h]} change no action"


def test_tanh_rational_never_exceeds_one_below_the_threshold():
    """every f32 in [0.5, PHX_TANH_SAT): the rational is <= 1, so the definition's "t > 1 ? 1 : t" is never active for a finite
    pre-activation (tanh_no_clamp is the definition itself; no edge network can target it)"""
    lo, hi = int(np.float32(0.5).view(np.uint32)), int(pr.TANH_SAT.view(np.uint32))
    for s in range(lo, hi, 1 << 22):
        a = np.arange(s, min(s + (1 << 22), hi), dtype=np.uint32).view(np.float32)
        t = pr.tanh_def(a, {"tanh_no_clamp"})
        assert (t <= 1).all(), a[t > 1][:4]


def test_perturbations_are_validated():
    with pytest.raises(ValueError):
        pr.action(_random((4,), "relu", 0), np.zeros((1, 3), np.float32), {"no_such_change"})


# ---- what the device refuses ----------------------------------------------------------------------------------------------------------------
def _broken(pol, how):
    st = pol.host_struct()
    if how.startswith("width"):
        st.width[0] = int(how[5:])
    elif how == "activation3":
        st.activation = 3
    elif how == "misaligned":
        st.w[1] = st.w[1] + 2
    elif how == "null":
        st.b[1] = None
    elif how == "hidden3":
        st.n_hidden = 3
    elif how == "out_lo":
        st.out_lo = -1.0
    return st


BROKEN = ["width65", "width257", "width288", "width0", "activation3", "misaligned", "null", "hidden3", "out_lo"]


@pytest.mark.parametrize("how", BROKEN)
def test_oracle_refuses_what_the_device_refuses(how):
    env = supply_chain_env(3, [2] * 3, 5, 4, seed=1)
    o = OracleEnv(env.spec, threads=1)
    o.reset()
    pol = _random((256, 256), "tanh", 1)
    with pytest.raises(ValueError):
        o.rollout(4, policy=_broken(pol, how))
    o.rollout(4, policy=pol.host_struct())                             # (the same struct unbroken: served)


@pytest.fixture(scope="module")
def cpu_lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "libphantom_cpu.so"])
    return _abi.bind_signatures(C.CDLL(os.path.join(ROOT, "oracle", "libphantom_cpu.so")))


def _cpu_rollout(lib, spec, T, st, **extra):
    cs, keep = spec.to_ctypes()
    n = lib.phx_state_nbytes(C.byref(cs))
    blob = np.zeros(n, np.uint8)
    h = C.c_void_p()
    assert lib.phx_create(C.byref(cs), 0, blob.ctypes.data, n, C.byref(h)) == 0
    try:
        B, S = spec.batch, lib.phx_n_strategic(C.byref(cs))
        obs = np.zeros((B, S, 3), np.float32); ov = np.zeros((B, S), np.uint8)
        assert lib.phx_reset(h, None, None, None, obs.ctypes.data, ov.ctypes.data, None) == 0
        bufs = [np.zeros((T, B, S, 3), np.float32)] + [np.zeros((T, B, S), np.float32) for _ in range(2)] + [np.zeros((T, B, S), np.uint8) for _ in range(2)]
        io = _abi.PhxRolloutIO()
        io.T = T
        io.obs, io.action_out, io.reward, io.terminated, io.truncated = (b.ctypes.data for b in bufs)
        io.policy = C.addressof(st)
        for k, v in extra.items():
            setattr(io, k, v)
        return lib.phx_rollout(h, C.byref(io), None), bufs[1]
    finally:
        lib.phx_destroy(h)


@pytest.mark.parametrize("how", BROKEN)
def test_cpu_library_refuses_with_the_device_codes(cpu_lib, how):
    spec = supply_chain_env(3, [2] * 3, 5, 4, seed=1).spec
    pol = _random((256, 256), "tanh", 1)
    rc, _ = _cpu_rollout(cpu_lib, spec, 4, _broken(pol, how))
    assert rc == -1                                                    # PHX_EINVAL, as phx_api.hip returns for phx_policy_mlp's rules
    st = pol.host_struct()
    rc, acts = _cpu_rollout(cpu_lib, spec, 4, st)
    assert rc == 0 and np.unique(acts).size > 1
    acts_in = np.zeros((4, 4, 3), np.float32)
    assert _cpu_rollout(cpu_lib, spec, 4, st, actions=acts_in.ctypes.data)[0] == -1      # `policy` excludes replayed actions
    fsm = supply_chain_env(3, [2] * 3, 10, 4, fsm=True).spec
    assert _cpu_rollout(cpu_lib, fsm, 4, st)[0] == -2                  # PHX_EUNSUPPORTED: not a plain supply chain
