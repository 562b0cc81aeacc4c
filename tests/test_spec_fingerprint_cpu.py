"""CPU: what the library derives from a spec -- the strategic agents, the observation width, the exogenous columns and the state
blob's size -- for one spec of every family the spec code classifies, and the error code and text of one invalid spec per
validation step.  The state blob's size moves whenever the supply-chain / market classification, the lean-workspace rule, the
workspace rule or the rollout-scratch rule flips, so the table pins the classification without a GPU.

The expected numbers and texts were recorded from the library as it was before the spec code moved into phx_spec.hip; they are
literals on purpose (a change of the spec code that moves one of them has to say so here)."""
import ctypes as C

import pytest

import phantom_amd as ph
from phantom_amd import _abi
from helpers import market_env, supply_chain_env
import kats

PHX_EINVAL, PHX_EUNSUPPORTED = -1, -2


def _typed(fsm=False, **kw):
    s0, s1 = ph.UniformFloatSampler(0.0, 0.2), ph.UniformFloatSampler(0.05, 0.15, 0.07, 0.13)
    sup = {"SHOP0": ph.TypedShopAgent.Supertype(s0), "SHOP1": ph.TypedShopAgent.Supertype(s0),
           "SHOP2": ph.TypedShopAgent.Supertype(s1), "SHOP3": ph.TypedShopAgent.Supertype(0.15)}
    return supply_chain_env(5, [2] * 5, 10, 16, fsm=fsm, typed=True, agent_supertypes=sup, exogenous="device", seed=13, **kw)


def _rules_env():
    h = ph.state_rules([ph.StageRule("shop.stock", "<", 60, "RESTOCK")])(lambda env: None)
    h._phx_skip_check = True
    env = supply_chain_env(3, [2] * 3, 10, 16, fsm=True, seed=13, restock_handler=h)
    env._rules_checked = True
    return env


def _ads(batch=8, **kw):
    return ph.DigitalAdsEnv(num_steps=6, num_agents_theme={"travel": 2, "tech": 2}, batch_size=batch, seed=3,
                            agent_supertypes={f"ADV_{i + 1}": ph.AdvertiserAgent.Supertype(budget=0.3) for i in range(4)}, **kw)


SPECS = {
    "plain sc, uniform shops": lambda: supply_chain_env(9, [6] * 9, 100, 64).spec,
    "plain sc, non-uniform shops": lambda: supply_chain_env(3, [2, 3, 1], 10, 16).spec,
    "plain sc, non-uniform normaliser": lambda: supply_chain_env(3, [2] * 3, 10, 16, norm_customers=5).spec,
    "typed sc": lambda: _typed().spec,
    "typed fsm sc": lambda: _typed(fsm=True).spec,
    "sc, 300 shops": lambda: supply_chain_env(300, [1] * 300, 10, 4).spec,
    "fsm sc, handler-less": lambda: supply_chain_env(3, [2] * 3, 20, 16, fsm=True).spec,
    "fsm sc, tabulated handler": lambda: supply_chain_env(
        3, [2] * 3, 20, 16, fsm=True, restock_handler=ph.state_independent(lambda env: "SELL")).spec,
    "fsm sc, rule-form handler": lambda: _rules_env().spec,
    "market, packed": lambda: market_env(6, 20, 3, 5, 16).spec,
    "market, dynamic graph": lambda: market_env(6, 20, 3, 5, 16, rates=[0.7, 0.35, 1.0, 0.0, 0.5], exogenous="device").spec,
    "market, degree 9 (not packed)": lambda: market_env(17, 20, 9, 5, 16).spec,
    "market, A > 3072": lambda: market_env(40, 3100, 2, 5, 2).spec,
    "ads": lambda: _ads().spec,
    "ads, stochastic": lambda: _ads(connection_rates=(1.0, 0.8, 0.9)).spec,
    "generic net (cashboxes)": lambda: kats._net_spec(kats._cash_net()),
    "two-wave sc, forced generic, 91 agents": lambda: supply_chain_env(9, [9] * 9, 10, 16, force_generic=True).spec,
    "two-wave fsm sc, forced generic, 91 agents": lambda: supply_chain_env(9, [9] * 9, 10, 16, fsm=True, force_generic=True).spec,
    "sc, forced generic, 64 agents": lambda: supply_chain_env(9, [6] * 9, 10, 16, force_generic=True).spec,
    "sc, forced generic, 307 agents": lambda: supply_chain_env(51, [5] * 51, 10, 4, force_generic=True).spec,
    "sc with the mt19937 stream": lambda: supply_chain_env(3, [2] * 3, 10, 16, exogenous="mt19937", seed=9).spec,
    "sc with a message trace": lambda: supply_chain_env(3, [2] * 3, 10, 16, tracking=True).spec,
}

# name -> (phx_n_strategic, phx_obs_dim, phx_n_exo, phx_state_nbytes)
EXPECTED = {
    "plain sc, uniform shops": (9, 3, 54, 25344),
    "plain sc, non-uniform shops": (3, 3, 6, 4864),
    "plain sc, non-uniform normaliser": (3, 3, 6, 4864),
    "typed sc": (5, 4, 10, 7168),
    "typed fsm sc": (5, 4, 10, 7168),
    "sc, 300 shops": (300, 3, 300, 86528),
    "fsm sc, handler-less": (3, 3, 6, 4864),
    "fsm sc, tabulated handler": (3, 3, 6, 4864),
    "fsm sc, rule-form handler": (3, 3, 6, 8192),
    "market, packed": (26, 2, 0, 24320),
    "market, dynamic graph": (26, 2, 0, 25600),
    "market, degree 9 (not packed)": (37, 2, 0, 28672),
    "market, A > 3072": (3140, 2, 0, 1364992),
    "ads": (4, 3, 2, 10240),
    "ads, stochastic": (4, 3, 2, 10240),
    "generic net (cashboxes)": (0, 1, 0, 5888),
    "two-wave sc, forced generic, 91 agents": (9, 3, 81, 34816),
    "two-wave fsm sc, forced generic, 91 agents": (9, 3, 81, 34816),
    "sc, forced generic, 64 agents": (9, 3, 54, 14336),
    "sc, forced generic, 307 agents": (51, 3, 255, 18176),
    "sc with the mt19937 stream": (3, 3, 6, 45056),
    "sc with a message trace": (3, 3, 6, 8192),
}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_spec_fingerprint(name):
    lib = _abi.load_library()
    cs, keep = SPECS[name]().to_ctypes()
    ref = C.byref(cs)
    got = (lib.phx_n_strategic(ref), lib.phx_obs_dim(ref), lib.phx_n_exo(ref), lib.phx_state_nbytes(ref))
    assert got == EXPECTED[name]


def _i32(ptr):
    return C.cast(ptr, C.POINTER(C.c_int32))


def _u8(ptr):
    return C.cast(ptr, C.POINTER(C.c_uint8))


def _set(**fields):
    def mutate(cs):
        for k, v in fields.items():
            setattr(cs, k, v)
    return mutate


def _poke(field, cast, index, value):
    def mutate(cs):
        cast(getattr(cs, field))[index] = value
    return mutate


_SC = lambda: supply_chain_env(3, [2] * 3, 10, 16).spec
_FSM = lambda: supply_chain_env(3, [2] * 3, 10, 16, fsm=True).spec
_MKT = lambda: market_env(6, 20, 3, 5, 16).spec

# name -> (spec builder, what breaks it); one or two per step of derive()
INVALID = {
    "header: abi version": (_SC, _set(abi_version=99)),
    "header: batch": (_SC, _set(batch=0)),
    "header: shuffle with ignored connection errors": (_SC, _set(flags=_abi.F_SHUFFLE_BATCHES | _abi.F_IGNORE_CONN_ERRORS)),
    "samplers: negative count": (_SC, _set(n_samplers=-1)),
    "connections: negative count": (_SC, _set(n_conn=-1)),
    "type sources: sampler column out of range": (lambda: _typed().spec, _poke("type_src", _i32, 0, 99)),
    "adjacency: column out of range": (_SC, _poke("col", _i32, 0, -1)),
    "agents: unknown kind": (_SC, _poke("kind", _u8, 0, 0)),
    "agents: customer of a non-shop": (_SC, _poke("kind", _u8, 0, _abi.KIND_FACTORY)),
    "undirected: edge without its mirror": (_SC, _poke("col", _i32, 3, 2)),
    "lists: unknown env type": (_SC, _set(env_type=77)),
    "lists, fsm: initial stage": (_FSM, _set(initial_stage=5)),
    "lists, stackelberg: leader out of range": (_MKT, _poke("leaders", _i32, 0, 999)),
    "stage rules: negative count": (_FSM, _set(n_stage_rules=-1)),
    "stage rules: on a plain env": (lambda: _rules_env().spec, _set(env_type=_abi.ENV_PLAIN)),
}

# name -> (return code of phx_state_nbytes' derive: the error code as phx_create returns it, phx_last_error())
EXPECTED_ERRORS = {
    "header: abi version": (-1, "abi_version 99 != 10"),
    "header: batch": (-1, "batch must be positive"),
    "header: shuffle with ignored connection errors": (-2, "shuffle_batches with ignore_connection_errors"),
    "samplers: negative count": (-1, "sampler tables missing"),
    "connections: negative count": (-1, "StochasticNetwork tables missing"),
    "type sources: sampler column out of range": (-1, "agent 0: type_src out of range"),
    "adjacency: column out of range": (-1, "col out of range"),
    "agents: unknown kind": (-1, "agent 0: unknown kind 0"),
    "agents: customer of a non-shop": (-1, "agent 4: CustomerAgent.shop_id is not a ShopAgent"),
    "undirected: edge without its mirror": (-1, "edge 1->2 has no mirror edge (connections are undirected, network.py:122-123)"),
    "lists: unknown env type": (-1, "unknown env_type 77"),
    "lists, fsm: initial stage": (-1, "initial_stage out of range"),
    "lists, stackelberg: leader out of range": (-1, "leader out of range"),
    "stage rules: negative count": (-1, "stage_rules: bad count / NULL table"),
    "stage rules: on a plain env": (-1, "stage_rules need a FiniteStateMachineEnv"),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_spec_error(name):
    """phx_n_strategic returns -1 for every failure; the failure's own code is what phx_create returns -- without a GPU it
    fails before the first HIP call, so the code can be read there with a dummy, aligned blob address."""
    lib = _abi.load_library()
    build, mutate = INVALID[name]
    cs, keep = build().to_ctypes()
    mutate(cs)
    assert lib.phx_n_strategic(C.byref(cs)) == -1
    handle = C.c_void_p()
    rc = lib.phx_create(C.byref(cs), 0, C.c_void_p(256), 0, C.byref(handle))
    assert (rc, lib.phx_last_error().decode()) == EXPECTED_ERRORS[name]
    assert not handle.value
