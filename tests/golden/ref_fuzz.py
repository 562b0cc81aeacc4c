#!/usr/bin/env python
"""Random differential runs of the CPU oracle against the reference (jpmorganchase/Phantom).  Complements the
committed golden vectors: random agent orders, several factories, ragged customers, random FSM stage tables
(acting / rewarded lists), partial action dicts, tutorial-2 typed shops, random Stackelberg markets on static and
stochastic networks.

A case is a seeded random scenario.  Run LIVE (the reference imported from its source tree through ref_import.py, in
the build container only), the reference steps it and what it returned -- observation / reward / done keys and values,
the customers' draws, the shops' state, the connectivity of stochastic networks -- is checked against the oracle and
can be kept as a TRACE of plain arrays.  Run from a trace (``run_case(case, trace)``), the same scenario is rebuilt on
the phantom_amd side alone and the oracle is checked against the recorded reference output: no reference needed
(tests/test_oracle_vs_live_reference.py replays tests/golden/live_fuzz.npz, written by gen_goldens_live.py).

    python tests/golden/ref_fuzz.py [N] [first]          (live)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import phantom_amd as ph  # noqa: E402
from helpers import f32_bits, f64_bits  # noqa: E402
from oracle import OracleEnv  # noqa: E402


def _ref():
    """(reference phantom package, reference supply-chain example module, gen_goldens) -- live runs only"""
    sys.dont_write_bytecode = True
    import ref_import
    rph, rsc = ref_import.import_phantom(), ref_import.import_supply_chain()
    import gen_goldens as gg  # (DrawRecorder, market agents, typed shop class)
    return rph, rsc, gg


class _Trace:
    """the reference's side of one case: recorded while the live reference runs, read back when replaying"""

    def __init__(self, arrays=None):
        self.live = arrays is None
        self.lists = {}
        self.arrays = arrays
        self.pos = {}

    def put(self, name, value):
        self.lists.setdefault(name, []).append(np.asarray(value))
        return np.asarray(value)

    def get(self, name):
        k = self.pos.get(name, 0)
        self.pos[name] = k + 1
        return self.arrays[name][k]

    def take(self, name, live_fn):
        """the next `name` record: computed from the reference (live) or read from the trace"""
        return self.put(name, live_fn()) if self.live else self.get(name)

    def to_arrays(self):
        return {k: np.stack(v) for k, v in self.lists.items()}


def _keyed_rows(d, sidx, Ss, D, dtype=np.float32):
    """a reference dict {agent id: vector} as (present [Ss] u8, values [Ss, D], lengths [Ss] i32)"""
    present, vals, lens = np.zeros(Ss, np.uint8), np.zeros((Ss, D), dtype), np.zeros(Ss, np.int32)
    for k, v in d.items():
        s = sidx[k]
        v = np.asarray(v, dtype).ravel()
        present[s], vals[s, :len(v)], lens[s] = 1, v, len(v)
    return present, vals, lens


def _reward_rows(rewards, sidx, Ss):
    """the reference's reward dict as (kind [Ss] u8: 0 absent / 1 value / 2 None, value [Ss] f64)"""
    kind, val = np.zeros(Ss, np.uint8), np.zeros(Ss, np.float64)
    for k, r in rewards.items():
        if k in sidx:
            kind[sidx[k]] = 2 if r is None else 1
            val[sidx[k]] = 0.0 if r is None else np.float64(r)
    return kind, val


def _check_step(o, case, t, ref, D_cmp=None, done_keys=True):
    present, vals, lens, rkind, rval, dkey = ref
    for s in range(len(present)):
        assert present[s] == o.obs_valid[0, s], (case, t, "obs key", s)
        if present[s]:
            n = int(lens[s]) if D_cmp is None else D_cmp
            assert np.array_equal(f32_bits(vals[s, :n]), f32_bits(o.obs[0, s, :n])), (case, t, "obs", s)
        assert rkind[s] == o.reward_valid[0, s], (case, t, "reward key", s, rkind[s], o.reward_valid[0, s])
        if rkind[s] == 1:
            assert f64_bits(rval[s]) == f64_bits(o.reward[0, s]), (case, t, "reward", s)
        if done_keys:
            assert dkey[s] == o.done_valid[0, s], (case, t, "done key", s)


def supply_chain_case(rng, case, tr):
    if tr.live:
        rph, rsc, gg = _ref()
    nF, S = int(rng.randint(1, 4)), int(rng.randint(1, 8))
    ks = [int(rng.randint(0, 7)) for _ in range(S)]
    norm = int(rng.randint(1, 8))
    fsm, typed = rng.rand() < 0.5, rng.rand() < 0.3
    num_steps, T = int(rng.randint(1, 8)), int(rng.randint(4, 30))
    if tr.live:
        rsc.NUM_CUSTOMERS = norm
    fac = [f"F{i}" for i in range(nF)]
    shop_fac = [fac[rng.randint(nF)] for _ in range(S)]
    names = [("S", i) for i in range(S)] + [("F", i) for i in range(nF)] + [("C", i, j) for i in range(S) for j in range(ks[i])]
    names = [names[i] for i in rng.permutation(len(names))]

    def aid(t):
        return f"SHOP{t[1]}" if t[0] == "S" else (fac[t[1]] if t[0] == "F" else f"C{t[1]}_{t[2]}")
    RShop = (gg.make_typed_shop_class() if typed else rsc.ShopAgent) if tr.live else None
    r_agents, m_agents = [], []
    for t in names:
        if t[0] == "S":
            if tr.live:
                r_agents.append(RShop(aid(t), factory_id=shop_fac[t[1]]))
            cls = ph.TypedShopAgent if typed else ph.ShopAgent
            m_agents.append(cls(aid(t), factory_id=shop_fac[t[1]], num_customers=norm))
        elif t[0] == "F":
            if tr.live:
                r_agents.append(rsc.FactoryAgent(aid(t)))
            m_agents.append(ph.FactoryAgent(aid(t)))
        else:
            if tr.live:
                r_agents.append(rsc.CustomerAgent(aid(t), shop_id=f"SHOP{t[1]}"))
            m_agents.append(ph.CustomerAgent(aid(t), shop_id=f"SHOP{t[1]}"))
    rnet = rph.Network(r_agents) if tr.live else None
    mnet = ph.Network(m_agents)
    conns = [(f"SHOP{i}", shop_fac[i]) for i in range(S)] + [(f"C{i}_{j}", f"SHOP{i}") for i in range(S) for j in range(ks[i])]
    for k in rng.permutation(len(conns)):
        if tr.live:
            rnet.add_connection(*conns[k])
        mnet.add_connection(*conns[k])
    shops = [f"SHOP{i}" for i in range(S)]
    custs = [f"C{i}_{j}" for i in range(S) for j in range(ks[i])]
    sup_r = sup_m = None
    r_samplers, m_samplers = [], []
    if typed:
        n_sm = int(rng.randint(0, 3))
        prm = [(float(rng.uniform(0, 0.1)), float(rng.uniform(0.1, 0.2)), None if rng.rand() < 0.5 else 0.04,
                None if rng.rand() < 0.5 else 0.16) for _ in range(n_sm)]
        if tr.live:
            from phantom.utils.samplers import UniformFloatSampler as RUniform
            r_samplers = [RUniform(*q) for q in prm]
        m_samplers = [ph.UniformFloatSampler(*q) for q in prm]
        sup_r, sup_m = {}, {}
        for s in shops:
            r = rng.rand()
            if r < 0.25:
                continue                                     # no supertype passed: Supertype() defaults
            if r < 0.6 and n_sm:
                j = int(rng.randint(n_sm))
                if tr.live:
                    sup_r[s] = RShop.Supertype(excess_stock_weight=r_samplers[j])
                sup_m[s] = ph.TypedShopAgent.Supertype(excess_stock_weight=m_samplers[j])
            else:
                v = float(rng.randint(0, 21)) / 100.0
                if tr.live:
                    sup_r[s] = RShop.Supertype(excess_stock_weight=v)
                sup_m[s] = ph.TypedShopAgent.Supertype(excess_stock_weight=v)
    renv = None
    if fsm:
        n_st = int(rng.randint(2, 5))                          # 2..4 stages in a cycle, random tables
        snames = [chr(ord("A") + i) for i in range(n_st)]
        tabs = []
        for i in range(n_st):
            acting = [c for c in custs if rng.rand() < 0.6] + [s for s in shops if rng.rand() < 0.5]
            acting = [acting[j] for j in rng.permutation(len(acting))]
            rewarded = None if rng.rand() < 0.3 else [s for s in shops if rng.rand() < 0.5]
            tabs.append((acting, rewarded))
        init = snames[int(rng.randint(n_st))]
        if tr.live:
            renv = rph.FiniteStateMachineEnv(num_steps=num_steps, network=rnet, initial_stage=init, agent_supertypes=sup_r,
                                             stages=[rph.FSMStage(nm, acting_agents=a_, rewarded_agents=r_, next_stages=[snames[(i + 1) % n_st]])
                                                     for i, (nm, (a_, r_)) in enumerate(zip(snames, tabs))])
        menv = ph.FiniteStateMachineEnv(num_steps, mnet, initial_stage=init, agent_supertypes=sup_m,
                                        stages=[ph.FSMStage(nm, acting_agents=a_, rewarded_agents=r_, next_stages=[snames[(i + 1) % n_st]])
                                                for i, (nm, (a_, r_)) in enumerate(zip(snames, tabs))])
        acting_of = {nm: a_ for nm, (a_, r_) in zip(snames, tabs)}
    else:
        if tr.live:
            renv = rph.PhantomEnv(num_steps=num_steps, network=rnet, agent_supertypes=sup_r)
        menv = ph.PhantomEnv(num_steps, mnet, agent_supertypes=sup_m)
    spec = menv.spec
    if tr.live:
        assert [str(a) for a in spec.agent_ids] == [str(a) for a in renv.agent_ids]
    o = OracleEnv(spec)
    sidx = {spec.agent_ids[a]: s for s, a in enumerate(spec.strategic_idx)}
    cust_rank = {c: r for r, c in enumerate(a for a in spec.agent_ids if str(a).startswith("C"))}
    shop_rank = {s: r for r, s in enumerate(a for a in spec.agent_ids if str(a).startswith("SHOP"))}
    Ss, D = spec.n_strategic, spec.obs_dim
    need_reset = True
    for t in range(T):
        if need_reset:
            if tr.live:
                robs, _ = renv.reset()
                if spec.n_samplers:
                    assert len(renv._samplers) == spec.n_samplers
            # the values the reference's samplers drew at this reset, in env._samplers order
            vals = tr.take("sampler_values", lambda: np.asarray([sm.value for sm in renv._samplers], np.float64))
            oobs, ovalid = o.reset(None, vals[None] if spec.n_samplers else None)
            present, rvals, lens = (tr.put(n, x) for n, x in zip(("reset_present", "reset_obs", "reset_len"), _keyed_rows(robs, sidx, Ss, D))) \
                if tr.live else (tr.get("reset_present"), tr.get("reset_obs"), tr.get("reset_len"))
            assert (present == ovalid[0]).all(), (case, t, "reset keys")
            for s in np.flatnonzero(present):
                assert np.array_equal(f32_bits(rvals[s, :lens[s]]), f32_bits(oobs[0, s, :lens[s]])), (case, t, "reset obs", s)
            need_reset = False
        acts, act, valid = {}, np.zeros((1, Ss), np.float32), np.zeros((1, Ss), np.uint8)
        for sname, s in sidx.items():
            if rng.rand() < 0.85:
                a = np.float32(rng.choice([rng.uniform(-10, 130), rng.randint(0, 100) + 0.5]))
                acts[sname] = np.array([a], np.float32); act[0, s] = a; valid[0, s] = 1
        if tr.live:
            with gg.DrawRecorder() as rec:
                st = renv.step(acts)
            # the customers that drew, in consumption order = acting order
            if fsm:
                acting = [c for c in acting_of[renv.previous_stage] if str(c).startswith("C")]
            else:
                acting = [c for c in spec.agent_ids if str(c).startswith("C")]
            exo = np.zeros(max(spec.n_exo, 1), np.uint8)
            assert len(rec.draws) == len(acting), (case, t, "draw count")
            for c, v in zip(acting, rec.draws):
                exo[cust_rank[c]] = v
            tr.put("exo", exo)
            ref = [tr.put(n, x) for n, x in zip(("obs_present", "obs", "obs_len"), _keyed_rows(st.observations, sidx, Ss, D))]
            ref += [tr.put(n, x) for n, x in zip(("reward_kind", "reward"), _reward_rows(st.rewards, sidx, Ss))]
            ref.append(tr.put("done_present", _keyed_rows({k: [0] for k in st.terminations if k in sidx}, sidx, Ss, 1)[0]))
            flags = tr.put("all_flags", np.asarray([bool(st.truncations["__all__"]), bool(st.terminations["__all__"])], np.uint8))
            shop_state = np.zeros((len(shop_rank), 3), np.int32)
            for s in shops:
                ag = renv.agents[s]
                shop_state[shop_rank[s]] = (ag.stock, ag.sales, ag.missed_sales)
            tr.put("shop_state", shop_state)
        else:
            exo = tr.get("exo")
            ref = [tr.get(n) for n in ("obs_present", "obs", "obs_len", "reward_kind", "reward", "done_present")]
            flags, shop_state = tr.get("all_flags"), tr.get("shop_state")
        o.step(act, valid, exo[None, :spec.n_exo] if spec.n_exo else None)
        assert o.err[0] == 0
        _check_step(o, case, t, ref)
        assert flags[0] == o.all_truncated[0] and flags[1] == o.all_terminated[0], (case, t, "__all__")
        for s in shops:
            kr = shop_rank[s]
            assert tuple(shop_state[kr]) == (o.get_i32("shop.stock")[0, kr], o.get_i32("shop.sales")[0, kr],
                                             o.get_i32("shop.missed_sales")[0, kr]), (case, t, "state", s)
        if flags.any():
            need_reset = True
    return f"sc S={S} ks={ks} nF={nF} fsm={fsm} typed={typed} ns={num_steps}"


def market_case(rng, case, tr):
    if tr.live:
        rph, rsc, gg = _ref()
    L, Fw = int(rng.randint(1, 7)), int(rng.randint(1, 16))
    num_steps, T = int(rng.randint(1, 9)), int(rng.randint(4, 26))
    stochastic = rng.rand() < 0.5
    names = [("S", i) for i in range(L)] + [("B", i) for i in range(Fw)]
    names = [names[i] for i in rng.permutation(len(names))]
    values = [float(rng.randint(1, 9)) / 8.0 for _ in range(Fw)]
    r_agents = [gg.SellerAgent(f"S{i}") if k == "S" else gg.BuyerAgent(f"B{i}", values[i]) for k, i in names] if tr.live else None
    m_agents = [ph.SellerAgent(f"S{i}") if k == "S" else ph.BuyerAgent(f"B{i}", values[i]) for k, i in names]
    pairs = [(f"B{f}", f"S{l}") for f in range(Fw) for l in range(L) if rng.rand() < min(1.0, 2.5 / L)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    seed = int(rng.randint(1 << 30))
    rnet = None
    if stochastic:
        rates = [float(rng.choice([0.0, 0.3, 0.7, 1.0])) for _ in pairs]
        if tr.live:
            np.random.seed(seed)
            rnet = rph.StochasticNetwork(r_agents)
            for (u, v), r in zip(pairs, rates):
                rnet.add_connection(u, v, r)
        np.random.seed(seed)
        mnet = ph.StochasticNetwork(m_agents)
        for (u, v), r in zip(pairs, rates):
            mnet.add_connection(u, v, r)
    else:
        rnet, mnet = (rph.Network(r_agents) if tr.live else None), ph.Network(m_agents)
        for u, v in pairs:
            if tr.live:
                rnet.add_connection(u, v)
            mnet.add_connection(u, v)
    if rng.rand() < 0.5:
        leaders = [f"S{i}" for i in rng.permutation(L)]
        followers = [f"B{i}" for i in rng.permutation(Fw)]
    else:                                                  # arbitrary lists: any agent on either side, or on none
        leaders, followers = [], []
        allids = [f"S{i}" for i in range(L)] + [f"B{i}" for i in range(Fw)]
        for aid_ in [allids[i] for i in rng.permutation(len(allids))]:
            if rng.rand() < 0.1:
                continue
            (leaders if rng.rand() < (0.7 if aid_.startswith("S") else 0.2) else followers).append(aid_)
    renv = rph.StackelbergEnv(num_steps, rnet, leaders, followers) if tr.live else None
    menv = ph.StackelbergEnv(num_steps, mnet, leaders, followers)
    spec = menv.spec
    o = OracleEnv(spec)
    sidx = {spec.agent_ids[a]: s for s, a in enumerate(spec.strategic_idx)}
    Ss = spec.n_strategic
    need_reset = True
    for t in range(T):
        if need_reset:
            if tr.live:
                robs, _ = renv.reset()
            conn = None
            if stochastic:
                conn = tr.take("conn", lambda: np.asarray([rnet.graph.has_edge(u, v) for u, v in pairs], np.uint8))[None]
            oobs, ovalid = o.reset(None, None, conn)
            present, rvals = (tr.put(n, x) for n, x in zip(("reset_present", "reset_obs"), _keyed_rows(robs, sidx, Ss, 2)[:2])) \
                if tr.live else (tr.get("reset_present"), tr.get("reset_obs"))
            assert (present == ovalid[0]).all(), (case, t, "reset keys")
            for s in np.flatnonzero(present):
                assert np.array_equal(f32_bits(rvals[s]), f32_bits(oobs[0, s, :2])), (case, t, "reset obs", s)
            need_reset = False
        odd = bool(tr.take("odd", lambda: (renv.current_step + 1) % 2 == 1))
        acts, act, valid = {}, np.zeros((1, Ss), np.float32), np.zeros((1, Ss), np.uint8)
        for aid in (leaders if odd else followers):
            if rng.rand() < 0.9:
                a = np.float32(rng.randint(1, 9) / 8.0) if odd else np.float32(rng.randint(0, 4) > 0)
                acts[aid] = np.array([a], np.float32); act[0, sidx[aid]] = a; valid[0, sidx[aid]] = 1
        if tr.live:
            st = renv.step(acts)
            ref = [tr.put(n, x) for n, x in zip(("obs_present", "obs", "obs_len"), _keyed_rows(st.observations, sidx, Ss, 2))]
            ref += [tr.put(n, x) for n, x in zip(("reward_kind", "reward"), _reward_rows(st.rewards, sidx, Ss))]
            all_trunc = tr.put("all_truncated", np.uint8(bool(st.truncations["__all__"])))
            ends = bool(st.truncations["__all__"] or st.terminations["__all__"])
            tr.put("episode_end", np.uint8(ends))
        else:
            ref = [tr.get(n) for n in ("obs_present", "obs", "obs_len", "reward_kind", "reward")]
            all_trunc, ends = tr.get("all_truncated"), bool(tr.get("episode_end"))
        o.step(act, valid, None)
        assert o.err[0] == 0
        _check_step(o, case, t, ref + [None], D_cmp=2, done_keys=False)
        assert all_trunc == o.all_truncated[0], (case, t, "__all__")
        if ends:
            need_reset = True
    return f"stk L={L} Fw={Fw} edges={len(pairs)} stochastic={stochastic} ns={num_steps}"


def run_case(case, trace=None):
    """one case against the live reference (trace None: returns (description, the recorded trace as arrays)) or
    against a recorded trace (returns the description)"""
    rng = np.random.RandomState(case)
    tr = _Trace(trace)
    desc = (market_case if case % 3 == 2 else supply_chain_case)(rng, case, tr)
    return (desc, tr.to_arrays()) if tr.live else desc


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    for case in range(first, first + n):
        try:
            desc, _ = run_case(case)
        except AssertionError as e:
            print("FAIL case", case, e.args, flush=True)
            raise
        if case % 10 == 0:
            print("ok", case, desc, flush=True)
    print("reference fuzz done", n)
