// phx_spec.hip -- the host's reading of a phx_spec (phx_spec.h): validation and the derived tables (derive), the state blob's layout
// (layout), the launch-loop rollout's scratch (gen_scratch) and the generic engine's static round schedule (build_static_schedule).
// Plain host code: no HIP API call, no kernel.
#include "phx_spec.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <unordered_map>

#include "phx_launch.h"

static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}
const char* fail_text() { return g_err; }

static const int GENERIC_LDS_LIMIT = 60 * 1024;

static bool kind_is_strategic(int k) {
  return k == PHX_KIND_SHOP || k == PHX_KIND_SELLER || k == PHX_KIND_BUYER || k == PHX_KIND_MOCK_STRAT ||
         k == PHX_KIND_ADVERTISER;
}
static int kind_obs_dim(int k) {
  switch (k) { case PHX_KIND_SHOP: return 3; case PHX_KIND_SELLER: case PHX_KIND_BUYER: return 2;
               case PHX_KIND_MOCK_STRAT: return 1; case PHX_KIND_ADVERTISER: return 3; default: return 0; }
}

// phx_spec.variant_step == PHX_VS_GENERIC and variant_rollout == PHX_VR_LAUNCH_LOOP select the message-passing engine like PHX_F_FORCE_GENERIC
static uint32_t eff_flags(const phx_spec* sp) {
  return sp->flags | ((sp->variant_step == PHX_VS_GENERIC || sp->variant_step == PHX_VS_GENERIC_DYNAMIC || sp->variant_rollout == PHX_VR_LAUNCH_LOOP) ? PHX_F_FORCE_GENERIC : 0u);
}

static bool has_edge(const phx_spec* sp, int u, int v) {
  for (int k = sp->row_ptr[u]; k < sp->row_ptr[u + 1]; ++k) if (sp->col[k] == v) return true;
  return false;
}

// ---- derive(), step by step: each returns PHX_OK or the failure ------------------------------------------------------------------
static int check_header_and_tables(const phx_spec* sp, Derived& d) {
  const int A = sp->n_agents;
  if (sp->abi_version != PHX_ABI_VERSION) return fail(PHX_EINVAL, "abi_version %d != %d", sp->abi_version, PHX_ABI_VERSION);
  if (sp->flags & PHX_F_SHUFFLE_BATCHES) {                    // resolvers.py:150-151
    if (sp->flags & PHX_F_IGNORE_CONN_ERRORS) return fail(PHX_EUNSUPPORTED, "shuffle_batches with ignore_connection_errors");
    for (int a = 0; a < sp->n_agents; ++a)
      if (sp->kind && sp->kind[a] == PHX_KIND_ADEXCHANGE) return fail(PHX_EUNSUPPORTED, "shuffle_batches with an AdExchangeAgent (its handle_batch is order sensitive in ties)");
  }
  if (sp->n_agents <= 0 || sp->n_agents > 65535) return fail(PHX_EINVAL, "n_agents out of range");
  if (sp->batch <= 0) return fail(PHX_EINVAL, "batch must be positive");
  if (!sp->kind || !sp->param_i || !sp->param_f || !sp->row_ptr || !sp->col) return fail(PHX_EINVAL, "null table");
  if (sp->queue_cap <= 0) return fail(PHX_EINVAL, "queue_cap must be positive");
  // the device RNG counter carries the global env index in 48 bits (bits 48.. hold the redraw attempt)
  if (sp->env_offset < 0 || sp->env_offset + (int64_t)sp->batch > ((int64_t)1 << 48))
    return fail(PHX_EINVAL, "env_offset + batch must stay below 2^48");
  if (sp->n_samplers < 0 || (sp->n_samplers > 0 && (!sp->sampler_kind || !sp->sampler_param)))
    return fail(PHX_EINVAL, "sampler tables missing");
  d.device_sampling = sp->n_samplers > 0;
  for (int j = 0; j < sp->n_samplers; ++j) {
    if (sp->sampler_kind[j] != PHX_SAMPLER_HOST && sp->sampler_kind[j] != PHX_SAMPLER_UNIFORM)
      return fail(PHX_EINVAL, "sampler %d: unknown kind %d", j, sp->sampler_kind[j]);
    if (sp->sampler_kind[j] == PHX_SAMPLER_UNIFORM && !(sp->sampler_param[4 * j + 1] >= sp->sampler_param[4 * j]))
      return fail(PHX_EINVAL, "sampler %d: high < low", j);                       // samplers.py:134
    d.device_sampling = d.device_sampling && sp->sampler_kind[j] == PHX_SAMPLER_UNIFORM;
  }
  if (sp->n_conn < 0 || (sp->n_conn > 0 && (!sp->conn_rate || !sp->col_conn))) return fail(PHX_EINVAL, "StochasticNetwork tables missing");
  bool all_on = true;
  for (int i = 0; i < sp->n_conn; ++i) {
    if (!(sp->conn_rate[i] >= 0.0)) return fail(PHX_EINVAL, "connection %d: bad rate", i);
    all_on = all_on && sp->conn_rate[i] >= 1.0;
  }
  for (int k = 0; k < (sp->n_conn > 0 ? sp->row_ptr[A] : 0); ++k)
    if (sp->col_conn[k] < 0 || sp->col_conn[k] >= sp->n_conn) return fail(PHX_EINVAL, "col_conn out of range");
  d.dynamic_graph = sp->n_conn > 0 && !all_on;
  d.type_src.assign(A, PHX_TYPE_NONE);
  for (int a = 0; a < A && sp->type_src; ++a) {
    const int src = sp->type_src[a];
    if (src == PHX_TYPE_NONE) continue;
    if (src < PHX_TYPE_NONE || src >= sp->n_samplers) return fail(PHX_EINVAL, "agent %d: type_src out of range", a);
    if (sp->kind[a] != PHX_KIND_SHOP && sp->kind[a] != PHX_KIND_ADVERTISER)
      return fail(PHX_EUNSUPPORTED, "agent %d: only ShopAgent / AdvertiserAgent consume a type field on the device", a);
    if (sp->kind[a] == PHX_KIND_SHOP && !(sp->param_f[a * PHX_NPF + 1] != 0.0)) return fail(PHX_EINVAL, "agent %d: type normaliser (pf1) is zero", a);
    d.type_src[a] = src; d.any_typed = d.any_typed || sp->kind[a] == PHX_KIND_SHOP;
  }
  d.A = A; d.nnz = sp->row_ptr[A];
  if (sp->row_ptr[0] != 0) return fail(PHX_EINVAL, "row_ptr[0] != 0");
  for (int a = 0; a < A; ++a) if (sp->row_ptr[a + 1] < sp->row_ptr[a]) return fail(PHX_EINVAL, "row_ptr not monotone");
  for (int k = 0; k < d.nnz; ++k) if (sp->col[k] < 0 || sp->col[k] >= A) return fail(PHX_EINVAL, "col out of range");
  return PHX_OK;
}
// ranks of every agent within its kind, among the strategic agents and among the exogenous columns; the kinds' parameters
static int derive_agents(const phx_spec* sp, Derived& d) {
  const int A = d.A;
  d.strat_rank.assign(A, -1); d.kind_rank.assign(A, 0); d.exo_rank.assign(A, -1); d.buyer_off.assign(A, 0);
  for (int a = 0; a < A; ++a) {
    const int k = sp->kind[a];
    if (k <= 0 || k >= PHX_KIND_COUNT) return fail(PHX_EINVAL, "agent %d: unknown kind %d", a, k);
    d.kind_rank[a] = d.kind_count[k]++;
    if (kind_is_strategic(k)) { d.strat_rank[a] = d.S++; d.strat_idx.push_back(a);
      d.D = std::max(d.D, kind_obs_dim(k) + (k == PHX_KIND_SHOP && d.type_src[a] != PHX_TYPE_NONE ? 1 : 0)); }
    if (k == PHX_KIND_CUSTOMER) d.exo_rank[a] = d.n_exo++;
    if (k == PHX_KIND_PUBLISHER) {                              // user id + pi1 click draws per step
      if (sp->param_i[a * PHX_NPI + 1] < 0 || sp->param_i[a * PHX_NPI + 1] > 4095) return fail(PHX_EINVAL, "agent %d: click draws per step out of range", a);
      d.exo_rank[a] = d.n_exo; d.n_exo += 1 + sp->param_i[a * PHX_NPI + 1];
    }
    if (k == PHX_KIND_BUYER) { d.buyer_off[a] = d.kind_rank[a]; d.buyer_dmax = std::max(d.buyer_dmax, sp->row_ptr[a + 1] - sp->row_ptr[a]); }
    const int32_t* pi = sp->param_i + a * PHX_NPI;
    if ((k == PHX_KIND_SHOP || k == PHX_KIND_CUSTOMER) && (pi[0] < 0 || pi[0] >= A))
      return fail(PHX_EINVAL, "agent %d: target agent index out of range", a);
    if (k == PHX_KIND_SHOP && pi[1] <= 0) return fail(PHX_EINVAL, "agent %d: ShopAgent max_sales_per_step must be > 0", a);
    if (k == PHX_KIND_FORWARDER && pi[0] >= A) return fail(PHX_EINVAL, "agent %d: forward target out of range", a);
    if ((k == PHX_KIND_PUBLISHER || k == PHX_KIND_ADVERTISER || k == PHX_KIND_ADEXCHANGE) && (pi[0] < 0 || pi[0] >= A))
      return fail(PHX_EINVAL, "agent %d: exchange / publisher index out of range", a);
    if (k == PHX_KIND_ADVERTISER && (pi[1] < 0 || pi[1] > 3)) return fail(PHX_EINVAL, "agent %d: theme index must be 0..3", a);
    if (k == PHX_KIND_ADVERTISER && d.type_src[a] == PHX_TYPE_NONE) return fail(PHX_EINVAL, "agent %d: AdvertiserAgent needs a budget (type_src)", a);
    if (k == PHX_KIND_CUSTOMER && sp->kind[pi[0]] != PHX_KIND_SHOP)
      return fail(PHX_EINVAL, "agent %d: CustomerAgent.shop_id is not a ShopAgent", a);
  }
  d.buyer_nnz = d.buyer_dmax * d.kind_count[PHX_KIND_BUYER];   // slot-major (ELL) price table per env
  return PHX_OK;
}
// connections are undirected: every CSR entry u->v has its mirror v->u on the same base connection
static int check_undirected(const phx_spec* sp, Derived& d) {
  const int A = d.A;
  std::unordered_map<uint64_t, int32_t> ent;
  ent.reserve((size_t)d.nnz * 2);
  for (int u = 0; u < A; ++u)
    for (int k = sp->row_ptr[u]; k < sp->row_ptr[u + 1]; ++k)
      if (!ent.emplace(((uint64_t)u << 32) | (uint32_t)sp->col[k], sp->n_conn > 0 ? sp->col_conn[k] : 0).second)
        return fail(PHX_EINVAL, "agent %d: duplicate edge to %d", u, sp->col[k]);
  for (int u = 0; u < A; ++u)
    for (int k = sp->row_ptr[u]; k < sp->row_ptr[u + 1]; ++k) {
      auto it = ent.find(((uint64_t)sp->col[k] << 32) | (uint32_t)u);
      if (it == ent.end() || it->second != (sp->n_conn > 0 ? sp->col_conn[k] : 0))
        return fail(PHX_EINVAL, "edge %d->%d has no mirror edge (connections are undirected, network.py:122-123)", u, sp->col[k]);
    }
  return PHX_OK;
}
// ---- acting lists + masks, per env type ---------------------------------------------------------------------------------------
static int derive_lists_plain(const phx_spec*, Derived& d) {
  const int A = d.A;
  d.n_lists = 1; d.act_ptr = {0, A};
  for (int a = 0; a < A; ++a) d.act_idx.push_back(a);
  d.obs_mask.assign(A, 1); d.rew_mask.assign(A, 1); d.stage_next = {0};
  d.reset_obs_idx = d.strat_idx;                                            // env.py:227
  return PHX_OK;
}
static int derive_lists_fsm(const phx_spec* sp, Derived& d) {
  const int A = d.A, ns = sp->n_stages;
  if (ns <= 0 || !sp->stage_act_ptr || !sp->stage_act_idx || !sp->stage_rewarded || !sp->stage_rewarded_all || !sp->stage_next)
    return fail(PHX_EINVAL, "FSM tables missing");
  if (sp->initial_stage < 0 || sp->initial_stage >= ns) return fail(PHX_EINVAL, "initial_stage out of range");
  d.n_lists = ns;
  d.act_ptr.assign(sp->stage_act_ptr, sp->stage_act_ptr + ns + 1);
  d.act_idx.assign(sp->stage_act_idx, sp->stage_act_idx + sp->stage_act_ptr[ns]);
  for (int v : d.act_idx) if (v < 0 || v >= A) return fail(PHX_EINVAL, "acting agent out of range");
  d.stage_next.assign(sp->stage_next, sp->stage_next + ns);
  d.stage_rew_all.assign(sp->stage_rewarded_all, sp->stage_rewarded_all + ns);
  d.stage_allowed.assign((size_t)ns * ns, 0);                               // fsm.py:304: next_stage in next_stages
  for (int st = 0; st < ns; ++st)
    for (int nx = 0; nx < ns; ++nx)
      d.stage_allowed[(size_t)st * ns + nx] = sp->stage_allowed ? (sp->stage_allowed[(size_t)st * ns + nx] != 0) : (nx == sp->stage_next[st]);
  if (sp->stage_tab) {                                                      // tabulated clock / stage handlers (ABI 6)
    d.stage_tab.assign(sp->stage_tab, sp->stage_tab + (size_t)ns * (sp->num_steps + 1));
    for (int st = 0; st < ns; ++st)
      for (int t = 0; t <= sp->num_steps; ++t) {
        const int nx = d.stage_tab[(size_t)st * (sp->num_steps + 1) + t];
        if (nx < 0 || nx >= ns || !d.stage_allowed[(size_t)st * ns + nx])
          return fail(PHX_EINVAL, "stage_tab[%d][%d] = %d is not one of the stage's next_stages (fsm.py:304-307)", st, t, nx);
      }
  }
  d.obs_mask.assign((size_t)ns * A, 0); d.rew_mask.assign((size_t)ns * A, 0);
  for (int st = 0; st < ns; ++st) {
    const int nx = sp->stage_next[st];
    if (nx < 0 || nx >= ns) return fail(PHX_EINVAL, "stage_next out of range");
    if (sp->stage_rewarded_all[st]) {                                       // fsm.py:315-317
      for (int a = 0; a < A; ++a) d.obs_mask[(size_t)st * A + a] = d.rew_mask[(size_t)st * A + a] = 1;
    } else {                                                                // fsm.py:319-320
      for (int a = 0; a < A; ++a) d.rew_mask[(size_t)st * A + a] = sp->stage_rewarded[(size_t)st * A + a];
      for (int k = sp->stage_act_ptr[nx]; k < sp->stage_act_ptr[nx + 1]; ++k)
        d.obs_mask[(size_t)st * A + sp->stage_act_idx[k]] = 1;
    }
  }
  const int i0 = sp->initial_stage;                                         // fsm.py:237-241
  for (int k = sp->stage_act_ptr[i0]; k < sp->stage_act_ptr[i0 + 1]; ++k) d.reset_obs_idx.push_back(sp->stage_act_idx[k]);
  return PHX_OK;
}
static int derive_lists_stackelberg(const phx_spec* sp, Derived& d) {
  const int A = d.A;
  if ((sp->n_leaders && !sp->leaders) || (sp->n_followers && !sp->followers)) return fail(PHX_EINVAL, "leader/follower lists missing");
  d.n_lists = 2; d.act_ptr = {0, sp->n_leaders, sp->n_leaders + sp->n_followers};
  d.obs_mask.assign((size_t)2 * A, 0); d.rew_mask.assign((size_t)2 * A, 0); d.stage_next = {0, 0};
  for (int k = 0; k < sp->n_leaders; ++k) {
    const int a = sp->leaders[k]; if (a < 0 || a >= A) return fail(PHX_EINVAL, "leader out of range");
    d.act_idx.push_back(a); d.rew_mask[a] = 1; d.obs_mask[(size_t)A + a] = 1; d.reset_obs_idx.push_back(a);
  }
  for (int k = 0; k < sp->n_followers; ++k) {
    const int a = sp->followers[k]; if (a < 0 || a >= A) return fail(PHX_EINVAL, "follower out of range");
    d.act_idx.push_back(a); d.obs_mask[a] = 1; d.rew_mask[(size_t)A + a] = 1;
  }
  return PHX_OK;
}
static int derive_lists(const phx_spec* sp, Derived& d) {
  int rc;
  if (sp->env_type == PHX_ENV_PLAIN) rc = derive_lists_plain(sp, d);
  else if (sp->env_type == PHX_ENV_FSM) rc = derive_lists_fsm(sp, d);
  else if (sp->env_type == PHX_ENV_STACKELBERG) rc = derive_lists_stackelberg(sp, d);
  else return fail(PHX_EINVAL, "unknown env_type %d", sp->env_type);
  if (rc != PHX_OK) return rc;
  const int A = d.A;
  d.act_mask.assign((size_t)d.n_lists * A, 0);
  int longest = 0;
  for (int l = 0; l < d.n_lists; ++l) {
    longest = std::max(longest, d.act_ptr[l + 1] - d.act_ptr[l]);
    for (int k = d.act_ptr[l]; k < d.act_ptr[l + 1]; ++k) d.act_mask[(size_t)l * A + d.act_idx[k]] = 1;
  }
  d.scan_cap = std::max(sp->queue_cap, longest + PHX_MAX_INJECT);
  return PHX_OK;
}
// device-evaluated state handlers (ABI 9): what can be checked before the state layout exists
static int derive_stage_rules(const phx_spec* sp, Derived& d) {
  if (sp->n_stage_rules < 0 || (sp->n_stage_rules > 0 && !sp->stage_rules)) return fail(PHX_EINVAL, "stage_rules: bad count / NULL table");
  if (sp->n_stage_rules == 0) return PHX_OK;
  if (sp->env_type != PHX_ENV_FSM) return fail(PHX_EINVAL, "stage_rules need a FiniteStateMachineEnv");
  const int ns = sp->n_stages;
  d.stage_has_rules.assign((size_t)ns, 0);
  for (int r = 0; r < sp->n_stage_rules; ++r) {
    const phx_stage_rule& q = sp->stage_rules[r];
    if (q.stage < 0 || q.stage >= ns || q.next_stage < 0 || q.next_stage >= ns) return fail(PHX_EINVAL, "stage_rules[%d]: stage out of range", r);
    if (!d.stage_allowed[(size_t)q.stage * ns + q.next_stage]) return fail(PHX_EINVAL, "stage_rules[%d]: %d is not one of stage %d's next_stages (fsm.py:304-307)", r, q.next_stage, q.stage);
    if (q.cmp < PHX_CMP_LT || q.cmp > PHX_CMP_NE) return fail(PHX_EINVAL, "stage_rules[%d]: unknown comparison", r);
    if (!(q.threshold == q.threshold)) return fail(PHX_EINVAL, "stage_rules[%d]: NaN threshold", r);
    d.stage_has_rules[q.stage] = 1;
  }
  if (sp->stage_tab)
    for (int st = 0; st < ns; ++st)
      if (d.stage_has_rules[st])
        for (int t = 0; t <= sp->num_steps; ++t)
          if (sp->stage_tab[(size_t)st * (sp->num_steps + 1) + t] != sp->stage_next[st]) return fail(PHX_EINVAL, "stage %d has both rules and a tabulated handler", st);
  return PHX_OK;
}
// ---- which fused schedule serves the spec? ------------------------------------------------------------------------------------
// What every fused kernel asks of a spec: the message-passing engine is not forced, batches are not shuffled, no message trace,
// and the round limit leaves room for the `rounds` rounds of the kernel's step.  Each classifier adds its own terms.
static bool fused_may_serve(const phx_spec* sp, int rounds) {
  return !(eff_flags(sp) & (PHX_F_FORCE_GENERIC | PHX_F_SHUFFLE_BATCHES)) && sp->trace_cap == 0 && (sp->round_limit < 0 || sp->round_limit >= rounds);
}
// the supply chain's topology: every shop talks to a factory, every customer to its shop, nothing else
static bool sc_topology(const phx_spec* sp) {
  for (int a = 0; a < sp->n_agents; ++a) {
    const int k = sp->kind[a]; const int32_t* pi = sp->param_i + a * PHX_NPI;
    if (k == PHX_KIND_SHOP) { if (!(sp->kind[pi[0]] == PHX_KIND_FACTORY && has_edge(sp, a, pi[0]) && has_edge(sp, pi[0], a))) return false; }
    else if (k == PHX_KIND_CUSTOMER) { if (!(has_edge(sp, a, pi[0]) && has_edge(sp, pi[0], a))) return false; }
    else if (k != PHX_KIND_FACTORY) return false;
  }
  return true;
}
static int classify_sc(const phx_spec* sp, Derived& d) {
  const int nS = d.kind_count[PHX_KIND_SHOP];
  const bool fits = nS > 0 && nS <= 256 && fused_may_serve(sp, 2) && !(sp->flags & PHX_F_IGNORE_CONN_ERRORS) && !d.dynamic_graph;
  d.sc_static = fits && (sp->env_type == PHX_ENV_PLAIN || sp->env_type == PHX_ENV_FSM) && sp->n_stage_rules == 0 && sc_topology(sp);
  // the same topology with stage handlers in rule form: phx_rollout has a fused loop that evaluates the rules (phx_sc_rollout_fsm_kernel<true>);
  // phx_step / the engine's other entries stay on the message-passing engine
  d.sc_rules_fused = fits && sp->env_type == PHX_ENV_FSM && sp->n_stage_rules > 0 && !d.any_typed && sp->n_samplers == 0 && d.D == 3 &&
                     d.S == nS && sc_topology(sp);
  return PHX_OK;
}
// the fused market kernels' tables: slot-major neighbour table of the buyers (seller ranks), per-agent records and flags
static void derive_stk_tables(const phx_spec* sp, Derived& d) {
  const int A = d.A, nB = d.kind_count[PHX_KIND_BUYER];
  d.stk_nbr.assign((size_t)std::max(d.buyer_dmax, 1) * std::max(nB, 1), 0xFFFF);
  d.stk_nbr_conn.assign(d.stk_nbr.size(), 0);
  for (int a = 0; a < A; ++a)
    if (sp->kind[a] == PHX_KIND_BUYER)
      for (int e = sp->row_ptr[a]; e < sp->row_ptr[a + 1]; ++e) {
        d.stk_nbr[(size_t)(e - sp->row_ptr[a]) * nB + d.kind_rank[a]] = (uint16_t)d.kind_rank[sp->col[e]];
        if (sp->n_conn > 0) d.stk_nbr_conn[(size_t)(e - sp->row_ptr[a]) * nB + d.kind_rank[a]] = sp->col_conn[e];
      }
  d.stk_rec.assign(A, 0); d.stk_flags.assign((size_t)2 * A, 0);
  for (int a = 0; a < A; ++a) {
    // buyers: deg <= buyer_dmax < 256; a seller's degree (its obs divisor) is read from row_ptr
    const int deg = sp->row_ptr[a + 1] - sp->row_ptr[a];
    d.stk_rec[a] = (uint32_t)sp->kind[a] | ((uint32_t)std::min(deg, 255) << 8) | ((uint32_t)d.kind_rank[a] << 16);
    for (int l = 0; l < 2; ++l)
      d.stk_flags[(size_t)l * A + a] = (uint8_t)((d.act_mask[(size_t)l * A + a] ? 1 : 0) | (d.obs_mask[(size_t)l * A + a] ? 2 : 0) |
                                                 (d.rew_mask[(size_t)l * A + a] ? 4 : 0));
  }
  // packed per-agent words of the batched-load kernels (phx_stk_fused.hip)
  d.stk_packed = !d.dynamic_graph && d.buyer_dmax <= 8;
  d.stk_rec2.assign(A, 0); d.stk_agent.assign((size_t)4 * A, 0);
  if (d.stk_packed)
    for (int a = 0; a < A; ++a) {
      const bool seller = sp->kind[a] == PHX_KIND_SELLER;
      const int deg = sp->row_ptr[a + 1] - sp->row_ptr[a];
      d.stk_rec2[a] = (d.stk_rec[a] & 0xffffff00u) | (seller ? 1u : 0u) | ((uint32_t)(d.stk_flags[a] & 7) << 1) |
                      ((uint32_t)(d.stk_flags[(size_t)A + a] & 7) << 4);
      if (seller) d.stk_agent[(size_t)4 * a] = (uint32_t)deg;
      else for (int j = 0; j < deg; ++j)
        d.stk_agent[(size_t)4 * a + (j >> 1)] |= (uint32_t)d.kind_rank[sp->col[sp->row_ptr[a] + j]] << ((j & 1) * 16);
    }
}
static int classify_stk(const phx_spec* sp, Derived& d) {
  const int A = d.A;
  bool stk = sp->env_type == PHX_ENV_STACKELBERG && d.kind_count[PHX_KIND_SELLER] > 0 && fused_may_serve(sp, 1) &&
             !(sp->flags & PHX_F_IGNORE_CONN_ERRORS) && (!d.dynamic_graph || sp->n_samplers == 0);
  for (int a = 0; a < A && stk; ++a) {
    const int k = sp->kind[a];
    if (k != PHX_KIND_SELLER && k != PHX_KIND_BUYER) { stk = false; break; }
    for (int e = sp->row_ptr[a]; e < sp->row_ptr[a + 1] && stk; ++e) {
      const int v = sp->col[e];                    // bipartite, symmetric adjacency
      stk = sp->kind[v] == (k == PHX_KIND_SELLER ? PHX_KIND_BUYER : PHX_KIND_SELLER) && has_edge(sp, v, a);
    }
  }
  d.stk_static = stk && d.kind_count[PHX_KIND_SELLER] < 65535 && d.kind_count[PHX_KIND_BUYER] < 65536 && d.buyer_dmax < 256 && d.S == A && d.D == 2;
  if (d.stk_static) derive_stk_tables(sp, d);
  return PHX_OK;
}
// static digital-ads schedule (phx_ads_fused.hip): the shipped env (digital_ads_market.py:525-596): one exchange, one publisher,
// N advertisers, every connection present, stage P {acting = [publisher]} <-> stage A {acting = the advertisers in agent order}
static int classify_ads(const phx_spec* sp, Derived& d) {
  const int A = d.A, N = d.kind_count[PHX_KIND_ADVERTISER];
  bool ads = sp->env_type == PHX_ENV_FSM && sp->n_stages == 2 && N >= 1 && N <= 1024 && d.kind_count[PHX_KIND_PUBLISHER] == 1 &&
             d.kind_count[PHX_KIND_ADEXCHANGE] == 1 && A == N + 2 && fused_may_serve(sp, 3) &&
             (!d.dynamic_graph || (sp->flags & PHX_F_IGNORE_CONN_ERRORS)) && d.D == 3 &&
             sp->stage_next[0] == 1 && sp->stage_next[1] == 0 && !sp->stage_tab;
  if (ads) {
    for (int a = 0; a < A; ++a) { if (sp->kind[a] == PHX_KIND_PUBLISHER) d.ads_pub = a; if (sp->kind[a] == PHX_KIND_ADEXCHANGE) d.ads_adx = a; }
    const int pub = d.ads_pub, adx = d.ads_adx;
    ads = sp->param_i[pub * PHX_NPI] == adx && sp->param_i[adx * PHX_NPI] == pub && sp->param_i[pub * PHX_NPI + 1] >= 1 &&
          has_edge(sp, pub, adx) && sp->row_ptr[adx + 1] - sp->row_ptr[adx] == N + 1 && sp->row_ptr[pub + 1] - sp->row_ptr[pub] == N + 1;
    for (int a = 0; a < A && ads; ++a)
      if (sp->kind[a] == PHX_KIND_ADVERTISER)
        ads = sp->param_i[a * PHX_NPI] == adx && has_edge(sp, a, adx) && has_edge(sp, a, pub) && sp->row_ptr[a + 1] - sp->row_ptr[a] == 2;
    int ps = -1;                                            // which stage is the publisher's
    for (int l = 0; l < 2 && ads; ++l)
      if (d.act_ptr[l + 1] - d.act_ptr[l] == 1 && d.act_idx[d.act_ptr[l]] == pub) ps = l;
    ads = ads && ps >= 0;
    if (ads) {
      const int l = 1 - ps;
      ads = d.act_ptr[l + 1] - d.act_ptr[l] == N;
      for (int k = 0; k < N && ads; ++k) ads = d.act_idx[d.act_ptr[l] + k] == d.strat_idx[k];
      d.ads_pub_stage = ps;
    }
  }
  d.ads_static = ads;
  return PHX_OK;
}
// ---- per-shop tables of the supply-chain kernels ------------------------------------------------------------------------------
// lookup tables of the rollout kernel: the reference's own formulas evaluated on the host
//   obs   np.float32(x / n)            supply_chain.py:127-134
//   penalty 0.1*stock (f64)            supply_chain.py:147
static void derive_sc_lookup_tables(Derived& d) {
  const int nS = d.kind_count[PHX_KIND_SHOP];
  bool uniform = true;
  for (int s2 = 1; s2 < nS; ++s2) uniform = uniform && d.shop_norm[s2] == d.shop_norm[0];
  const int n_quot = uniform ? std::min(4 * d.max_cust + 1, 512) : 0;   // valid x/norm entries
  d.n_tabn = n_quot; d.n_quot = n_quot;
  d.rew_smax = 0;                                             // penalty table present
  for (int x = 0; x <= 100; ++x) d.sc_tab.push_back((float)((double)x / 100.0));
  for (int x = 0; x < d.n_tabn; ++x) d.sc_tab.push_back((float)((double)x / (double)d.shop_norm[0]));
  if ((d.sc_tab.size() & 1) != 0) d.sc_tab.push_back(0.f);    // 8-byte align the f64 part
  d.n_tabn = (int)d.sc_tab.size() - 101;                       // padded length of the x/norm part
  for (int st = 0; st <= 100; ++st) {                         // 0.1 * stock as f64, two floats each
    volatile double pen = 0.1 * (double)st;
    double pv = pen; float two[2]; memcpy(two, &pv, 8);
    d.sc_tab.push_back(two[0]); d.sc_tab.push_back(two[1]);
  }
}
// per acting list: which customers act, and each shop's flag byte (Derived::sc_shop_flags)
static void derive_shop_flags(Derived& d) {
  const int A = d.A, nS = d.kind_count[PHX_KIND_SHOP];
  d.shop_cust_act.assign((size_t)d.n_lists * std::max(d.n_exo, 1), 0);
  for (int l = 0; l < d.n_lists; ++l)
    for (size_t k = 0; k < d.shop_cust_agent.size(); ++k)
      d.shop_cust_act[(size_t)l * d.n_exo + k] = d.act_mask[(size_t)l * A + d.shop_cust_agent[k]];
  d.sc_shop_flags.assign((size_t)d.n_lists * nS, 0);
  for (int l = 0; l < d.n_lists; ++l)
    for (int s2 = 0; s2 < nS; ++s2) {
      const int a_shop = d.shop_agent[s2];
      bool any = false, all = true;
      for (int k = d.shop_cust_ptr[s2]; k < d.shop_cust_ptr[s2 + 1]; ++k) { const bool on = d.shop_cust_act[(size_t)l * d.n_exo + k] != 0; any |= on; all &= on; }
      d.sc_shop_flags[(size_t)l * nS + s2] = (uint8_t)((d.act_mask[(size_t)l * A + a_shop] ? 1 : 0) | (any ? 2 : 0) | ((any && all) ? 4 : 0) |
                                                       (d.obs_mask[(size_t)l * A + a_shop] ? 8 : 0) | (d.rew_mask[(size_t)l * A + a_shop] ? 16 : 0));
    }
}
static int derive_shop_tables(const phx_spec* sp, Derived& d) {
  const int A = d.A, nS = d.kind_count[PHX_KIND_SHOP];
  if (nS == 0) return PHX_OK;
  d.shop_agent.assign(nS, 0); d.shop_norm.assign(nS, 1);
  d.shop_type_src.assign(nS, PHX_TYPE_NONE); d.shop_type_prm.assign((size_t)2 * nS, 0.0);
  std::vector<std::vector<int>> cust(nS);
  for (int a = 0; a < A; ++a) {
    if (sp->kind[a] == PHX_KIND_SHOP) { d.shop_agent[d.kind_rank[a]] = a; d.shop_norm[d.kind_rank[a]] = sp->param_i[a * PHX_NPI + 1];
      d.shop_type_src[d.kind_rank[a]] = d.type_src[a];
      d.shop_type_prm[2 * d.kind_rank[a]] = sp->param_f[a * PHX_NPF]; d.shop_type_prm[2 * d.kind_rank[a] + 1] = sp->param_f[a * PHX_NPF + 1]; }
    if (sp->kind[a] == PHX_KIND_CUSTOMER) cust[d.kind_rank[sp->param_i[a * PHX_NPI]]].push_back(a);
  }
  d.shop_cust_ptr.push_back(0);
  for (int s = 0; s < nS; ++s) {
    for (int a : cust[s]) { d.shop_cust_agent.push_back(a); d.shop_cust_exo.push_back(d.exo_rank[a]); }
    d.shop_cust_ptr.push_back((int)d.shop_cust_agent.size());
    d.max_cust = std::max(d.max_cust, (int)cust[s].size());
  }
  // device-RNG counter word = shop | customer group << 20 (six customers per group)
  if (d.max_cust > 6 * 4096 || nS > (1 << 20))
    return fail(PHX_EUNSUPPORTED, "at most 24576 customers per shop and 2^20 shops (device RNG counter layout)");
  derive_sc_lookup_tables(d);
  derive_shop_flags(d);
  return PHX_OK;
}

int derive(const phx_spec* sp, Derived& d) {
  if (!sp) return fail(PHX_EINVAL, "null spec");
  typedef int (*Step)(const phx_spec*, Derived&);
  static const Step steps[] = {check_header_and_tables, derive_agents, check_undirected, derive_lists, derive_stage_rules, classify_sc, classify_stk,
                               classify_ads, derive_shop_tables};
  for (Step step : steps) {
    const int rc = step(sp, d);
    if (rc != PHX_OK) return rc;
  }
  return PHX_OK;
}

// ---- scratch of the launch-loop rollout: the outputs of one phx_step for the whole batch ----------------
GenScratch gen_scratch(int64_t B, int64_t S, int64_t D) {
  GenScratch g; int64_t off = 0;
  auto take = [&](int64_t bytes) { const int64_t o = off; off += (bytes + 255) & ~(int64_t)255; return o; };
  g.obs = take(B * S * D * 4); g.reward = take(B * S * 8);
  g.obs_valid = take(B * S); g.reward_valid = take(B * S); g.terminated = take(B * S); g.truncated = take(B * S);
  g.done_valid = take(B * S); g.all_term = take(B); g.all_trunc = take(B); g.done = take(B); g.actions = take(B * S * 4);
  g.total = off;
  return g;
}

// ---- state blob layout ------------------------------------------------------------------------------
int64_t layout(const phx_spec* sp, const Derived& d, std::vector<FieldDef>& out, int64_t* ws_stride) {
  const int64_t B = sp->batch, S = std::max(d.S, 1);
  auto kc = [&](int k) { return (int64_t)std::max(d.kind_count[k], 0); };
  std::vector<FieldDef> f = {
    {F_ENV_STEP, "env.step", 0, 0, B, 1, 1, 0}, {F_ENV_STAGE, "env.stage", 0, 0, B, 1, 1, 0},
    {F_ENV_PREV_STAGE, "env.prev_stage", 0, 0, B, 1, 1, 0}, {F_ENV_TICK, "env.tick", 0, 0, B, 1, 1, 0},
    {F_ENV_CLOCK, "env.clock", 0, 0, B, 1, 1, 0},
    {F_ENV_TERM, "env.term", 2, 0, B, S, 1, 0}, {F_ENV_TRUNC, "env.trunc", 2, 0, B, S, 1, 0},
    {F_ENV_REW_CACHE, "env.rew_cache", 1, 0, B, S, 1, 0}, {F_ENV_REW_CACHE_VALID, "env.rew_cache_valid", 2, 0, B, S, 1, 0},
    {F_ENV_OBS_CACHE, "env.obs_cache", 3, 0, B, S, d.D, 0}, {F_ENV_OBS_CACHE_VALID, "env.obs_cache_valid", 2, 0, B, S, 1, 0},
    {F_ENV_SAMPLER, "env.sampler", 1, 0, B, sp->n_samplers, 1, 0}, {F_ENV_EPISODE, "env.episode", 0, 0, B, (sp->n_samplers > 0 || sp->n_conn > 0) ? 1 : 0, 1, 0},
    {F_NET_CONN_ON, "net.conn_on", 2, 0, B, sp->n_conn, 1, 0},
    {F_ENV_ARRIVE, "env.arrive", 0, 0, B, d.sc_static ? 1 : 0, 1, 0},
    {F_ENV_MT_STATE, "env.mt_state", 0, 0, B, (sp->flags & PHX_F_MT19937) ? 624 : 0, 1, 0},
    {F_ENV_MT_POS, "env.mt_pos", 0, 0, B, (sp->flags & PHX_F_MT19937) ? 1 : 0, 1, 0},
    {F_SHOP_STOCK, "shop.stock", 0, PHX_KIND_SHOP, B, kc(PHX_KIND_SHOP), 1, 0},
    {F_SHOP_SALES, "shop.sales", 0, PHX_KIND_SHOP, B, kc(PHX_KIND_SHOP), 1, 0},
    {F_SHOP_MISSED, "shop.missed_sales", 0, PHX_KIND_SHOP, B, kc(PHX_KIND_SHOP), 1, 0},
    {F_SHOP_DELIVERED, "shop.delivered_stock", 0, PHX_KIND_SHOP, B, kc(PHX_KIND_SHOP), 1, 0},
    {F_SELLER_PRICE, "seller.price", 1, PHX_KIND_SELLER, B, kc(PHX_KIND_SELLER), 1, 0},
    {F_SELLER_REVENUE, "seller.revenue", 1, PHX_KIND_SELLER, B, kc(PHX_KIND_SELLER), 1, 0},
    {F_SELLER_TX, "seller.tx", 0, PHX_KIND_SELLER, B, kc(PHX_KIND_SELLER), 1, 0},
    {F_SELLER_POSTED, "seller.posted", 1, PHX_KIND_SELLER, B, kc(PHX_KIND_SELLER), 1, 0},
    {F_BUYER_PRICES, "buyer.prices", 1, PHX_KIND_BUYER, B, d.buyer_dmax, kc(PHX_KIND_BUYER), 0},
    {F_BUYER_PAID, "buyer.paid", 1, PHX_KIND_BUYER, B, kc(PHX_KIND_BUYER), 1, 0},
    {F_BUYER_BOUGHT, "buyer.bought", 0, PHX_KIND_BUYER, B, kc(PHX_KIND_BUYER), 1, 0},
    {F_CASHBOX_TOTAL, "cashbox.total_cash", 1, PHX_KIND_CASHBOX, B, kc(PHX_KIND_CASHBOX), 1, 0},
    {F_REQRESP_REQ, "reqresp.req_time", 0, PHX_KIND_REQRESP, B, kc(PHX_KIND_REQRESP), 1, 0},
    {F_REQRESP_RES, "reqresp.res_time", 0, PHX_KIND_REQRESP, B, kc(PHX_KIND_REQRESP), 1, 0},
    {F_MOCK_ENC, "mock.encode_obs_count", 0, PHX_KIND_MOCK_STRAT, B, kc(PHX_KIND_MOCK_STRAT), 1, 0},
    {F_MOCK_DEC, "mock.decode_action_count", 0, PHX_KIND_MOCK_STRAT, B, kc(PHX_KIND_MOCK_STRAT), 1, 0},
    {F_MOCK_REW, "mock.compute_reward_count", 0, PHX_KIND_MOCK_STRAT, B, kc(PHX_KIND_MOCK_STRAT), 1, 0},
    {F_ADV_LEFT, "adv.left", 1, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_BID, "adv.bid", 1, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_LEFT_TAG, "adv.left_tag", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_BID_TAG, "adv.bid_tag", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_CLICKS, "adv.step_clicks", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_WINS, "adv.step_wins", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_USER, "adv.user", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 1, 0},
    {F_ADV_TOT_CLICKS, "adv.total_clicks", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 3, 0},
    {F_ADV_TOT_REQUESTS, "adv.total_requests", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 3, 0},
    {F_ADV_TOT_WINS, "adv.total_wins", 0, PHX_KIND_ADVERTISER, B, kc(PHX_KIND_ADVERTISER), 3, 0},
    {F_PUB_ADS_SEEN, "pub.ads_seen", 0, PHX_KIND_PUBLISHER, B, kc(PHX_KIND_PUBLISHER), 1, 0},
  };
  int64_t off = 0;
  out.clear();
  for (auto& x : f) {
    const int64_t n = x.dim0 * x.dim1 * x.dim2;
    if (n == 0) continue;
    x.offset = off;
    off += (n * esize(x.dtype) + 255) & ~(int64_t)255;
    out.push_back(x);
  }
  // workspace of the generic engine when its queues do not fit LDS
  int n_adx_spec = 0;
  for (int a = 0; a < d.A; ++a) n_adx_spec += sp->kind[a] == PHX_KIND_ADEXCHANGE;
  const size_t qb = phx_generic_queue_bytes(d.A, d.S, sp->queue_cap, d.scan_cap, n_adx_spec);
  *ws_stride = 0;
  if (lean_lds_spec(sp, d)) {
    // scheduled two-wave supply chains: the sort / scan scratch of a DYNAMIC step lives here instead of LDS (phx_generic.hip, LEAN)
    *ws_stride = ((int64_t)phx_generic_lean_ws_bytes(sp->queue_cap, d.scan_cap) + 255) & ~(int64_t)255;
    FieldDef w = {F_WORKSPACE, "workspace", 2, 0, B, *ws_stride, 1, off};
    off += B * *ws_stride;
    out.push_back(w);
  } else if (qb > (size_t)GENERIC_LDS_LIMIT) {
    *ws_stride = ((int64_t)qb + 255) & ~(int64_t)255;
    FieldDef w = {F_WORKSPACE, "workspace", 2, 0, B, *ws_stride, 1, off};
    off += B * *ws_stride;
    out.push_back(w);
  }
  // step-shaped scratch of the launch-loop rollout (envs without a fused rollout kernel)
  // (a market too large for the LDS-resident rollout kernel falls back to the generic engine's loop as well)
  const int64_t stk_nS = d.kind_count[PHX_KIND_SELLER], stk_nB = d.kind_count[PHX_KIND_BUYER];
  // NOTE: an estimate of its own, not phx_stk_rollout_lds() (phx_stk_fused.hip), which phx_rollout tests: a market of one seller and roughly
  // 2400-3072 buyers passes here (no rollout.scratch) and fails there -- it is refused, not sent to the generic engine.  Kept as is; to be reconciled.
  const bool stk_big = d.stk_static && (d.A > 3 * 1024 ||
                                        8 * (3 * stk_nS + d.A + stk_nB) + 9 * stk_nS + d.A + stk_nB + sp->n_conn + 32 > 60 * 1024);
  if ((!d.sc_static && !d.stk_static) || stk_big) {       // (the fused ads kernels keep it: injected sends fall back to the loop)
    const int64_t n = gen_scratch(B, S, d.D).total;
    FieldDef r = {F_ROLLOUT_SCRATCH, "rollout.scratch", 2, 0, 1, n, 1, off};
    off += n;
    out.push_back(r);
  }
  return std::max<int64_t>(off, 256);
}

// ---- static round schedule of the generic engine --------------------------------------------
// For specs whose message flow cannot drop or add a message -- static Network, no ignore_connection_errors, no shuffle, only
// the supply-chain kinds (every send and every reply is unconditional: supply_chain.py:40-45,55-67,98-122,136-142) and the mock
// kinds that never send -- the rounds of a step in which every agent has a context and every acting ShopAgent an action are the
// same for every env and every step: which message sits where in which inbox (resolvers.py:128-158 -- receivers in first-arrival
// order, batches in send order, replies in handling order).  Simulated here per acting list; the kernel checks the premise per env
// and step and otherwise runs its atomics / scan / rank sort as before.
void build_static_schedule(const phx_spec* sp, const Derived& d, StaticSched& out) {
  const int A = d.A;
  out.blob.clear(); out.off.assign(d.n_lists, -1);
  if ((sp->flags & (PHX_F_SHUFFLE_BATCHES | PHX_F_IGNORE_CONN_ERRORS)) || d.dynamic_graph) return;
  for (int a = 0; a < A; ++a) {
    const int k = sp->kind[a];
    if (k != PHX_KIND_FACTORY && k != PHX_KIND_SHOP && k != PHX_KIND_CUSTOMER && k != PHX_KIND_MOCK_STRAT && k != PHX_KIND_MOCK_AGENT) return;
  }
  auto payload_ok = [&](int src, int dst, int type) {
    if (sp->flags & PHX_F_NO_PAYLOAD_CHECKS) return true;
    int sk = 0, rk = 0;
    switch (type) {
      case PHX_MSG_ORDER_REQUEST: sk = PHX_KIND_CUSTOMER; rk = PHX_KIND_SHOP; break;
      case PHX_MSG_ORDER_RESPONSE: sk = PHX_KIND_SHOP; rk = PHX_KIND_CUSTOMER; break;
      case PHX_MSG_STOCK_REQUEST: sk = PHX_KIND_SHOP; rk = PHX_KIND_FACTORY; break;
      case PHX_MSG_STOCK_RESPONSE: sk = PHX_KIND_FACTORY; rk = PHX_KIND_SHOP; break;
      default: return false;
    }
    return sp->kind[src] == sk && sp->kind[dst] == rk;
  };
  struct M { int src, dst, type; };
  for (int l = 0; l < d.n_lists; ++l) {
    std::vector<M> q;
    std::vector<int32_t> act_off;                                // queue offset of each acting item's message, -1: sends nothing
    bool ok = true;
    for (int k = d.act_ptr[l]; k < d.act_ptr[l + 1] && ok; ++k) {
      const int a = d.act_idx[k], kind = sp->kind[a], dst = sp->param_i[a * PHX_NPI];
      if (kind == PHX_KIND_SHOP || kind == PHX_KIND_CUSTOMER) {
        const int type = kind == PHX_KIND_SHOP ? PHX_MSG_STOCK_REQUEST : PHX_MSG_ORDER_REQUEST;
        ok = dst >= 0 && dst < A && has_edge(sp, a, dst) && payload_ok(a, dst, type);
        act_off.push_back((int32_t)q.size());
        q.push_back({a, dst, type});
      } else act_off.push_back(-1);
    }
    if (!ok || (int)q.size() > sp->queue_cap) continue;
    std::vector<int32_t> rec(1 + PHX_SCHED_MAX_ROUNDS, 0);
    rec.insert(rec.end(), act_off.begin(), act_off.end());
    int R = 0;
    while (!q.empty() && ok) {
      if (R == PHX_SCHED_MAX_ROUNDS || (sp->round_limit >= 0 && R >= sp->round_limit)) { ok = false; break; }
      const int n = (int)q.size();
      std::vector<int32_t> cnt(A, 0), first(A, 0x7fffffff), goff(A, 0), order(n, 0), fill(A, 0);
      for (int i = 0; i < n; ++i) { cnt[q[i].dst]++; first[q[i].dst] = std::min(first[q[i].dst], i); }
      int run = 0;
      for (int i = 0; i < n; ++i) if (first[q[i].dst] == i) { goff[q[i].dst] = run; run += cnt[q[i].dst]; }   // dict order of receivers
      for (int i = 0; i < n; ++i) order[goff[q[i].dst] + fill[q[i].dst]++] = i;                               // batches in send order
      std::vector<M> nq;
      std::vector<int32_t> next_off(n, -1);                       // where the reply to inbox position P goes in the next queue
      for (int P = 0; P < n && ok; ++P) {                       // replies in handling order
        const M m = q[order[P]];
        const int rk = sp->kind[m.dst];
        if (rk == PHX_KIND_FACTORY && m.type == PHX_MSG_STOCK_REQUEST) {
          ok = payload_ok(m.dst, m.src, PHX_MSG_STOCK_RESPONSE); next_off[P] = (int32_t)nq.size(); nq.push_back({m.dst, m.src, PHX_MSG_STOCK_RESPONSE});
        } else if (rk == PHX_KIND_SHOP && m.type == PHX_MSG_ORDER_REQUEST) {
          ok = payload_ok(m.dst, m.src, PHX_MSG_ORDER_RESPONSE); next_off[P] = (int32_t)nq.size(); nq.push_back({m.dst, m.src, PHX_MSG_ORDER_RESPONSE});
        } else if ((rk == PHX_KIND_SHOP && m.type == PHX_MSG_STOCK_RESPONSE) || (rk == PHX_KIND_CUSTOMER && m.type == PHX_MSG_ORDER_RESPONSE)) {
        } else ok = false;                                        // no handler: the dynamic path reports it
      }
      if ((int)nq.size() > sp->queue_cap) ok = false;
      rec[1 + R] = n;
      rec.insert(rec.end(), cnt.begin(), cnt.end()); rec.insert(rec.end(), goff.begin(), goff.end()); rec.insert(rec.end(), order.begin(), order.end());
      rec.insert(rec.end(), next_off.begin(), next_off.end());
      ++R; q.swap(nq);
    }
    if (!ok) continue;
    rec[0] = R;
    out.off[l] = (int32_t)out.blob.size();
    out.blob.insert(out.blob.end(), rec.begin(), rec.end());
  }
}

// LEAN layout of the generic engine (phx_generic.hip): every acting list of a two-wave supply chain has a static schedule ->
// the sort / scan scratch only a dynamic step needs (order, slot, scanbuf) moves from LDS to a per-env workspace in the blob
bool lean_lds_spec(const phx_spec* sp, const Derived& d) {
  if (d.sc_static) return false;                 // the fused kernels serve this spec: the generic engine is its rare fallback (phx_inject / phx_resolve,
                                                 // the split FSM step) and gets no schedule (DevSpec::sched) -- it keeps the plain layout
  if (d.A <= 64 || d.A > 256) return false;
  for (int a = 0; a < d.A; ++a) { const int k = sp->kind[a]; if (k != PHX_KIND_FACTORY && k != PHX_KIND_SHOP && k != PHX_KIND_CUSTOMER) return false; }
  if (phx_generic_queue_bytes(d.A, d.S, sp->queue_cap, d.scan_cap, 0, true) > (size_t)GENERIC_LDS_LIMIT) return false;
  StaticSched ss;
  build_static_schedule(sp, d, ss);
  if (ss.blob.empty()) return false;
  for (int l = 0; l < d.n_lists; ++l) if (ss.off[l] < 0) return false;
  return true;
}
