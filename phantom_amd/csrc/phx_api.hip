// phx_api.hip -- the C ABI of include/phantom_amd.h: the handle (phx_create builds it in stages from what phx_spec.hip derived),
// table upload and kernel dispatch.  No torch types cross this boundary; the caller owns the state
// blob and every I/O buffer, the library owns only its copy of the static spec tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "phx_launch.h"
#include "phx_spec.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return fail(PHX_EHIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

// ---- handle ----------------------------------------------------------------------------------------------
struct phx_env {
  DevSpec d;
  Derived der;
  std::vector<FieldDef> fields;
  std::vector<void*> dev_allocs;
  int device = 0;
  bool use_fused = false, use_stk = false, use_ads = false, lds_ok = true;
  bool sc_rules_fused = false;      // rule-form FSM supply chain: phx_rollout takes phx_sc_rollout_fsm_kernel<true>
  bool prices_compressed = false;   // buyer.prices is represented by seller.posted (fused Stackelberg kernel)
  std::atomic<int32_t> fsm_gen{0};  // launch generation of the time-parallel FSM rollout (DevSpec::fsm_gen_host)
  int32_t sw_guard_gen = 0;         // number of the last replayed-actions call on the store-wave kernel (DevSpec::sc_sw_guard)
  DevMsg* inject_dev = nullptr;
  DevMsg inject_host[PHX_MAX_INJECT];
  int n_inject = 0;
  // PHX_VR_AUTO by measurement (FSM supply chains): the kernel chosen for a (T, n_frag) shape on THIS box, 0 = the store-wave
  // instantiation, 1 = the lane-per-pair chain; the state blob's copy the probe launches start from and restore
  void* state_blob = nullptr; int64_t state_nbytes = 0;
  void* probe_snapshot = nullptr;
  std::unordered_map<uint64_t, int> fsm_auto;
  std::string fsm_auto_note;        // "T=400: store-wave 861.2 us, loop 772.4 us -> loop" (phx_last_error's sibling: phx_autotune_note)
};

// a failing step ends the calling function with the step's code (its text is already in fail_text())
#define TRY(x) do { const int rc_ = (x); if (rc_ != PHX_OK) return rc_; } while (0)

// a host table's copy in device memory, owned by the handle (freed by phx_destroy); n == 0 still yields a valid pointer
template <typename T, typename U>
static int upload(phx_env* e, const T* host, size_t n, U** out) {
  static_assert(std::is_same<typename std::remove_const<U>::type, T>::value, "the device pointer has the host table's element type");
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  HIPCHK(hipMalloc(&p, bytes));
  e->dev_allocs.push_back(p);
  if (n) HIPCHK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  *out = (U*)p;
  return PHX_OK;
}
// the one way phx_create's stages upload: UP(pointer lvalue, host table, elements)
#define UP(dst, ptr, n) TRY(upload(e, ptr, (size_t)(n), &(dst)))

// ---- phx_create, stage by stage: each fills its part of e->d from (spec, der) and returns PHX_OK or the failure ------------------
static int create_spec_tables(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  const int A = der.A;
  d.A = der.A; d.S = der.S; d.B = spec->batch; d.D = der.D; d.n_exo = der.n_exo; d.nnz = der.nnz;
  d.num_steps = spec->num_steps; d.round_limit = spec->round_limit; d.env_type = spec->env_type;
  d.flags = spec->flags; d.queue_cap = spec->queue_cap; d.trace_cap = spec->trace_cap; d.scan_cap = der.scan_cap;
  d.n_lists = der.n_lists; d.initial_stage = spec->initial_stage; d.buyer_nnz = der.buyer_nnz; d.buyer_stride = der.kind_count[PHX_KIND_BUYER];
  d.seed = spec->seed; d.env_offset = spec->env_offset;
  d.variant_rollout = spec->variant_rollout; d.variant_block = spec->variant_block; d.variant_step = spec->variant_step;
  d.policy_mfma = d.variant_rollout == PHX_VR_POLICY_MFMA;             // (a policy-kernel choice: every other path sees PHX_VR_AUTO)
  if (d.policy_mfma) d.variant_rollout = PHX_VR_AUTO;
  memcpy(d.kind_count, der.kind_count, sizeof d.kind_count);
  d.n_reset_obs = (int)der.reset_obs_idx.size(); d.n_conn = spec->n_conn; d.stk_packed = der.stk_packed ? 1 : 0;
  d.dynamic_graph = der.dynamic_graph ? 1 : 0;
  d.n_samplers = spec->n_samplers; d.any_typed = der.any_typed ? 1 : 0; d.device_sampling = der.device_sampling ? 1 : 0;
  d.n_tabn = der.n_tabn; d.n_quot = der.n_quot; d.rew_smax = der.rew_smax; d.max_cust = der.max_cust;
  d.ads_pub = der.ads_pub; d.ads_adx = der.ads_adx; d.ads_pub_stage = der.ads_pub_stage;
  d.sc_all_or_none = 1;
  for (size_t i = 0; i < der.sc_shop_flags.size(); ++i) if ((der.sc_shop_flags[i] & 2) && !(der.sc_shop_flags[i] & 4)) d.sc_all_or_none = 0;

  UP(d.kind, spec->kind, A); UP(d.param_i, spec->param_i, A * PHX_NPI); UP(d.param_f, spec->param_f, A * PHX_NPF);
  UP(d.row_ptr, spec->row_ptr, A + 1); UP(d.col, spec->col, der.nnz);
  UP(d.strat_rank, der.strat_rank.data(), A); UP(d.strat_idx, der.strat_idx.data(), der.strat_idx.size());
  UP(d.kind_rank, der.kind_rank.data(), A); UP(d.exo_rank, der.exo_rank.data(), A); UP(d.buyer_off, der.buyer_off.data(), A);
  UP(d.act_ptr, der.act_ptr.data(), der.act_ptr.size()); UP(d.act_idx, der.act_idx.data(), der.act_idx.size());
  UP(d.act_mask, der.act_mask.data(), der.act_mask.size());
  UP(d.obs_mask, der.obs_mask.data(), der.obs_mask.size()); UP(d.rew_mask, der.rew_mask.data(), der.rew_mask.size());
  UP(d.stage_next, der.stage_next.data(), der.stage_next.size());
  if (spec->flags & PHX_F_MT19937) {                            // the draw sequence of every acting list (phx_mt_draw)
    std::vector<int32_t> mp = {0}, mr;
    for (int l = 0; l < der.n_lists; ++l) {
      for (int k = der.act_ptr[l]; k < der.act_ptr[l + 1]; ++k) { const int r = der.exo_rank[der.act_idx[k]]; if (r >= 0) mr.push_back(r); }
      mp.push_back((int32_t)mr.size());
    }
    UP(d.mt_ptr, mp.data(), mp.size()); UP(d.mt_rank, mr.data(), mr.size());
  }
  UP(d.stage_allowed, der.stage_allowed.data(), der.stage_allowed.size());
  if (!der.stage_tab.empty()) UP(d.stage_tab, der.stage_tab.data(), der.stage_tab.size());
  UP(d.stage_rew_all, der.stage_rew_all.data(), der.stage_rew_all.size()); UP(d.reset_obs_idx, der.reset_obs_idx.data(), der.reset_obs_idx.size());
  UP(d.shop_agent, der.shop_agent.data(), der.shop_agent.size()); UP(d.shop_norm, der.shop_norm.data(), der.shop_norm.size());
  UP(d.shop_cust_ptr, der.shop_cust_ptr.data(), der.shop_cust_ptr.size()); UP(d.shop_cust_exo, der.shop_cust_exo.data(), der.shop_cust_exo.size());
  UP(d.shop_cust_agent, der.shop_cust_agent.data(), der.shop_cust_agent.size()); UP(d.shop_cust_act, der.shop_cust_act.data(), der.shop_cust_act.size());
  UP(d.sc_shop_flags, der.sc_shop_flags.data(), der.sc_shop_flags.size()); UP(d.sc_tab, der.sc_tab.data(), der.sc_tab.size());
  UP(d.conn_rate, spec->conn_rate, spec->n_conn); UP(d.col_conn, spec->col_conn, spec->n_conn > 0 ? der.nnz : 0);
  UP(d.stk_nbr, der.stk_nbr.data(), der.stk_nbr.size()); UP(d.stk_nbr_conn, der.stk_nbr_conn.data(), der.stk_nbr_conn.size());
  UP(d.stk_rec, der.stk_rec.data(), der.stk_rec.size()); UP(d.stk_flags, der.stk_flags.data(), der.stk_flags.size());
  UP(d.stk_rec2, der.stk_rec2.data(), der.stk_rec2.size()); UP(d.stk_agent, der.stk_agent.data(), der.stk_agent.size());
  UP(d.sampler_kind, spec->sampler_kind, spec->n_samplers); UP(d.sampler_param, spec->sampler_param, 4 * spec->n_samplers);
  UP(d.type_src, der.type_src.data(), A); UP(d.shop_type_src, der.shop_type_src.data(), der.shop_type_src.size()); UP(d.shop_type_prm, der.shop_type_prm.data(), der.shop_type_prm.size());
  return PHX_OK;
}
static const FieldDef* find_field_by_name(const phx_env* e, const char* name) {
  for (const FieldDef& f : e->fields) if (!strcmp(f.name, name)) return &f;
  return nullptr;
}
// the stage rules' fields by name: per-agent i32 / f64 state of one kind
static int create_stage_rules(const phx_spec* spec, const Derived&, phx_env* e) {
  DevSpec& d = e->d;
  if (spec->n_stage_rules <= 0) return PHX_OK;
  std::vector<DevRule> rl;
  for (int r = 0; r < spec->n_stage_rules; ++r) {
    const phx_stage_rule& q = spec->stage_rules[r];
    char nm[33]; memcpy(nm, q.field, 32); nm[32] = 0;
    const FieldDef* f = find_field_by_name(e, nm);
    if (!f || f->kind <= 0 || (f->dtype != 0 && f->dtype != 1) || f->dim2 != 1 || f->dim1 < 1)
      return fail(PHX_EINVAL, "stage_rules[%d]: '%s' is not a per-agent i32 / f64 state field", r, nm);
    if (q.agent < -1 || q.agent >= f->dim1) return fail(PHX_EINVAL, "stage_rules[%d]: agent column %d outside the %lld agents of '%s'", r, q.agent, (long long)f->dim1, nm);
    DevRule dr; dr.stage = q.stage; dr.field_id = f->id; dr.col = q.agent; dr.ncols = (int32_t)f->dim1; dr.cmp = q.cmp; dr.next_stage = q.next_stage;
    dr.is_f64 = f->dtype == 1; dr.pad = 0; dr.threshold = q.threshold;
    rl.push_back(dr);
  }
  UP(d.rules, rl.data(), rl.size());
  d.n_rules = (int32_t)rl.size();
  return PHX_OK;
}
// specs the generic engine serves: its static round schedule and, where the flow is the supply chain's, the same schedule COMPILED
// for the several-envs-per-wave kernel (phx_generic_sched.hip)
static int create_generic_schedule(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  if (der.sc_static || der.stk_static || der.ads_static) return PHX_OK;
  StaticSched ss;
  build_static_schedule(spec, der, ss);
  if (ss.blob.empty()) return PHX_OK;
  UP(d.sched, ss.blob.data(), ss.blob.size()); UP(d.sched_off, ss.off.data(), ss.off.size());
  bool sched_every_list = true;
  for (int l = 0; l < der.n_lists; ++l) sched_every_list = sched_every_list && ss.off[l] >= 0;
  if (!(sched_every_list && der.D == 3 && !der.any_typed)) return PHX_OK;
  std::vector<int32_t> gblob, grecs; int gL = 0, gq = 0;
  if (!phx_sched_compile(spec, der.A, der.n_lists, der.act_ptr.data(), der.act_idx.data(), der.act_mask.data(), der.obs_mask.data(), der.rew_mask.data(),
                         der.kind_rank.data(), der.exo_rank.data(), der.strat_rank.data(), der.reset_obs_idx.data(), (int)der.reset_obs_idx.size(),
                         &gblob, &grecs, &gL, &gq)) return PHX_OK;
  int qstride = gq + 1;
  while ((qstride & 31) != 9) ++qstride;                    // (the env instances of a wave start their queues 9 banks apart)
  if (der.n_lists < 65536 && phx_sched_lds_bytes((int)gblob.size(), gL, qstride, d.n_rules, der.n_lists) <= 48 * 1024 &&
      phx_generic_queue_bytes(der.A, der.S, spec->queue_cap, der.scan_cap, 0, false) <= 48 * 1024) {      // (the tail workgroups run the dynamic engine in LDS)
    UP(d.gs_blob, gblob.data(), gblob.size());
    if (grecs.empty()) grecs.assign(2, 0);
    UP(d.gs_rec, grecs.data(), grecs.size());
    std::vector<int32_t> zf((size_t)d.B, 0);
    UP(d.gs_dyn_flag, zf.data(), zf.size());
    d.gs_ok = 1; d.gs_L = gL; d.gs_qstride = qstride; d.gs_words = (int32_t)gblob.size();
  }
  return PHX_OK;
}
// phx_generic_step_kernel's LDS table layout, packed, and the ad exchanges' advertiser edges
static int create_generic_tables(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  const int A = der.A;
  std::vector<char> blob(phx_generic_table_bytes(A, der.nnz), 0);
  char* tb = blob.data();
  auto put = [&](const void* src, size_t bytes) { if (bytes) memcpy(tb, src, bytes); tb += (bytes + 15) & ~(size_t)15; };
  put(spec->row_ptr, (size_t)(A + 1) * 4); put(spec->col, (size_t)der.nnz * 4); put(spec->param_i, (size_t)A * PHX_NPI * 4);
  put(der.strat_rank.data(), (size_t)A * 4); put(der.kind_rank.data(), (size_t)A * 4); put(der.exo_rank.data(), (size_t)A * 4);
  put(spec->kind, (size_t)A);
  d.tab_bytes = (int32_t)blob.size();
  UP(d.tab_blob, blob.data(), blob.size());
  std::vector<int32_t> adx;
  for (int a = 0; a < A; ++a) if (spec->kind[a] == PHX_KIND_ADEXCHANGE) adx.push_back(a);
  d.n_adx = (int32_t)adx.size();
  UP(d.adx_idx, adx.data(), adx.size());
  std::vector<int32_t> nptr = {0}, ne;
  for (int a : adx) {
    for (int k = spec->row_ptr[a]; k < spec->row_ptr[a + 1]; ++k) if (spec->kind[spec->col[k]] == PHX_KIND_ADVERTISER) ne.push_back(k);
    nptr.push_back((int32_t)ne.size());
  }
  UP(d.adx_nbr_ptr, nptr.data(), nptr.size()); UP(d.adx_nbr_e, ne.data(), ne.size());
  return PHX_OK;
}
// ---- what the supply-chain plans ask of the shops ---------------------------------------------------------------------------------
struct ShopShape { int K; bool norm_uniform; };      // K: customers per shop where every shop has the same number, else -1
static ShopShape shop_shape(const Derived& der, int S) {
  ShopShape sh = {der.shop_cust_ptr.size() > 1 ? der.shop_cust_ptr[1] - der.shop_cust_ptr[0] : -1, true};
  for (int s2 = 0; s2 < S; ++s2) {
    if (der.shop_cust_ptr[s2 + 1] - der.shop_cust_ptr[s2] != sh.K) sh.K = -1;
    sh.norm_uniform = sh.norm_uniform && der.shop_norm[s2] == der.shop_norm[0];
  }
  return sh;
}
// a stage's flags (Derived::sc_shop_flags) are the same for every shop
static bool stage_flags_uniform(const Derived& der, int n_lists, int S) {
  for (int l = 0; l < n_lists; ++l)
    for (int s2 = 1; s2 < S; ++s2) if (der.sc_shop_flags[(size_t)l * S + s2] != der.sc_shop_flags[(size_t)l * S]) return false;
  return true;
}
// the handler-less stage chain from the initial stage: visit(p, stage, the stage's flags) for the episode positions p = 0 .. ns - 1;
// false when the chain leaves the stages
template <typename F>
static bool walk_stage_chain(const phx_spec* spec, const Derived& der, const DevSpec& d, F visit) {
  int sg = spec->initial_stage;
  for (int p = 0; p < d.num_steps; ++p) {
    if (sg < 0 || sg >= d.n_lists) return false;
    visit(p, sg, (int)der.sc_shop_flags[(size_t)sg * d.S]);
    sg = spec->stage_next[sg];
  }
  return true;
}
// a store-wave plan was accepted: build the kernel's table image, upload it, and keep the plan in *dst
static int accept_sw_plan(phx_env* e, ScSwPlan sw, int norm, ScSwPlan* dst) {
  sw.norm = norm;
  std::vector<uint8_t> img;
  phx_sc_sw_tables(sw.K, sw.norm, &img);
  const uint8_t* dev_img = nullptr;
  UP(dev_img, img.data(), img.size());
  e->d.sc_sw_tables = dev_img;
  *dst = sw;
  return PHX_OK;
}
// time-parallel FSM rollout (phx_sc_rollout_fsm.hip): the env has no samplers, and along the handler-less chain from the initial stage
// every lookback the kernel serves from its tiles is at most PHX_FSM_LB steps.  The table holds, per episode position, the flags, the
// lookbacks and the stage.
static int plan_fsm_fast(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  if (!(spec->n_samplers == 0 && d.num_steps >= PHX_FAST_TC && d.num_steps <= 4096 && d.n_lists <= 255)) return PHX_OK;
  const int ns = d.num_steps, LB = PHX_FSM_LB;
  std::vector<int> stage(ns), fl(ns);
  if (!walk_stage_chain(spec, der, d, [&](int p, int sg, int f) { stage[p] = sg; fl[p] = f; })) return PHX_OK;
  std::vector<uint32_t> fsm_tab(ns, 0);       // position table
  auto back_in_episode = [&](int p, int bit) { for (int k = 0; k <= p; ++k) if (fl[p - k] & bit) return k; return -1; };
  auto back_cyclic = [&](int p, int bit, bool* same_episode) {
    for (int k = 0; k <= LB; ++k) { const int q = p - k; if (fl[((q % ns) + ns) % ns] & bit) { *same_episode = q >= 0; return k; } }
    *same_episode = false; return -1;
  };
  for (int p = 0; p < ns; ++p) {
    const int f = fl[p];
    uint32_t w = (uint32_t)((f & 1) | ((f & 2) ? 2 : 0) | ((f & 8) ? 4 : 0) | ((f & 16) ? 8 : 0));
    const bool emits = (f & 8) || p == ns - 1;               // the shop observes, or the episode ends: a reward is emitted
    const int lr = back_in_episode(p, 16), lo = back_in_episode(p, 8);
    if (emits && lr > LB) return PHX_OK;
    if (p == ns - 1 && lo != 0) return PHX_OK;                 // the episode's last step observes (no dump of an older observation)
    w |= (uint32_t)((lr < 0 || lr > LB) ? 7 : lr) << 4;
    w |= (uint32_t)((lo < 0 || lo > LB) ? 7 : lo) << 8;
    bool se = false, dummy = false;
    const int cr = back_cyclic(p, 16, &se), co = back_cyclic(p, 8, &dummy), ca = back_cyclic(p, 1, &dummy);
    if (cr < 0 || co < 0 || ca < 0) return PHX_OK;             // the state left behind must be in reach from every position
    w |= (uint32_t)cr << 12; w |= (uint32_t)(se ? 1 : 0) << 15;
    w |= (uint32_t)co << 16; w |= (uint32_t)ca << 20;
    w |= (uint32_t)stage[p] << 24;
    fsm_tab[p] = w;
  }
  ScFastPlan plan;
  if (!phx_sc_fast_plan(d.B, d.S, d.fsm_lean_K, true, d.num_steps, d.variant_block, false, &plan)) return PHX_OK;
  plan.norm = d.fsm_lean_norm; d.fsm_fast = plan;
  UP(d.fsm_pos_tab, fsm_tab.data(), fsm_tab.size());
  return PHX_OK;
}
// the store-wave kernel's FSM instantiation (phx_sc_rollout_sw.hip, MODE 2) for the same envs: per episode position along the
// handler-less chain the stage's flags and whether a rewarded position lies at or before it; the episode's last position observes
// (its terminal dump, fsm.py:360-375, is then the row's own observation).  No lookback limit: the recurrence lanes carry fsm.py's caches.
static int plan_fsm_sw(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  if (!(spec->n_samplers == 0 && d.num_steps >= 16 && d.num_steps <= 4096 && d.n_lists <= 255 &&
        (d.variant_rollout == PHX_VR_AUTO || d.variant_rollout == PHX_VR_STORE_WAVES))) return PHX_OK;
  const int ns = d.num_steps;
  std::vector<uint16_t> tab((size_t)2 * ns, 0);
  bool has_rew = false;
  if (!walk_stage_chain(spec, der, d, [&](int p, int sg, int f) {
        has_rew = has_rew || (f & 16);
        // (the SWF_* word of phx_sc_rollout_sw.hip: operand masks and flags at the tile word's bits)
        tab[p] = (uint16_t)(((f & 1) ? 0x407F : 0) | ((f & 2) ? 0x1F00 : 0) | ((f & 8) ? 0x0080 : 0) | ((f & 16) ? 0x2000 : 0) | (has_rew ? 0x8000 : 0));
        tab[ns + p] = (uint16_t)sg;
      })) return PHX_OK;
  if (!(tab[ns - 1] & 0x0080)) return PHX_OK;
  // the state a fragment leaves (delivered_stock, self._rewards, self._observations) is tracked over its last two chunks: the acting /
  // rewarded / observing positions of the (cyclic) chain lie at most 16 steps apart, or never occur
  for (uint16_t bit : {(uint16_t)0x4000, (uint16_t)0x2000, (uint16_t)0x0080}) {
    int first = -1, prev = -1, gap = 0;
    for (int p = 0; p < ns; ++p) if (tab[p] & bit) { if (first < 0) first = p; else gap = std::max(gap, p - prev); prev = p; }
    if (first >= 0) gap = std::max(gap, first + ns - prev);
    if (gap > 16) return PHX_OK;
  }
  ScSwPlan sw;
  if (phx_sc_sw_plan(d.B, d.S, d.fsm_lean_K, true, ns, d.variant_block, &sw, ns) && (sw.specialised || d.variant_rollout == PHX_VR_STORE_WAVES) && sw.G != 144) {
    TRY(accept_sw_plan(e, sw, d.fsm_lean_norm, &d.fsm_sw));
    UP(d.fsm_sw_tab, tab.data(), tab.size());
  }
  return PHX_OK;
}
// FSM supply chains on the fused schedule: the lean lane-per-pair loop, the time-parallel kernel, the store-wave kernel
static int create_fsm_sc_plans(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  if (!(der.sc_static && spec->env_type == PHX_ENV_FSM && !der.any_typed && d.S > 0 && d.D == 3)) return PHX_OK;
  // lean FSM rollout loop: every shop with the same 1..6 customers and normaliser, a shop's customers act all or none per stage
  // (tabulated handlers: the general lane-per-pair loop looks every transition up; the lean loop, the time-parallel and the store-wave
  //  kernel are built on the handler-less stage chain)
  const ShopShape sh = shop_shape(der, d.S);
  if (!(sh.norm_uniform && d.sc_all_or_none && sh.K >= 1 && sh.K <= 6 && der.shop_norm[0] > 0 && !spec->stage_tab)) return PHX_OK;
  d.fsm_lean_K = sh.K; d.fsm_lean_norm = der.shop_norm[0];
  // the time-parallel and the store-wave kernel: additionally the stage's flags are the same for every shop
  if (!stage_flags_uniform(der, d.n_lists, d.S)) return PHX_OK;
  TRY(plan_fsm_fast(spec, der, e));
  TRY(plan_fsm_sw(spec, der, e));
  if (d.fsm_fast.ok || d.fsm_sw.ok) {
    const int32_t zero = 0;
    UP(d.fsm_irregular, &zero, 1);
    d.fsm_gen_host = &e->fsm_gen;
  }
  return PHX_OK;
}
// plain supply chains on the fused schedule: the wide step kernel, the time-parallel rollout kernel (phx_sc_rollout.hip), the store-wave
// kernel and its replay words
static int create_plain_sc_plans(const phx_spec* spec, const Derived& der, phx_env* e) {
  DevSpec& d = e->d;
  if (!(der.sc_static && spec->env_type == PHX_ENV_PLAIN && !der.any_typed && d.S > 0)) return PHX_OK;
  const ShopShape sh = shop_shape(der, d.S);      // the fast kernels: every shop with the same 1..6 customers and the same normaliser
  // four-pairs-per-thread step kernel (large batches): additionally every shop acts and every customer orders in the env's one list
  bool all_act = d.n_lists == 1;
  for (int s2 = 0; s2 < d.S && all_act; ++s2) all_act = (der.sc_shop_flags[s2] & 7) == 7;
  if (all_act && sh.K >= 1 && sh.K <= 6 && sh.norm_uniform && der.shop_norm[0] > 0 && d.D == 3 && ((int64_t)d.B * d.S) % 4 == 0) { d.sc_wide_K = sh.K; d.sc_wide_norm = der.shop_norm[0]; }
  ScFastPlan plan;
  if (phx_sc_fast_plan(d.B, d.S, sh.K, sh.norm_uniform, d.num_steps, d.variant_block, true, &plan)) {
    plan.norm = der.shop_norm[0];
    d.sc_fast = plan;
  }
  // the store-wave kernel serves the same envs (planes only) where a 16-pair-aligned workgroup shape exists;
  // variant_rollout PHX_VR_TIME_PARALLEL keeps the time-parallel kernel, PHX_VR_STORE_WAVES / PHX_VR_AUTO take this one
  ScSwPlan sw;
  if (!(d.sc_fast.ok && (d.variant_rollout == PHX_VR_AUTO || d.variant_rollout == PHX_VR_STORE_WAVES) &&
        phx_sc_sw_plan(d.B, d.S, sh.K, sh.norm_uniform, d.num_steps, d.variant_block, &sw) && (sw.specialised || d.variant_rollout == PHX_VR_STORE_WAVES)))
    return PHX_OK;
  TRY(accept_sw_plan(e, sw, der.shop_norm[0], &d.sc_sw));
  // replays (REPLAY instantiation): the exogenous column of each shop's first customer where its customers' columns are consecutive
  // (they are for every env the host layer builds: customers are numbered shop by shop), and the pre-scan's device word
  std::vector<int32_t> first((size_t)d.S, 0);
  bool consecutive = true;
  for (int s2 = 0; s2 < d.S; ++s2) {
    const int c0 = der.shop_cust_ptr[s2];
    first[s2] = der.shop_cust_exo[c0];
    for (int k = 0; k < sh.K; ++k) consecutive = consecutive && der.shop_cust_exo[c0 + k] == first[s2] + k;
  }
  if (consecutive) UP(d.sc_sw_exo_first, first.data(), first.size());
  const int32_t zero = 0;
  UP(d.sc_sw_guard, &zero, 1);
  return PHX_OK;
}
// binds the fields to the caller's blob, puts the finished spec in device memory and brings the blob to the constructor's state
static int bind_blob_and_reset(const phx_spec* spec, const Derived& der, phx_env* e, void* state_blob, int64_t need, int64_t ws_stride) {
  DevSpec& d = e->d;
  e->state_blob = state_blob; e->state_nbytes = need;
  for (auto& f : e->fields) d.f[f.id] = (char*)state_blob + f.offset;
  d.ws_stride = ws_stride;
  d.lean_lds = lean_lds_spec(spec, der) ? 1 : 0;
  e->lds_ok = ws_stride == 0 || d.lean_lds;
  e->use_fused = der.sc_static;
  e->sc_rules_fused = der.sc_rules_fused && d.n_rules > 0 && SC_RULES_MAX_S >= d.S;
  e->use_stk = der.stk_static;
  e->use_ads = der.ads_static;
  e->prices_compressed = der.stk_static;
  hipError_t he = hipMalloc((void**)&e->inject_dev, sizeof(DevMsg) * PHX_MAX_INJECT);
  if (he != hipSuccess) return fail(PHX_EHIP, "hipMalloc: %s", hipGetErrorString(he));
  {                                   // the finished spec in device memory (DevSpec::self_dev)
    void* p = nullptr;
    he = hipMalloc(&p, sizeof(DevSpec));
    if (he != hipSuccess) return fail(PHX_EHIP, "hipMalloc: %s", hipGetErrorString(he));
    e->dev_allocs.push_back(p);
    d.self_dev = (const DevSpec*)p;
    he = hipMemcpy(p, &d, sizeof(DevSpec), hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(PHX_EHIP, "hipMemcpy: %s", hipGetErrorString(he));
  }
  // constructor state: zero blob, then Agent.reset() for every agent (env.py:122-124)
  he = hipMemset(state_blob, 0, (size_t)need);
  if (he != hipSuccess) return fail(PHX_EHIP, "hipMemset: %s", hipGetErrorString(he));
  if (d.env_type == PHX_ENV_FSM) {
    std::vector<int32_t> st((size_t)d.B, spec->initial_stage), pv((size_t)d.B, -1);
    (void)hipMemcpy(d.f[F_ENV_STAGE], st.data(), st.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d.f[F_ENV_PREV_STAGE], pv.data(), pv.size() * 4, hipMemcpyHostToDevice);
  }
  he = phx_launch_reset(d, nullptr, nullptr, nullptr, nullptr, nullptr, 0);   // also the constructor's first draws, env.py:118-119, network.py:389
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(PHX_EHIP, "initial reset: %s", hipGetErrorString(he));
  return PHX_OK;
}

static thread_local char g_kernels[384] = "";
void phx_note_reset() { g_kernels[0] = 0; }
static void note_reset() { phx_note_reset(); }
void phx_note_kernel(const char* name) {
  const size_t n = strlen(g_kernels), m = strlen(name);
  if (strstr(g_kernels, name) || n + m + 2 >= sizeof g_kernels) return;
  if (n) { g_kernels[n] = '+'; memcpy(g_kernels + n + 1, name, m + 1); } else memcpy(g_kernels, name, m + 1);
}

extern "C" {

// the process-wide switches: the only environment variables the library reads, here and nowhere else (first use: phx_create)
extern "C++" const PhxSwitches& phx_switches() {
  static const PhxSwitches sw = [] {
    auto rd = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    PhxSwitches k;
    k.autotune = rd("PHX_AUTOTUNE", 1);
    k.generic_sched = rd("PHX_GENERIC_SCHED", 1);
    return k;
  }();
  return sw;
}

int phx_abi_version(void) { return PHX_ABI_VERSION; }
const char* phx_last_error(void) { return fail_text(); }

const char* phx_last_kernel(void) { return g_kernels; }

int64_t phx_state_nbytes(const phx_spec* spec) {
  Derived d; if (derive(spec, d) != PHX_OK) return -1;
  std::vector<FieldDef> f; int64_t ws;
  return layout(spec, d, f, &ws);
}
int phx_obs_dim(const phx_spec* spec) { Derived d; return derive(spec, d) == PHX_OK ? d.D : -1; }
int phx_n_strategic(const phx_spec* spec) { Derived d; return derive(spec, d) == PHX_OK ? d.S : -1; }
int phx_n_exo(const phx_spec* spec) { Derived d; return derive(spec, d) == PHX_OK ? d.n_exo : -1; }

int phx_create(const phx_spec* spec, int device, void* state_blob, int64_t state_nbytes, phx_env** out) {
  if (!out) return fail(PHX_EINVAL, "null out");
  *out = nullptr;
  (void)phx_switches();                                 // the environment is read here, once per process
  std::unique_ptr<phx_env, void (*)(phx_env*)> guard(new phx_env(), phx_destroy);      // every early return below frees the handle
  phx_env* e = guard.get();
  TRY(derive(spec, e->der));
  const Derived& der = e->der;
  int64_t ws_stride = 0;
  const int64_t need = layout(spec, der, e->fields, &ws_stride);
  if (!state_blob || state_nbytes < need) return fail(PHX_EINVAL, "state blob too small: %lld < %lld", (long long)state_nbytes, (long long)need);
  if (((uintptr_t)state_blob & 255) != 0) return fail(PHX_EINVAL, "state blob must be 256-byte aligned");
  e->device = device;
  const hipError_t he = hipSetDevice(device);
  if (he != hipSuccess) return fail(PHX_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(he));
  memset(&e->d, 0, sizeof e->d);
  TRY(create_spec_tables(spec, der, e));
  TRY(create_stage_rules(spec, der, e));
  TRY(create_generic_schedule(spec, der, e));
  TRY(create_generic_tables(spec, der, e));
  TRY(create_fsm_sc_plans(spec, der, e));
  TRY(create_plain_sc_plans(spec, der, e));
  TRY(bind_blob_and_reset(spec, der, e, state_blob, need, ws_stride));
  *out = guard.release();
  return PHX_OK;
}

void phx_destroy(phx_env* e) {
  if (!e) return;
  for (void* p : e->dev_allocs) (void)hipFree(p);
  if (e->inject_dev) (void)hipFree(e->inject_dev);
  if (e->probe_snapshot) (void)hipFree(e->probe_snapshot);
  delete e;
}

int phx_n_fields(const phx_env* e) { return e ? (int)e->fields.size() : 0; }

int phx_field_info(const phx_env* e, int index, phx_field* out) {
  if (!e || !out || index < 0 || index >= (int)e->fields.size()) return fail(PHX_EINVAL, "bad field index");
  const FieldDef& f = e->fields[index];
  memset(out, 0, sizeof *out);
  out->field_id = f.id; out->dtype = f.dtype; out->offset = f.offset;
  out->dim0 = (int32_t)f.dim0; out->dim1 = (int32_t)f.dim1; out->dim2 = (int32_t)f.dim2; out->kind = f.kind;
  strncpy(out->name, f.name, sizeof(out->name) - 1);
  return PHX_OK;
}

const char* phx_autotune_note(const phx_env* e) { return e ? e->fsm_auto_note.c_str() : ""; }
int phx_uses_fused(const phx_env* e) { return e && (e->use_fused || e->use_stk || e->use_ads) ? 1 : 0; }


// the handle's device becomes the calling thread's current device (a no-op when it already is)
static inline hipError_t use_device(const phx_env* e) {
  int cur = -1;
  hipError_t r = hipGetDevice(&cur);
  if (r != hipSuccess) return r;
  return cur == e->device ? hipSuccess : hipSetDevice(e->device);
}

// materialise the price table the fused market kernel keeps compressed and leave that kernel: the env stays on the generic engine from here on
static int leave_stk(phx_env* e, hipStream_t st) {
  if (!e->prices_compressed) return PHX_OK;
  HIPCHK(phx_launch_stk_materialise(e->d, st));
  e->prices_compressed = false; e->use_stk = false;
  return PHX_OK;
}

// the pending injected messages go to the device; inject_host is free again when this returns
static int flush_inject(phx_env* e, hipStream_t st) {
  if (e->n_inject > 0) {
    HIPCHK(hipMemcpyAsync(e->inject_dev, e->inject_host, sizeof(DevMsg) * e->n_inject, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));   // inject_host is reused right after
  }
  e->n_inject = 0;
  return PHX_OK;
}

// fragment f of a fragment list as a plain rollout io of Tf steps (the replayed inputs and the message log stay the call's)
static phx_rollout_io frag_io(const phx_rollout_io& io, int f, int Tf) {
  const phx_rollout_frag& fr = io.frags[f];
  phx_rollout_io sub = io;
  sub.n_frag = 0; sub.frags = nullptr; sub.T = Tf;
  sub.obs = fr.obs; sub.action_out = fr.action_out; sub.reward = fr.reward; sub.terminated = fr.terminated; sub.truncated = fr.truncated;
  sub.obs_valid = fr.obs_valid; sub.reward_valid = fr.reward_valid;
  return sub;
}

int phx_sync_fields(phx_env* e, void* stream) {
  if (!e) return fail(PHX_EINVAL, "null env");
  if (!e->prices_compressed) return PHX_OK;
  HIPCHK(use_device(e));
  HIPCHK(phx_launch_stk_materialise(e->d, (hipStream_t)stream));
  return PHX_OK;
}

int phx_reset(phx_env* e, const uint8_t* reset_mask, const double* sampler_values, const uint8_t* conn_on, float* obs,
              uint8_t* obs_valid, void* stream) {
  if (!e) return fail(PHX_EINVAL, "null env");
  if (sampler_values && e->d.n_samplers == 0) return fail(PHX_EINVAL, "sampler_values given but the spec has no samplers");
  if (conn_on && e->d.n_conn == 0) return fail(PHX_EINVAL, "conn_on given but the spec is not a StochasticNetwork");
  HIPCHK(use_device(e));
  HIPCHK(phx_launch_reset(e->d, reset_mask, sampler_values, conn_on, obs, obs_valid, (hipStream_t)stream));
  return PHX_OK;
}

static int check_step_io(const phx_env* e, const phx_step_io* io) {
  if (!io) return fail(PHX_EINVAL, "null io");
  if (e->d.S > 0 && !io->actions && !io->action_valid) return fail(PHX_EINVAL, "actions is NULL");
  if (!io->obs || !io->obs_valid || !io->reward || !io->reward_valid || !io->terminated || !io->truncated ||
      !io->done_valid || !io->all_terminated || !io->all_truncated)
    return fail(PHX_EINVAL, "a required output pointer is NULL");
  // obs rows leave as 16-byte pieces, rewards as f64; the actions are read one f32 per strategic agent by every step
  // kernel, so a row slice actions[t] of a [n, B, S] tensor is fine whatever B * S is
  if (((uintptr_t)io->obs & 15u) != 0 || ((uintptr_t)io->reward & 7u) != 0 || ((uintptr_t)io->actions & 3u) != 0)
    return fail(PHX_EINVAL, "phx_step: obs must be 16-byte aligned, reward 8-byte aligned, actions 4-byte aligned");
  if ((io->msg_log || io->msg_count) && e->d.trace_cap <= 0) return fail(PHX_EINVAL, "msg_log given but trace_cap == 0");
  if (io->shuffle && !(e->d.flags & PHX_F_SHUFFLE_BATCHES)) return fail(PHX_EINVAL, "shuffle given but the spec has no PHX_F_SHUFFLE_BATCHES");
  if (io->next_stage && e->d.env_type != PHX_ENV_FSM) return fail(PHX_EINVAL, "next_stage given but the env is not a FiniteStateMachineEnv");
  return PHX_OK;
}

int phx_step(phx_env* e, const phx_step_io* io, void* stream) {
  note_reset();
  if (!e) return fail(PHX_EINVAL, "null env");
  HIPCHK(use_device(e));
  TRY(check_step_io(e, io));
  hipStream_t st = (hipStream_t)stream;
  if (e->use_fused && e->n_inject == 0 && !io->next_stage) {       // handler-chosen transitions: generic engine
    HIPCHK(phx_launch_sc_step(e->d, *io, st));
    return PHX_OK;
  }
  if (e->use_stk && e->n_inject == 0) {
    HIPCHK(phx_launch_stk_step(e->d, *io, st));
    return PHX_OK;
  }
  if (e->use_ads && e->n_inject == 0 && !io->msg_log && !io->msg_count && !io->next_stage) {
    HIPCHK(phx_launch_ads_step(e->d, *io, st));
    return PHX_OK;
  }
  TRY(leave_stk(e, st));            // host-injected messages can address a single price slot
  GenArgs g; memset(&g, 0, sizeof g); g.io = *io; g.inject = e->inject_dev; g.n_inject = e->n_inject; g.resolve_only = 0; g.roll_t = -1;
  TRY(flush_inject(e, st));
  HIPCHK(phx_launch_generic(e->d, g, e->lds_ok, st));
  return PHX_OK;
}

// The two halves of a step around a HOST-side stage handler that reads agent state (fsm.py:275-307): phx_step_begin runs the acting
// phase and resolve_network() (message log included) and leaves the env's clock words alone; the caller's handler then looks at
// the resolved state and picks the next stage; phx_step_end(io->next_stage) makes the transition and computes observations, rewards
// and done flags.  begin + end == phx_step(io->next_stage).  Always the generic engine (the fused kernels do not split).
static int step_half(phx_env* e, const phx_step_io* io, void* stream, int phase) {
  note_reset();
  if (!e) return fail(PHX_EINVAL, "null env");
  HIPCHK(use_device(e));
  TRY(check_step_io(e, io));
  if (phase == 2 && e->n_inject) return fail(PHX_EINVAL, "phx_step_end with injected messages pending (they belong to phx_step_begin)");
  hipStream_t st = (hipStream_t)stream;
  TRY(leave_stk(e, st));
  GenArgs g; memset(&g, 0, sizeof g); g.io = *io; g.inject = e->inject_dev; g.n_inject = phase == 1 ? e->n_inject : 0;
  g.resolve_only = 0; g.phase = phase; g.roll_t = -1;
  if (phase == 1) TRY(flush_inject(e, st));
  HIPCHK(phx_launch_generic(e->d, g, e->lds_ok, st));
  return PHX_OK;
}
int phx_step_begin(phx_env* e, const phx_step_io* io, void* stream) { return step_half(e, io, stream, 1); }
int phx_step_end(phx_env* e, const phx_step_io* io, void* stream) { return step_half(e, io, stream, 2); }

int phx_inject(phx_env* e, const phx_msg_rec* msgs, int n) {
  if (!e || (n > 0 && !msgs)) return fail(PHX_EINVAL, "null argument");
  if (e->n_inject + n > PHX_MAX_INJECT) return fail(PHX_ECAPACITY, "at most %d injected messages per resolve", PHX_MAX_INJECT);
  for (int k = 0; k < n; ++k) {
    if (msgs[k].sender >= e->d.A || msgs[k].receiver >= e->d.A) return fail(PHX_EINVAL, "agent index out of range");
    DevMsg m; m.src = msgs[k].sender; m.dst = msgs[k].receiver; m.type = msgs[k].type; m.pad = msgs[k].round; m.p.i = msgs[k].payload.i;
    e->inject_host[e->n_inject++] = m;
  }
  return PHX_OK;
}

int phx_resolve(phx_env* e, int32_t* err, phx_msg_rec* msg_log, int32_t* msg_count, void* stream) {
  note_reset();
  if (!e) return fail(PHX_EINVAL, "null env");
  if ((msg_log || msg_count) && e->d.trace_cap <= 0) return fail(PHX_EINVAL, "msg_log given but trace_cap == 0");
  HIPCHK(use_device(e));
  hipStream_t st = (hipStream_t)stream;
  TRY(leave_stk(e, st));
  GenArgs g; memset(&g, 0, sizeof g);
  g.io.err = err; g.io.msg_log = msg_log; g.io.msg_count = msg_count;
  g.inject = e->inject_dev; g.n_inject = e->n_inject; g.resolve_only = 1; g.roll_t = -1;
  TRY(flush_inject(e, st));
  HIPCHK(phx_launch_generic(e->d, g, e->lds_ok, st));
  return PHX_OK;
}

static int rollout_impl(phx_env* e, const phx_rollout_io* io, void* stream);

// PHX_VR_AUTO for an FSM supply chain, where the size rule would take the store-wave instantiation (on four boxes of seven
// the lane-per-pair loop was the faster kernel for config 3 and AUTO took the other one): the FIRST call of a (T, n_frag) shape on a handle
// times both -- one warm-up and two timed launches each, from a copy of the state blob that is restored before the call's own launch --
// and the handle keeps the winner for that shape.  Both kernels produce the same bits (tests/test_gpu_fsm_sw.py), the outputs of the
// probe launches are overwritten by the call's own.  Not while a stream is capturing (phx_fsm_sw_serves declines there already).
static bool fsm_auto_applies(phx_env* e, const phx_rollout_io* io, void* stream) {
  if (!phx_switches().autotune || !e->use_fused || e->d.env_type != PHX_ENV_FSM || e->d.variant_rollout != PHX_VR_AUTO || io->policy) return false;
  if (io->n_frag >= 2 && (!io->frags || !io->frags[0].terminated)) return false;
  if (io->n_frag < 2 && (io->frags || !io->obs || !io->terminated)) return false;
  return phx_fsm_sw_serves(e->d, *io, (hipStream_t)stream);
}
struct FsmAutoScope {             // the handle's spec with one candidate forced, for the duration of a call
  phx_env* e; int32_t vr, ok;
  FsmAutoScope(phx_env* e_, int choice) : e(e_), vr(e_->d.variant_rollout), ok(e_->d.fsm_sw.ok) { if (choice == 0) e->d.variant_rollout = PHX_VR_STORE_WAVES; else e->d.fsm_sw.ok = 0; }
  ~FsmAutoScope() { e->d.variant_rollout = vr; e->d.fsm_sw.ok = ok; }
};
static int fsm_auto_probe(phx_env* e, const phx_rollout_io* io, void* stream, int* choice) {
  hipStream_t st = (hipStream_t)stream;
  if (!e->probe_snapshot) HIPCHK(hipMalloc(&e->probe_snapshot, (size_t)e->state_nbytes));
  HIPCHK(hipMemcpyAsync(e->probe_snapshot, e->state_blob, (size_t)e->state_nbytes, hipMemcpyDeviceToDevice, st));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  float us[2] = {0.f, 0.f};
  int rc = PHX_OK;
  for (int c = 0; c < 2 && rc == PHX_OK; ++c) {
    FsmAutoScope scope(e, c);
    rc = rollout_impl(e, io, stream);                                         // warm-up (first-touch of the planes, the code object)
    if (rc == PHX_OK) { (void)hipEventRecord(e0, st); rc = rollout_impl(e, io, stream); }
    if (rc == PHX_OK) rc = rollout_impl(e, io, stream);
    if (rc == PHX_OK) {
      (void)hipEventRecord(e1, st);
      if (hipEventSynchronize(e1) != hipSuccess) rc = fail(PHX_EHIP, "autotune: hipEventSynchronize");
      else { float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1); us[c] = ms * 500.0f; }
    }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  HIPCHK(hipMemcpyAsync(e->state_blob, e->probe_snapshot, (size_t)e->state_nbytes, hipMemcpyDeviceToDevice, st));
  if (rc != PHX_OK) return rc;
  *choice = us[1] < us[0] ? 1 : 0;
  char buf[192];
  snprintf(buf, sizeof buf, "T=%d n_frag=%d: store-wave %.1f us, lane-per-pair chain %.1f us -> %s", io->T, io->n_frag, us[0], us[1], *choice ? "lane-per-pair chain" : "store-wave");
  e->fsm_auto_note = buf;
  return PHX_OK;
}

int phx_rollout(phx_env* e, const phx_rollout_io* io, void* stream) {
  note_reset();
  if (!e || !io) return fail(PHX_EINVAL, "null argument");
  if (io->T > 0 && fsm_auto_applies(e, io, stream)) {
    HIPCHK(use_device(e));
    const uint64_t key = ((uint64_t)(uint32_t)io->T << 8) | (uint64_t)(uint32_t)(io->n_frag & 0xff);
    auto it = e->fsm_auto.find(key);
    int choice = 0;
    if (it != e->fsm_auto.end()) choice = it->second;
    else {
      const int rc = fsm_auto_probe(e, io, stream, &choice);
      if (rc != PHX_OK) return rc;
      e->fsm_auto[key] = choice;
      note_reset();
    }
    FsmAutoScope scope(e, choice);
    return rollout_impl(e, io, stream);
  }
  return rollout_impl(e, io, stream);
}

static int rollout_impl(phx_env* e, const phx_rollout_io* io, void* stream) {
  if (!e || !io) return fail(PHX_EINVAL, "null argument");
  if (e->d.env_type != PHX_ENV_PLAIN && !(io->n_frag >= 2 || io->frags) && (!io->obs_valid || !io->reward_valid))
    return fail(PHX_EINVAL, "FSM / Stackelberg rollouts need obs_valid and reward_valid outputs");
  if ((io->hints & ~(PHX_RH_ACTIONS_IN_DOMAIN | PHX_RH_EXO_IN_DOMAIN)) != 0)
    return fail(PHX_EINVAL, "phx_rollout: unknown hint bits (ABI 9 removed PHX_RH_FLAGS_ZEROED)");
  if (io->explore && !io->policy)
    return fail(PHX_EINVAL, "phx_rollout: `explore` needs `policy` (ABI 7-8's record layout in this slot was removed in ABI 9)");
  if (io->policy && (io->actions || io->n_frag >= 2 || io->frags || io->msg_log || io->msg_count))
    return fail(PHX_EINVAL, "phx_rollout: `policy` excludes replayed actions, fragment lists and message logs");
  if (io->n_frag >= 2 || io->frags) {   // ABI 9: a fragment list
    if (io->n_frag < 2 || io->n_frag > PHX_MAX_FRAGMENTS || !io->frags) return fail(PHX_EINVAL, "phx_rollout: a fragment list needs 2 .. %d fragments and `frags`", PHX_MAX_FRAGMENTS);
    if (io->T <= 0 || io->T % io->n_frag) return fail(PHX_EINVAL, "phx_rollout: T must be a positive multiple of n_frag");
    if (io->obs || io->action_out || io->reward || io->terminated || io->truncated || io->obs_valid || io->reward_valid)
      return fail(PHX_EINVAL, "phx_rollout: with a fragment list the io's own planes must be NULL");
    const bool need_valid = e->d.env_type != PHX_ENV_PLAIN;
    for (int f = 0; f < io->n_frag; ++f) {
      const phx_rollout_frag& fr = io->frags[f];
      if (!fr.obs || !fr.action_out || !fr.reward || !fr.truncated || (need_valid && (!fr.obs_valid || !fr.reward_valid)))
        return fail(PHX_EINVAL, "phx_rollout: fragment %d lacks a required plane", f);
      if ((fr.terminated != nullptr) != (io->frags[0].terminated != nullptr)) return fail(PHX_EINVAL, "phx_rollout: `terminated` must be given for every fragment or for none");
      const void* bufs[] = {fr.obs, fr.action_out, fr.reward, fr.terminated, fr.truncated, fr.obs_valid, fr.reward_valid};
      for (const void* p : bufs) if (((uintptr_t)p & 15u) != 0) return fail(PHX_EINVAL, "phx_rollout: every buffer must be 16-byte aligned");
    }
    if (((uintptr_t)io->last_obs & 15u) || ((uintptr_t)io->actions & 3u)) return fail(PHX_EINVAL, "phx_rollout: every output buffer must be 16-byte aligned (replayed actions: 4-byte)");
    const int Tf = io->T / io->n_frag;
    // ONE launch where the store-wave supply-chain kernel serves the env (its store waves switch planes at the fragments' first rows) ...
    if (e->use_fused && e->d.env_type == PHX_ENV_PLAIN && !e->d.any_typed && e->d.sc_fast.ok && e->d.sc_sw.ok && !io->msg_log && !io->msg_count &&
        (!io->actions || (io->hints & PHX_RH_ACTIONS_IN_DOMAIN)) && (!io->exo || (e->d.sc_sw_exo_first && (io->hints & PHX_RH_EXO_IN_DOMAIN))) &&   // replays: only vouched-for
        e->d.variant_rollout != PHX_VR_GENERAL && io->T <= 0xFFFF && (e->d.variant_rollout == PHX_VR_STORE_WAVES || io->T >= 40)) {                // ones (round 1's kernel has no fragment lists)
      HIPCHK(use_device(e));
      HIPCHK(phx_launch_sc_rollout_sw(e->d, *io, (hipStream_t)stream));
      return PHX_OK;
    }
    // ... the same for an FSM supply chain on its FSM instantiation; the lane-per-pair loop that takes over when an env is off the stage
    // chain has no fragment lists: one guarded launch per fragment behind it (each returns at entry unless the check found such an env)
    if (e->use_fused && e->d.env_type == PHX_ENV_FSM && io->frags[0].terminated && phx_fsm_sw_serves(e->d, *io, (hipStream_t)stream)) {   // (`terminated`: the loop behind needs it)
      HIPCHK(use_device(e));
      const int32_t gen = phx_fsm_next_gen(e->d);
      HIPCHK(phx_launch_sc_rollout_sw(e->d, *io, (hipStream_t)stream, gen));
      for (int f = 0; f < io->n_frag; ++f) {
        const phx_rollout_io sub = frag_io(*io, f, Tf);
        HIPCHK(phx_launch_sc_rollout_fsm(e->d, sub, (hipStream_t)stream, e->d.fsm_irregular, gen));
      }
      return PHX_OK;
    }
    // ... n_frag consecutive launches everywhere else
    for (int f = 0; f < io->n_frag; ++f) {
      phx_rollout_io sub = frag_io(*io, f, Tf);
      const int64_t row = (int64_t)f * Tf * e->d.B;
      if (io->actions) sub.actions = io->actions + row * e->d.S;
      if (io->exo) sub.exo = io->exo + row * e->d.n_exo;
      if (io->msg_log) sub.msg_log = io->msg_log + row * e->d.trace_cap;
      if (io->msg_count) sub.msg_count = io->msg_count + row;
      TRY(rollout_impl(e, &sub, stream));
    }
    return PHX_OK;
  }
  if (io->T <= 0 || !io->obs || !io->action_out || !io->reward || !io->truncated)
    return fail(PHX_EINVAL, "bad rollout io");
  // `terminated` may be NULL where the plane would be all zero AND the kernel that serves the launch can leave it out: the
  // time-parallel supply-chain kernel (ShopAgent never terminates, agents.py:292-323).  4.5 % of the trajectory bytes, ~8 % of the launch.
  if (!io->terminated && !(e->use_fused && e->d.env_type == PHX_ENV_PLAIN && !e->d.any_typed && e->d.sc_fast.ok && !io->actions && !io->exo &&
                           e->d.variant_rollout != PHX_VR_GENERAL))
    return fail(PHX_EINVAL, "phx_rollout: `terminated` is required for this env (only the time-parallel supply-chain rollout can omit the all-zero plane)");
  if ((io->msg_log || io->msg_count) && (e->d.trace_cap <= 0 || !io->msg_log || !io->msg_count))
    return fail(PHX_EINVAL, "rollout message log needs trace_cap > 0 and both msg_log and msg_count");
  {                                   // the rollout kernels write 16-byte pieces
    const void* bufs[] = {io->obs, io->action_out, io->reward, io->terminated, io->truncated, io->obs_valid, io->reward_valid, io->last_obs};
    for (const void* p : bufs)
      if (((uintptr_t)p & 15u) != 0) return fail(PHX_EINVAL, "phx_rollout: every output buffer must be 16-byte aligned");
    // (the replayed inputs are read one float / one byte at a time: a row slice of a longer recording is fine whatever B S is)
    if (((uintptr_t)io->actions & 3u) != 0) return fail(PHX_EINVAL, "phx_rollout: `actions` must be 4-byte aligned");
  }
  if (e->d.n_samplers > 0 && !e->d.device_sampling)
    return fail(PHX_EUNSUPPORTED, "phx_rollout auto-resets on the device: every sampler must be PHX_SAMPLER_UNIFORM");
  HIPCHK(use_device(e));
  if (io->policy) {                   // ABI 10: the policy evaluated on the device (phx_sc_policy.hip; tanh / wide / PHX_VR_POLICY_MFMA: phx_sc_policy_mfma.hip)
    if (!e->use_fused) return fail(PHX_EUNSUPPORTED, "phx_rollout: `policy` needs a plain supply-chain env on its fused schedule");
    const char* why = phx_sc_policy_unsupported(e->d, *io);
    if (why) return fail(strstr(why, "phx_policy_") ? PHX_EINVAL : PHX_EUNSUPPORTED, "phx_rollout: %s", why);      // (phx_policy_mlp / _explore)
    if (phx_sc_policy_wants_mfma(e->d, *io)) HIPCHK(phx_launch_sc_rollout_policy_mfma(e->d, *io, (hipStream_t)stream));      // phx_sc_policy_mfma.hip
    else HIPCHK(phx_launch_sc_rollout_policy(e->d, *io, (hipStream_t)stream));
    return PHX_OK;
  }
  if (e->use_ads && e->n_inject == 0) {
    if (!io->obs_valid || !io->reward_valid) return fail(PHX_EINVAL, "FSM rollouts need obs_valid and reward_valid outputs");
    HIPCHK(phx_launch_ads_rollout(e->d, *io, (hipStream_t)stream));
    return PHX_OK;
  }
  if (e->use_stk && e->prices_compressed && (phx_stk_rollout_lds(e->d) > 60 * 1024 || e->d.A > 3 * 1024) && e->d.f[F_ROLLOUT_SCRATCH]) {
    // a market too large for the LDS-resident rollout kernel: materialise the price table and roll out on the generic
    // engine (the env stays there, like after a host-injected message)
    TRY(leave_stk(e, (hipStream_t)stream));
  }
  if (e->sc_rules_fused && e->d.variant_rollout != PHX_VR_LAUNCH_LOOP && e->d.variant_step != PHX_VS_GENERIC_DYNAMIC && !io->msg_log && !io->msg_count && e->n_inject == 0) {
    // an FSM supply chain whose handlers are rules: the fused lane-per-pair loop evaluates them (round 6; until then the engine's T-step loop)
    if (!io->obs_valid || !io->reward_valid || !io->terminated) return fail(PHX_EINVAL, "FSM rollouts need terminated, obs_valid and reward_valid outputs");
    HIPCHK(phx_launch_sc_rollout_fsm_rules(e->d, *io, (hipStream_t)stream));
    return PHX_OK;
  }
  if (!e->use_fused && !(e->use_stk && e->prices_compressed)) {
    // Launch loop for every other env (any topology of the device kinds, tracking off): per step ONE
    // launch of the generic engine (policy, trajectory row and auto-reset fused in), stream ordered,
    // the step-shaped intermediates in the blob's rollout.scratch field.
    if (!e->d.f[F_ROLLOUT_SCRATCH]) return fail(PHX_EUNSUPPORTED, "phx_rollout: this env switched engines after creation");
    if (e->n_inject) return fail(PHX_EINVAL, "phx_rollout with injected messages pending");
    hipStream_t st = (hipStream_t)stream;
    const GenScratch gs = gen_scratch(e->d.B, std::max(e->d.S, 1), e->d.D);
    char* base = (char*)e->d.f[F_ROLLOUT_SCRATCH];
    phx_step_io sio; memset(&sio, 0, sizeof sio);
    sio.actions = (const float*)(base + gs.actions);
    sio.obs = (float*)(base + gs.obs); sio.obs_valid = (uint8_t*)(base + gs.obs_valid);
    sio.reward = (double*)(base + gs.reward); sio.reward_valid = (uint8_t*)(base + gs.reward_valid);
    sio.terminated = (uint8_t*)(base + gs.terminated); sio.truncated = (uint8_t*)(base + gs.truncated);
    sio.done_valid = (uint8_t*)(base + gs.done_valid);
    sio.all_terminated = (uint8_t*)(base + gs.all_term); sio.all_truncated = (uint8_t*)(base + gs.all_trunc);
    sio.err = io->err;
    GenArgs g; memset(&g, 0, sizeof g); g.io = sio; g.inject = e->inject_dev; g.n_inject = 0; g.resolve_only = 0;
    g.roll = *io; g.roll_actions_in = io->actions; g.roll_actions = (float*)(base + gs.actions);
    if (e->d.variant_rollout != PHX_VR_LAUNCH_LOOP) {
      // ONE launch: the kernel loops over the T steps itself (GenArgs::roll_T) -- queues, staged tables and the env's
      // workgroup stay resident; policy, trajectory row, the caller's reset and the last observation are in the loop
      sio.exo = io->exo; sio.msg_log = io->msg_log; sio.msg_count = io->msg_count;
      g.io = sio; g.roll_t = 0; g.roll_T = io->T;
      HIPCHK(phx_launch_generic(e->d, g, e->lds_ok, st));
      return PHX_OK;
    }
    for (int t = 0; t < io->T; ++t) {            // one launch per step: policy + step + trajectory row + the caller's reset
      sio.exo = io->exo ? io->exo + (int64_t)t * e->d.B * e->d.n_exo : nullptr;
      sio.msg_log = io->msg_log ? io->msg_log + (int64_t)t * e->d.B * e->d.trace_cap : nullptr;   // rollout.py:369-373
      sio.msg_count = io->msg_count ? io->msg_count + (int64_t)t * e->d.B : nullptr;
      g.io = sio; g.roll_t = t;
      HIPCHK(phx_launch_generic(e->d, g, e->lds_ok, st));
    }
    if (io->last_obs) HIPCHK(phx_launch_gen_last_obs(e->d, sio.obs, io->last_obs, st));
    return PHX_OK;
  }
  if (e->use_stk) {
    if (io->exo) return fail(PHX_EINVAL, "the market has no exogenous draws");
    if (phx_stk_rollout_lds(e->d) > 60 * 1024 || e->d.A > 3 * 1024) return fail(PHX_EUNSUPPORTED, "market too large for the LDS-resident rollout");
    HIPCHK(phx_launch_stk_rollout(e->d, *io, (hipStream_t)stream)); return PHX_OK;
  }
  // typed shops (obs dim 4, per-env penalty weight) take the lane-per-pair kernel too
  if (e->d.env_type == PHX_ENV_FSM || e->d.any_typed) { HIPCHK(phx_launch_sc_rollout_fsm(e->d, *io, (hipStream_t)stream)); return PHX_OK; }
  if (e->d.sc_fast.ok && !io->actions && !io->exo && e->d.variant_rollout != PHX_VR_GENERAL) {
    // the store-wave kernel where the caller asked for it, or (PHX_VR_AUTO) where a compile-time shape serves the env and the fragment
    // is longer than its pipeline fill (SC64, B = 4 096: T = 32 14.1 us either way, T = 50 14.7 against 16.4, T = 100 21.2 against
    // 23.1, T = 400 57 against 72-76; several rounds of workgroups: B = 16 384 221 against 242; SC256, B = 8 192, T = 100: 195 against 204)
    if (e->d.sc_sw.ok && io->T <= 0xFFFF && (e->d.variant_rollout == PHX_VR_STORE_WAVES || io->T >= 40)) HIPCHK(phx_launch_sc_rollout_sw(e->d, *io, (hipStream_t)stream));
    else HIPCHK(phx_launch_sc_rollout_fast(e->d, *io, (hipStream_t)stream));
    return PHX_OK;
  }
  // Replayed actions and / or order sizes (a recorded policy, the reference's own numpy stream): the store-wave kernel's REPLAY
  // instantiation where its shape serves the env.  Its tiles hold the stock in a byte: a call with an action that rounds below zero
  // (a negative StockRequest takes the stock below zero) is found by a pre-scan of the call's actions and served by round 1's kernel
  // -- both launches are issued, the device word decides which one runs.
  if (e->d.sc_fast.ok && e->d.sc_sw.ok && e->d.variant_rollout != PHX_VR_GENERAL && e->d.variant_rollout != PHX_VR_TIME_PARALLEL && io->T <= 0xFFFF &&
      (e->d.variant_rollout == PHX_VR_STORE_WAVES || io->T >= 40) && e->d.sc_sw_guard &&
      (!io->exo || (e->d.sc_sw_exo_first && (io->hints & PHX_RH_EXO_IN_DOMAIN)))) {      // (order sizes: only those the caller vouches for, see the hint)
    const bool scan = io->actions && !(io->hints & PHX_RH_ACTIONS_IN_DOMAIN);
    const int32_t gen = scan ? ++e->sw_guard_gen : 0;
    HIPCHK(phx_launch_sc_rollout_sw(e->d, *io, (hipStream_t)stream, gen));
    if (scan) HIPCHK(phx_launch_sc_rollout(e->d, *io, (hipStream_t)stream, e->d.sc_sw_guard, gen));
    return PHX_OK;
  }
  HIPCHK(phx_launch_sc_rollout(e->d, *io, (hipStream_t)stream));
  return PHX_OK;
}

// ---- copying state access by field name -------------------------------------------------
static int64_t field_nbytes(const FieldDef& f) { return (int64_t)f.dim0 * f.dim1 * f.dim2 * esize(f.dtype); }

int64_t phx_get_state(phx_env* e, const char* field, void* buf, int64_t buf_nbytes, void* stream) {
  if (!e || !field || !buf) return fail(PHX_EINVAL, "null argument");
  const FieldDef* f = find_field_by_name(e, field);
  if (!f) return fail(PHX_EINVAL, "unknown state field '%s'", field);
  const int64_t nb = field_nbytes(*f);
  if (!e->d.f[f->id]) return fail(PHX_EINVAL, "field '%s' is not bound", field);
  if (buf_nbytes < nb) return fail(PHX_EINVAL, "buffer of %lld bytes for field '%s' of %lld bytes", (long long)buf_nbytes, field, (long long)nb);
  HIPCHK(use_device(e));
  if (e->prices_compressed && !strcmp(field, "buyer.prices")) HIPCHK(phx_launch_stk_materialise(e->d, (hipStream_t)stream));
  HIPCHK(hipMemcpyAsync(buf, (const char*)e->d.f[f->id], (size_t)nb, hipMemcpyDefault, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return nb;
}

int64_t phx_set_state(phx_env* e, const char* field, const void* buf, int64_t buf_nbytes, void* stream) {
  if (!e || !field || !buf) return fail(PHX_EINVAL, "null argument");
  const FieldDef* f = find_field_by_name(e, field);
  if (!f) return fail(PHX_EINVAL, "unknown state field '%s'", field);
  const int64_t nb = field_nbytes(*f);
  if (!e->d.f[f->id]) return fail(PHX_EINVAL, "field '%s' is not bound", field);
  if (buf_nbytes != nb) return fail(PHX_EINVAL, "field '%s' holds %lld bytes, got %lld", field, (long long)nb, (long long)buf_nbytes);
  HIPCHK(use_device(e));
  if (e->prices_compressed && !strcmp(field, "buyer.prices"))
    return fail(PHX_EUNSUPPORTED, "buyer.prices is kept compressed by the fused market kernel: set seller.posted instead");
  HIPCHK(hipMemcpyAsync((char*)e->d.f[f->id], buf, (size_t)nb, hipMemcpyDefault, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return nb;
}

int phx_trace(phx_env* e, const phx_msg_rec* msg_log, const int32_t* msg_count, int b, phx_msg_rec* out, int cap, void* stream) {
  if (!e || !msg_log || !msg_count || (cap > 0 && !out)) return fail(PHX_EINVAL, "null argument");
  if (e->d.trace_cap <= 0) return fail(PHX_EINVAL, "tracking is off (trace_cap == 0)");
  if (b < 0 || b >= e->d.B) return fail(PHX_EINVAL, "env index out of range");
  HIPCHK(use_device(e));
  int32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, msg_count + b, sizeof n, hipMemcpyDefault, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  int m = n < e->d.trace_cap ? n : e->d.trace_cap;
  if (m > cap) m = cap;
  if (m > 0) {
    HIPCHK(hipMemcpyAsync(out, msg_log + (int64_t)b * e->d.trace_cap, sizeof(phx_msg_rec) * m, hipMemcpyDefault, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  }
  return n;
}

// ---- done-flag planes, bit-packed for rollout collection (SURVEY 8e iii) ----------------------------
__global__ __launch_bounds__(256) void phx_pack_flags_kernel(const uint8_t* __restrict__ src, uint64_t* __restrict__ dst, const int64_t n) {
  // one wave packs 64 consecutive bytes into one word with a ballot; consecutive waves take consecutive words
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = i < n && src[i] != 0;
  const uint64_t bits = __ballot(on);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < ((n + 63) >> 6)) dst[i >> 6] = bits;
}
__global__ __launch_bounds__(256) void phx_unpack_flags_kernel(const uint64_t* __restrict__ src, uint8_t* __restrict__ dst, const int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (uint8_t)((src[i >> 6] >> (i & 63)) & 1u);
}

int phx_pack_flags(const uint8_t* src, uint64_t* dst, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(PHX_EINVAL, "bad argument");
  if (n == 0) return PHX_OK;
  hipLaunchKernelGGL(phx_pack_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
  HIPCHK(hipGetLastError());
  return PHX_OK;
}
int phx_unpack_flags(const uint64_t* src, uint8_t* dst, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(PHX_EINVAL, "bad argument");
  if (n == 0) return PHX_OK;
  hipLaunchKernelGGL(phx_unpack_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
  HIPCHK(hipGetLastError());
  return PHX_OK;
}

// ---- ABI 7: per-env legacy-numpy MT19937 streams (PHX_F_MT19937; supply_chain.py:64's np.random.randint(5)) -----------------
// np.random.seed(seed) of a 32-bit integer = init_genrand (numpy random/src/mt19937/mt19937.c: mt19937_seed): one lane per env
__global__ __launch_bounds__(256) void phx_mt_seed_kernel(const uint32_t* __restrict__ seeds, uint32_t* __restrict__ state,
                                                          int32_t* __restrict__ pos, const int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  uint32_t* mt = state + (int64_t)b * 624;
  uint32_t x = seeds[b];
  mt[0] = x;
  for (uint32_t i = 1; i < 624; ++i) { x = 1812433253u * (x ^ (x >> 30)) + i; mt[i] = x; }
  pos[b] = 624;                                               // the first draw regenerates
}
// One wave per env: the state is staged in LDS, regenerated 64 words at a time (word k of the next state needs the OLD words k and
// k + 1 and, k < 227, the old word k + 397, otherwise the NEW word k - 227: chunks of 64 in order have them all), and 64 words per
// pass are tempered, masked (& 7) and rejected (> 4) with the accepted ones compacted by a ballot -- the words a sequence of
// np.random.randint(5) calls would consume, in order; the pass that reaches a step's last draw consumes up to ITS word only.
// Step by step: the drawing agents of a step are those of the env's acting list (FSM: of its stage, which is walked forward from
// the env's words along stage_next / stage_tab with the reset at the episode's end, as phx_rollout walks it).
struct MtArgs {
  uint32_t* state; int32_t* pos; uint8_t* exo;
  const int32_t *mt_ptr, *mt_rank, *stage_next, *stage_tab, *env_step, *env_stage;
  int32_t B, n_exo, T, fsm, num_steps, initial_stage, zero_rows;
};
__global__ __launch_bounds__(64) void phx_mt_draw_kernel(const MtArgs a) {
  __shared__ uint32_t mt[624];
  const int b = blockIdx.x, lane = threadIdx.x;
  uint32_t* gs = a.state + (int64_t)b * 624;
  for (int i = lane; i < 624; i += 64) mt[i] = gs[i];
  int p = a.pos[b];
  int step = a.fsm ? a.env_step[b] : 0, stage = a.fsm ? a.env_stage[b] : 0;
  __syncthreads();
  for (int t = 0; t < a.T; ++t) {
    const int base = a.mt_ptr[stage], need = a.mt_ptr[stage + 1] - base;
    uint8_t* row = a.exo + ((int64_t)t * a.B + b) * a.n_exo;
    if (a.zero_rows) {                                          // customers that do not act in this step draw nothing: their entries are 0
      for (int j = lane; j < a.n_exo; j += 64) row[j] = 0;       // (one wave: these stores are issued before the draws' stores below)
      __syncthreads();
    }
    int have = 0;
    while (have < need) {
      if (p >= 624) {                                         // genrand's regeneration (mt19937_gen)
        for (int c = 0; c < 624; c += 64) {
          const int k = c + lane;
          uint32_t y = 0, src = 0;
          if (k < 624) {
            y = (mt[k] & 0x80000000u) | (mt[k == 623 ? 0 : k + 1] & 0x7fffffffu);
            src = k < 227 ? mt[k + 397] : mt[k - 227];
          }
          __syncthreads();
          if (k < 624) mt[k] = src ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
          __syncthreads();
        }
        p = 0;
      }
      const int len = 624 - p < 64 ? 624 - p : 64;
      uint32_t y = lane < len ? mt[p + lane] : 0u;
      y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
      const uint32_t v = y & 7u;                              // mask of rng = 4 (buffered_bounded_masked_uint32)
      const bool acc = lane < len && v <= 4u;
      const uint64_t m = __ballot(acc);
      const int before = __popcll(m & ((1ull << lane) - 1ull)), total = __popcll(m);
      const int left = need - have;
      if (acc && before < left) row[a.mt_rank[base + have + before]] = (uint8_t)v;
      if (total <= left) { have += total; p += len; }
      else {                                                  // the step's last draw is inside this pass: stop behind its word
        const uint64_t last = __ballot(acc && before == left - 1);
        p += __ffsll((long long)last);                        // 1-based lane of that word = words consumed
        have = need;
      }
    }
    if (a.fsm) {                                              // fsm.py:281-307 / the auto-reset of a rollout (fsm.py:217)
      const int tn = step + 1;
      stage = a.stage_tab ? a.stage_tab[(int64_t)stage * (a.num_steps + 1) + (tn <= a.num_steps ? tn : a.num_steps)] : a.stage_next[stage];
      step = tn;
      if (step >= a.num_steps) { step = 0; stage = a.initial_stage; }
    }
  }
  __syncthreads();
  for (int i = lane; i < 624; i += 64) gs[i] = mt[i];
  if (lane == 0) a.pos[b] = p;
}

static int mt_check(phx_env* e) {
  if (!e) return fail(PHX_EINVAL, "null env");
  if (!e->d.f[F_ENV_MT_STATE]) return fail(PHX_EUNSUPPORTED, "the spec was compiled without PHX_F_MT19937");
  return PHX_OK;
}
int phx_mt_seed(phx_env* e, const uint32_t* seeds, void* stream) {
  int rc = mt_check(e);
  if (rc != PHX_OK) return rc;
  if (!seeds) return fail(PHX_EINVAL, "seeds is NULL");
  hipStream_t st = (hipStream_t)stream;
  uint32_t* dseeds = nullptr;
  HIPCHK(hipMalloc((void**)&dseeds, sizeof(uint32_t) * e->d.B));
  hipError_t he = hipMemcpyAsync(dseeds, seeds, sizeof(uint32_t) * e->d.B, hipMemcpyHostToDevice, st);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(phx_mt_seed_kernel, dim3((e->d.B + 255) / 256), dim3(256), 0, st, dseeds, (uint32_t*)e->d.f[F_ENV_MT_STATE],
                       (int32_t*)e->d.f[F_ENV_MT_POS], e->d.B);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipStreamSynchronize(st);        // `seeds` is the caller's host memory, the staging buffer is ours
  (void)hipFree(dseeds);
  HIPCHK(he);
  return PHX_OK;
}
int phx_mt_draw(phx_env* e, uint8_t* exo, int T, void* stream) {
  int rc = mt_check(e);
  if (rc != PHX_OK) return rc;
  if (!exo || T < 1) return fail(PHX_EINVAL, "bad argument");
  if (e->d.env_type != PHX_ENV_PLAIN && e->d.env_type != PHX_ENV_FSM) return fail(PHX_EUNSUPPORTED, "phx_mt_draw: PHX_ENV_PLAIN and PHX_ENV_FSM only");
  if (e->d.n_exo < 1) return fail(PHX_EUNSUPPORTED, "the env has no exogenous draws");
  // (a publisher's binomial draws depend on the auction's outcome: they cannot be drawn ahead of the step)
  if (e->der.kind_count[PHX_KIND_PUBLISHER] > 0) return fail(PHX_EUNSUPPORTED, "phx_mt_draw: PublisherAgent draws depend on the auction");
  hipStream_t st = (hipStream_t)stream;
  bool all = e->d.n_lists == 1;                                // every drawing agent draws in every step: no entry is left unwritten
  if (all) all = e->der.act_ptr.size() >= 2 && [&] { int n = 0; for (int k = e->der.act_ptr[0]; k < e->der.act_ptr[1]; ++k) n += e->der.exo_rank[e->der.act_idx[k]] >= 0; return n == e->d.n_exo; }();
  MtArgs a;
  a.state = (uint32_t*)e->d.f[F_ENV_MT_STATE]; a.pos = (int32_t*)e->d.f[F_ENV_MT_POS]; a.exo = exo;
  a.mt_ptr = e->d.mt_ptr; a.mt_rank = e->d.mt_rank; a.stage_next = e->d.stage_next; a.stage_tab = e->d.stage_tab;
  a.env_step = (const int32_t*)e->d.f[F_ENV_STEP]; a.env_stage = (const int32_t*)e->d.f[F_ENV_STAGE];
  a.B = e->d.B; a.n_exo = e->d.n_exo; a.T = T; a.fsm = e->d.env_type == PHX_ENV_FSM ? 1 : 0;
  a.num_steps = e->d.num_steps; a.initial_stage = e->d.initial_stage; a.zero_rows = all ? 0 : 1;
  hipLaunchKernelGGL(phx_mt_draw_kernel, dim3(e->d.B), dim3(64), 0, st, a);
  HIPCHK(hipGetLastError());
  return PHX_OK;
}

}  // extern "C"
