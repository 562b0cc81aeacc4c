// phx_spec.h -- what a phx_spec says, worked out on the host (phx_spec.hip): validation, the derived tables, which fused
// schedule serves the env, the state blob's layout and the generic engine's static round schedule.  No HIP API is called here.
#pragma once
#include <cstdint>
#include <vector>

#include "phx_dev.h"

// the calling thread's error text (phx_last_error): fail() formats it and returns `code`, fail_text() reads it
int fail(int code, const char* fmt, ...);
const char* fail_text();

// ---- derived quantities of a spec ---------------------------------------------------------------------------------------------
struct Derived {
  int A = 0, S = 0, D = 1, n_exo = 0, nnz = 0, buyer_nnz = 0, buyer_dmax = 0, n_lists = 1, scan_cap = 0;
  int kind_count[PHX_KIND_COUNT] = {0};
  std::vector<int32_t> strat_rank, strat_idx, kind_rank, exo_rank, buyer_off;
  std::vector<int32_t> act_ptr, act_idx, stage_next, reset_obs_idx;
  std::vector<uint8_t> stage_allowed, stage_rew_all;
  std::vector<int32_t> stage_tab;
  std::vector<uint8_t> stage_has_rules;   // [n_stages] the stage's handler is a rule list (phx_spec.stage_rules)
  std::vector<uint8_t> act_mask, obs_mask, rew_mask;
  // supply-chain schedule
  bool sc_static = false, stk_static = false, ads_static = false, sc_rules_fused = false;
  int ads_pub = -1, ads_adx = -1, ads_pub_stage = 0;
  bool dynamic_graph = false;      // StochasticNetwork with some rate < 1: edges differ per env
  std::vector<int32_t> shop_agent, shop_norm, shop_cust_ptr, shop_cust_exo, shop_cust_agent;
  std::vector<uint8_t> shop_cust_act;
  std::vector<uint8_t> sc_shop_flags;   // [n_lists][nS]: 1 acts, 2 a customer acts, 4 every customer acts, 8 observes, 16 rewarded
  std::vector<float> sc_tab;
  int n_tabn = 0, n_quot = 0, rew_smax = -1;
  int max_cust = 0;
  std::vector<uint16_t> stk_nbr;
  std::vector<int32_t> stk_nbr_conn;
  std::vector<uint32_t> stk_rec;
  std::vector<uint8_t> stk_flags;
  std::vector<uint32_t> stk_rec2, stk_agent;
  bool stk_packed = false;
  // supertypes
  bool any_typed = false, device_sampling = false;
  std::vector<int32_t> type_src, shop_type_src;
  std::vector<double> shop_type_prm;
};
// validates the spec and fills `d`: PHX_OK, or the failure's code with its text in fail_text()
int derive(const phx_spec* sp, Derived& d);

// ---- state blob layout ----------------------------------------------------------------------------------------------------------
struct FieldDef { int id; const char* name; int dtype; int kind; int64_t dim0, dim1, dim2; int64_t offset; };
inline int64_t esize(int dtype) { return dtype == 1 ? 8 : (dtype == 2 ? 1 : 4); }      // phx_field.dtype: 0 i32, 1 f64, 2 u8, 3 f32
// the blob's fields in order and its size in bytes; *ws_stride: per-env bytes of the generic engine's workspace field, 0 without one
int64_t layout(const phx_spec* sp, const Derived& d, std::vector<FieldDef>& out, int64_t* ws_stride);
// LEAN layout of the generic engine: a scheduled two-wave supply chain keeps its sort / scan scratch in the blob, not in LDS
bool lean_lds_spec(const phx_spec* sp, const Derived& d);

// ---- scratch of the launch-loop rollout: the outputs of one phx_step for the whole batch ---------------------------------------
struct GenScratch { int64_t obs, reward, obs_valid, reward_valid, terminated, truncated, done_valid, all_term, all_trunc, done, actions, total; };
GenScratch gen_scratch(int64_t B, int64_t S, int64_t D);

// ---- static round schedule of the generic engine: blob of per-list records, off[list] = a record's offset or -1 -----------------
struct StaticSched { std::vector<int32_t> blob, off; };
void build_static_schedule(const phx_spec* sp, const Derived& d, StaticSched& out);
