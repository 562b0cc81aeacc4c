// phx_launch.h -- every host function that crosses translation units: the kernels' launchers, their plan / size functions and the
// schedule compiler.  phx_api.hip and phx_spec.hip call them; every .hip that defines one includes this header, so the compiler
// checks the definition against the declaration.  Default arguments are stated here and nowhere else.
#pragma once
#include <vector>

#include "phx_dev.h"
// ---- the message-passing engine (phx_generic.hip, phx_generic_sched.hip) ------------------------------------------------------
size_t phx_generic_queue_bytes(int A, int S, int Q, int scan_cap, int n_adx, bool lean = false);
size_t phx_generic_lean_ws_bytes(int Q, int scan_cap);
size_t phx_generic_table_bytes(int A, int nnz);
hipError_t phx_launch_generic(const DevSpec& sp, const GenArgs& g, bool lds, hipStream_t st);
hipError_t phx_launch_reset(const DevSpec& sp, const uint8_t* mask, const double* sampler_values, const uint8_t* conn_values, float* obs, uint8_t* obs_valid, hipStream_t st);
hipError_t phx_launch_gen_last_obs(const DevSpec& sp, const float* obs, float* last_obs, hipStream_t st);
bool phx_sched_compile(const phx_spec* spec, int A, int n_lists, const int32_t* act_ptr, const int32_t* act_idx, const uint8_t* act_mask,
                       const uint8_t* obs_mask, const uint8_t* rew_mask, const int32_t* kind_rank, const int32_t* exo_rank, const int32_t* strat_rank,
                       const int32_t* reset_obs_idx, int n_reset_obs, std::vector<int32_t>* blob, std::vector<int32_t>* recs, int* L_out, int* qmax_out);
size_t phx_sched_lds_bytes(int words, int L, int qstride, int n_rules, int n_lists);
hipError_t phx_launch_sched(const DevSpec& sp, const GenArgs& g, hipStream_t st);
// ---- fused supply chain: step, lane-per-pair rollout loops (phx_sc_fused.hip) -------------------------------------------------
static const int SC_RULES_MAX_S = 256;      // rule-form FSM rollout: whole envs per 256-lane workgroup
hipError_t phx_launch_sc_step(const DevSpec& sp, const phx_step_io& io, hipStream_t st);
// only_if / gen: the launch runs only where *only_if == gen (DevSpec::sc_sw_guard, DevSpec::fsm_irregular); NULL: always
hipError_t phx_launch_sc_rollout(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st, const int32_t* only_if = nullptr, int32_t gen = 0);
hipError_t phx_launch_sc_rollout_fsm(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st, const int32_t* only_if = nullptr, int32_t gen = 0);
hipError_t phx_launch_sc_rollout_fsm_rules(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
// the store-wave kernel's FSM instantiation (phx_sc_rollout_sw.hip, MODE 2): does it serve this launch?
bool phx_fsm_sw_serves(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
// ---- time-parallel supply-chain rollout (phx_sc_rollout.hip) -------------------------------------------------------------------
// decides whether an env shape takes the fast rollout kernel and with which block shape
// `block`: phx_spec.variant_block (0 auto, PHX_VB_WHOLE_ENVS, or pairs per workgroup); `aligned`: the auto choice prefers
// workgroups of G consecutive (env, shop) pairs whose trajectory row segments are whole 64-byte pieces (G % 16 == 0) and a
// grid that is a multiple of the 256 CUs, over whole envs per workgroup
bool phx_sc_fast_plan(int B, int S, int K_uniform, bool norm_uniform, int num_steps, int block, bool aligned, ScFastPlan* p);
hipError_t phx_launch_sc_rollout_fast(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
// ---- store-wave rollout kernel (phx_sc_rollout_sw.hip): workgroups of G % 16 == 0 consecutive pairs, dense flag planes ---------
bool phx_sc_sw_plan(int B, int S, int K_uniform, bool norm_uniform, int num_steps, int block, ScSwPlan* p, int fsm_ns = 0);
// guard_gen: the call's number for DevSpec::sc_sw_guard (replayed actions: a pre-scan sends calls with an action that rounds below zero to round 1's kernel)
hipError_t phx_launch_sc_rollout_sw(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st, int32_t guard_gen = 0);
void phx_sc_sw_tables(int K, int norm, std::vector<uint8_t>* out);      // the kernel's table image (uploaded once per env)
// ---- time-parallel FSM rollout (phx_sc_rollout_fsm.hip) ------------------------------------------------------------------------
// issues the launch and returns true when the plan applies; the caller then issues the lane-per-pair loop guarded by
// DevSpec::fsm_irregular == *gen (it runs only if some env is off the tabulated stage chain)
bool phx_launch_sc_rollout_fsmfast(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st, hipError_t* err, int32_t* gen);
int32_t phx_fsm_next_gen(const DevSpec& sp);                            // the env's next launch generation for DevSpec::fsm_irregular (never 0)
// ---- device policies inside the fused rollout (phx_sc_policy.hip, phx_sc_policy_mfma.hip) --------------------------------------
const char* phx_sc_policy_unsupported(const DevSpec& sp, const phx_rollout_io& io);   // NULL, or why the policy kernels decline the call
bool phx_sc_policy_wants_mfma(const DevSpec& sp, const phx_rollout_io& io);
hipError_t phx_launch_sc_rollout_policy(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
hipError_t phx_launch_sc_rollout_policy_mfma(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
// ---- fused Stackelberg market (phx_stk_fused.hip) -------------------------------------------------------------------------------
size_t phx_stk_rollout_lds(const DevSpec& sp);
hipError_t phx_launch_stk_step(const DevSpec& sp, const phx_step_io& io, hipStream_t st);
hipError_t phx_launch_stk_rollout(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
hipError_t phx_launch_stk_materialise(const DevSpec& sp, hipStream_t st);
// ---- fused digital-ads market (phx_ads_fused.hip) -------------------------------------------------------------------------------
hipError_t phx_launch_ads_step(const DevSpec& sp, const phx_step_io& io, hipStream_t st);
hipError_t phx_launch_ads_rollout(const DevSpec& sp, const phx_rollout_io& io, hipStream_t st);
