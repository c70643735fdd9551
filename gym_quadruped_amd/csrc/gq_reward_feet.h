/*
 * gq_reward_feet.h - the foot terms of the learning rollout's reward (gq_rollout_policy_learn_feet, gq_reward_eval_feet): air time, slip,
 * impact and clearance.  They CONTINUE the sum S of gq_reward.h after `alive` and before dt * S, and one of them carries state: the air
 * time of every foot, which lives across steps, windows and calls.  Plain C++ for host and device (tests/foot_reward_host.cpp compiles it
 * with g++): contraction off, IEEE +, -, * and fmaf only.  The ORDER of the operations below is the definition.
 *
 * Feet are in canonical order FL, FR, RL, RR whatever the batch's legs_order: the columns are resolved per canonical foot.  Per physics
 * step, from the row AFTER the step, for foot i:  c_i = contact_state[i] != 0;  vx_i, vy_i = feet_vel[i][0:2] (world);  fz_i =
 * contact_forces[i][2] (world);  zb_i = feet_pos:base[i][2];  t_i = the foot's air time so far (the state).  In this order, each skipped
 * when its weight is 0 (its words are never read, its columns may be absent):
 *
 *   air_time   A = 0;  for i = 0..3:  tn = t_i + dt;  if (c_i && t_i > 0) A = A + (tn - air_time_target);  t_i <- c_i ? 0 : tn
 *              with min_cmd_speed > 0:  cx = ex + vx, cy = ey + vy (base_lin_vel_err:base + base_lin_vel:base = the command);
 *              if !(fmaf(cy, cy, cx cx) > min_cmd_speed^2) A = 0 (the state has advanced all the same);   S = fmaf(w, A, S)
 *              The first contact after a re-spawn earns nothing: t_i > 0 is false.
 *   slip       T = 0;  for the feet with c_i:  T = fmaf(vy_i, vy_i, fmaf(vx_i, vx_i, T));                  S = fmaf(w, T, S)
 *   impact     T = 0;  d = fz_i - impact_limit;  if (d > 0) T = T + d;                                     S = fmaf(w, T, S)
 *   clearance  T = 0;  d = zb_i - clearance_target;  T = fmaf(d d, fmaf(vy_i, vy_i, vx_i vx_i), T);         S = fmaf(w, T, S)
 *
 * min_cmd_speed^2 is formed ONCE, on the host.  With all four weights 0 the step reward has the bits of reward_step.
 */
#pragma once
#include "gq_reward.h"

#define GQ_FOOT_TERMS 4

namespace gq {

enum { FW_AIR_TIME = 0, FW_SLIP, FW_IMPACT, FW_CLEARANCE };

/* the foot law's parameters; columns index the observation row per canonical foot, -1 where no term that is on reads them */
struct FootLaw {
  float w[GQ_FOOT_TERMS];
  float air_time_target, min_cmd_speed2, impact_limit, clearance_target;
  int32_t col_c[4], col_vx[4], col_vy[4], col_fz[4], col_zb[4];
  int32_t col_cmd_err[2], col_cmd_vel[2];
};
/* what the foot law reads of one step (words of terms that are off are never looked at) */
struct FootIn {
  float c[4], vx[4], vy[4], fz[4], zb[4];
  float ex, ey, bvx, bvy;
};
__host__ __device__ inline bool foot_on(const FootLaw& F) { return F.w[FW_AIR_TIME] != 0.0f || F.w[FW_SLIP] != 0.0f || F.w[FW_IMPACT] != 0.0f || F.w[FW_CLEARANCE] != 0.0f; }
__host__ __device__ inline bool foot_needs_c(const FootLaw& F) { return F.w[FW_AIR_TIME] != 0.0f || F.w[FW_SLIP] != 0.0f; }
__host__ __device__ inline bool foot_needs_v(const FootLaw& F) { return F.w[FW_SLIP] != 0.0f || F.w[FW_CLEARANCE] != 0.0f; }
__host__ __device__ inline bool foot_needs_cmd(const FootLaw& F) { return F.w[FW_AIR_TIME] != 0.0f && F.min_cmd_speed2 > 0.0f; }

/* gather the row's words with `ld` (as reward_gather_row): every load is issued before any word is used */
template <class Ld>
__host__ __device__ inline void foot_gather_row(const FootLaw& F, Ld ld, FootIn& in) {
  if (foot_needs_c(F)) {
#pragma unroll
    for (int i = 0; i < 4; i++) in.c[i] = ld(F.col_c[i]);
  }
  if (foot_needs_v(F)) {
#pragma unroll
    for (int i = 0; i < 4; i++) { in.vx[i] = ld(F.col_vx[i]); in.vy[i] = ld(F.col_vy[i]); }
  }
  if (F.w[FW_IMPACT] != 0.0f) {
#pragma unroll
    for (int i = 0; i < 4; i++) in.fz[i] = ld(F.col_fz[i]);
  }
  if (F.w[FW_CLEARANCE] != 0.0f) {
#pragma unroll
    for (int i = 0; i < 4; i++) in.zb[i] = ld(F.col_zb[i]);
  }
  if (foot_needs_cmd(F)) { in.ex = ld(F.col_cmd_err[0]); in.ey = ld(F.col_cmd_err[1]); in.bvx = ld(F.col_cmd_vel[0]); in.bvy = ld(F.col_cmd_vel[1]); }
}

/* THE FOOT LAW: S (reward_sum's value) continued by the foot terms; t[4] is the air-time state, read and advanced when air_time is on */
__host__ __device__ inline float foot_sum(const FootLaw& F, const FootIn& in, const float dt, float S, float t[4]) {
#pragma clang fp contract(off)
  if (F.w[FW_AIR_TIME] != 0.0f) {
    float A = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool c = in.c[i] != 0.0f;
      const float tn = t[i] + dt;
      if (c && t[i] > 0.0f) A = A + (tn - F.air_time_target);
      t[i] = c ? 0.0f : tn;
    }
    if (F.min_cmd_speed2 > 0.0f) {
      const float cx = in.ex + in.bvx, cy = in.ey + in.bvy;
      if (!(fmaf(cy, cy, cx * cx) > F.min_cmd_speed2)) A = 0.0f;
    }
    S = fmaf(F.w[FW_AIR_TIME], A, S);
  }
  if (F.w[FW_SLIP] != 0.0f) {
    float T = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (in.c[i] != 0.0f) T = fmaf(in.vy[i], in.vy[i], fmaf(in.vx[i], in.vx[i], T));
    S = fmaf(F.w[FW_SLIP], T, S);
  }
  if (F.w[FW_IMPACT] != 0.0f) {
    float T = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float d = in.fz[i] - F.impact_limit;
      if (d > 0.0f) T = T + d;
    }
    S = fmaf(F.w[FW_IMPACT], T, S);
  }
  if (F.w[FW_CLEARANCE] != 0.0f) {
    float T = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float d = in.zb[i] - F.clearance_target;
      T = fmaf(d * d, fmaf(in.vy[i], in.vy[i], in.vx[i] * in.vx[i]), T);
    }
    S = fmaf(F.w[FW_CLEARANCE], T, S);
  }
  return S;
}

/* one step's reward with the foot terms: reward_step with its sum continued */
__host__ __device__ inline float foot_reward_step(const RewardLaw& R, const FootLaw& F, const RewardIn& in, const FootIn& fin, const int terminated, float t[4]) {
  return reward_finish(R, foot_sum(F, fin, R.dt, reward_sum(R, in), t), terminated);
}

/* as reward_law_load */
__host__ __device__ __forceinline__ FootLaw foot_law_load(const GQ_MODEL FootLaw& s) {
  FootLaw f;
#pragma unroll
  for (int i = 0; i < GQ_FOOT_TERMS; i++) f.w[i] = s.w[i];
  f.air_time_target = s.air_time_target; f.min_cmd_speed2 = s.min_cmd_speed2; f.impact_limit = s.impact_limit; f.clearance_target = s.clearance_target;
#pragma unroll
  for (int i = 0; i < 4; i++) { f.col_c[i] = s.col_c[i]; f.col_vx[i] = s.col_vx[i]; f.col_vy[i] = s.col_vy[i]; f.col_fz[i] = s.col_fz[i]; f.col_zb[i] = s.col_zb[i]; }
  f.col_cmd_err[0] = s.col_cmd_err[0]; f.col_cmd_err[1] = s.col_cmd_err[1]; f.col_cmd_vel[0] = s.col_cmd_vel[0]; f.col_cmd_vel[1] = s.col_cmd_vel[1];
  return f;
}
}  // namespace gq
