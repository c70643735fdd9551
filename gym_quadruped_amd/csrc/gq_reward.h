/*
 * gq_reward.h - the task reward of the learning rollout (gq_rollout_policy_learn, gq_reward_eval): the law of ONE physics step's reward,
 * and the block that carries a call's weights and columns to the device.  gq_reward_feet.h continues the sum with the foot terms; the
 * per-env window bookkeeping of policy_mlp_kernel<1 / 2> is gq_learn.h.
 * Plain C++ for host and device (tests/reward_host.cpp compiles it with g++): contraction off, IEEE +, -, * and fmaf only - the same
 * bits from any compiler.  The ORDER of the operations below is the definition.
 *
 *   step reward = dt * S + w_termination * terminated,      S = fmaf(w_i, term_i, S) over the terms with w_i != 0 in the order of the
 *   enum, from S = 0.  A term with weight 0 is skipped: its inputs are not read (its columns may be absent, its words may be anything).
 *
 *   track_lin_vel  exp(-(ex ex + ey ey) / sigma_lin)   base_lin_vel_err:base [0:2]     x = fmaf(ey, ey, ex ex) * inv_sigma_lin
 *   track_ang_vel  exp(-ez ez / sigma_ang)             base_ang_vel_err:base [2]       x = (ez ez) * inv_sigma_ang
 *   lin_vel_z      vz vz                               base_lin_vel:base [2]
 *   ang_vel_xy     fmaf(wy, wy, wx wx)                 base_ang_vel:base [0:2]
 *   orientation    fmaf(gy, gy, gx gx)                 gravity_vector:base [0:2]
 *   base_height    d d, d = z - base_height_target     base_pos [2]
 *   torques        sum u_j u_j                         the torques applied in the step
 *   joint_vel      sum qd_j qd_j                       qvel_js (or qvel[6:])
 *   power          sum |u_j| |qd_j|                    (= sum |u_j qd_j|)
 *   action_rate    sum (a_j - a_prev_j)^2              the policy's held action and the one before it
 *   alive          1
 *   termination    terminated (0 / 1), NOT multiplied by dt
 * Sums over the 12 joints: one fmaf chain from 0, j ascending.  exp(-x), x >= 0:  mlp_expm1(-min(x, 87)) + 1 (gq_policy_mlp.h) - no new
 * transcendental arithmetic.  inv_sigma = 1.0f / sigma is computed ONCE, on the host, by an IEEE division (the device's fp32 '/' is built
 * without the correctly rounded expansion: csrc/Makefile), so the law multiplies.
 */
#pragma once
#include "gq_policy_mlp.h"

#define GQ_REWARD_TERMS 12

namespace gq {

enum {
  RW_TRACK_LIN_VEL = 0, RW_TRACK_ANG_VEL, RW_LIN_VEL_Z, RW_ANG_VEL_XY, RW_ORIENTATION, RW_BASE_HEIGHT,
  RW_TORQUES, RW_JOINT_VEL, RW_POWER, RW_ACTION_RATE, RW_ALIVE, RW_TERMINATION
};

/* the law's parameters; columns index the observation row, -1 where the term that reads them is off */
struct RewardLaw {
  float w[GQ_REWARD_TERMS];
  float inv_sigma_lin, inv_sigma_ang, base_height_target, dt;
  int32_t col_lin_err[2], col_ang_err_z, col_vz, col_wxy[2], col_gxy[2], col_z, pad_;
  int32_t col_qd[12];
};
/* what the law reads of one step, gathered by the caller (words of terms that are off are never looked at) */
struct RewardIn {
  float ex, ey, ez, vz, wx, wy, gx, gy, z;
  float qd[12], u[12], a[12], a_prev[12];
};
__host__ __device__ inline bool reward_needs_qd(const RewardLaw& R) { return R.w[RW_JOINT_VEL] != 0.0f || R.w[RW_POWER] != 0.0f; }
__host__ __device__ inline bool reward_needs_u(const RewardLaw& R) { return R.w[RW_TORQUES] != 0.0f || R.w[RW_POWER] != 0.0f; }
__host__ __device__ inline bool reward_needs_a(const RewardLaw& R) { return R.w[RW_ACTION_RATE] != 0.0f; }

/* exp(-x) for x >= 0 (a NaN takes the clamp's value) */
__host__ __device__ inline float reward_exp_neg(const float x) {
#pragma clang fp contract(off)
  const float c = x < 87.0f ? x : 87.0f;
  return mlp_expm1(-c) + 1.0f;
}

/* gather the row's words with `ld` (column -> float: a plain load on the host and in the eval kernel, a device-scope load in the rollout) */
template <class Ld>
__host__ __device__ inline void reward_gather_row(const RewardLaw& R, Ld ld, RewardIn& in) {
  if (R.w[RW_TRACK_LIN_VEL] != 0.0f) { in.ex = ld(R.col_lin_err[0]); in.ey = ld(R.col_lin_err[1]); }
  if (R.w[RW_TRACK_ANG_VEL] != 0.0f) in.ez = ld(R.col_ang_err_z);
  if (R.w[RW_LIN_VEL_Z] != 0.0f) in.vz = ld(R.col_vz);
  if (R.w[RW_ANG_VEL_XY] != 0.0f) { in.wx = ld(R.col_wxy[0]); in.wy = ld(R.col_wxy[1]); }
  if (R.w[RW_ORIENTATION] != 0.0f) { in.gx = ld(R.col_gxy[0]); in.gy = ld(R.col_gxy[1]); }
  if (R.w[RW_BASE_HEIGHT] != 0.0f) in.z = ld(R.col_z);
  if (reward_needs_qd(R)) {
#pragma unroll
    for (int j = 0; j < 12; j++) in.qd[j] = ld(R.col_qd[j]);
  }
}

/* THE LAW, in two halves so that gq_reward_feet.h can continue the sum: S through `alive`, then dt * S and the termination */
__host__ __device__ inline float reward_sum(const RewardLaw& R, const RewardIn& in) {
#pragma clang fp contract(off)
  float S = 0.0f;
  if (R.w[RW_TRACK_LIN_VEL] != 0.0f) {
    const float e2 = fmaf(in.ey, in.ey, in.ex * in.ex);
    S = fmaf(R.w[RW_TRACK_LIN_VEL], reward_exp_neg(e2 * R.inv_sigma_lin), S);
  }
  if (R.w[RW_TRACK_ANG_VEL] != 0.0f) {
    const float e2 = in.ez * in.ez;
    S = fmaf(R.w[RW_TRACK_ANG_VEL], reward_exp_neg(e2 * R.inv_sigma_ang), S);
  }
  if (R.w[RW_LIN_VEL_Z] != 0.0f) S = fmaf(R.w[RW_LIN_VEL_Z], in.vz * in.vz, S);
  if (R.w[RW_ANG_VEL_XY] != 0.0f) S = fmaf(R.w[RW_ANG_VEL_XY], fmaf(in.wy, in.wy, in.wx * in.wx), S);
  if (R.w[RW_ORIENTATION] != 0.0f) S = fmaf(R.w[RW_ORIENTATION], fmaf(in.gy, in.gy, in.gx * in.gx), S);
  if (R.w[RW_BASE_HEIGHT] != 0.0f) {
    const float d = in.z - R.base_height_target;
    S = fmaf(R.w[RW_BASE_HEIGHT], d * d, S);
  }
  if (R.w[RW_TORQUES] != 0.0f) {
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < 12; j++) t = fmaf(in.u[j], in.u[j], t);
    S = fmaf(R.w[RW_TORQUES], t, S);
  }
  if (R.w[RW_JOINT_VEL] != 0.0f) {
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < 12; j++) t = fmaf(in.qd[j], in.qd[j], t);
    S = fmaf(R.w[RW_JOINT_VEL], t, S);
  }
  if (R.w[RW_POWER] != 0.0f) {
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < 12; j++) t = fmaf(fabsf(in.u[j]), fabsf(in.qd[j]), t);
    S = fmaf(R.w[RW_POWER], t, S);
  }
  if (R.w[RW_ACTION_RATE] != 0.0f) {
    float t = 0.0f;
#pragma unroll
    for (int j = 0; j < 12; j++) { const float d = in.a[j] - in.a_prev[j]; t = fmaf(d, d, t); }
    S = fmaf(R.w[RW_ACTION_RATE], t, S);
  }
  if (R.w[RW_ALIVE] != 0.0f) S = S + R.w[RW_ALIVE];
  return S;
}
__host__ __device__ inline float reward_finish(const RewardLaw& R, const float S, const int terminated) {
#pragma clang fp contract(off)
  const float r = R.dt * S;
  return terminated ? r + R.w[RW_TERMINATION] : r;
}
__host__ __device__ inline float reward_step(const RewardLaw& R, const RewardIn& in, const int terminated) { return reward_finish(R, reward_sum(R, in), terminated); }

/* the law out of the device block (constant address space: scalar loads) into registers; a plain copy on the host */
__host__ __device__ __forceinline__ RewardLaw reward_law_load(const GQ_MODEL RewardLaw& s) {
  RewardLaw r;
#pragma unroll
  for (int i = 0; i < GQ_REWARD_TERMS; i++) r.w[i] = s.w[i];
  r.inv_sigma_lin = s.inv_sigma_lin; r.inv_sigma_ang = s.inv_sigma_ang; r.base_height_target = s.base_height_target; r.dt = s.dt;
  r.col_lin_err[0] = s.col_lin_err[0]; r.col_lin_err[1] = s.col_lin_err[1]; r.col_ang_err_z = s.col_ang_err_z; r.col_vz = s.col_vz;
  r.col_wxy[0] = s.col_wxy[0]; r.col_wxy[1] = s.col_wxy[1]; r.col_gxy[0] = s.col_gxy[0]; r.col_gxy[1] = s.col_gxy[1];
  r.col_z = s.col_z; r.pad_ = 0;
#pragma unroll
  for (int j = 0; j < 12; j++) r.col_qd[j] = s.col_qd[j];
  return r;
}
}  // namespace gq
