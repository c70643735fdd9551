/*
 * gq_joint_cmd.h - joint-impedance actions (gq_step_joint_cmd): the law a robot's low-level interface applies to the command
 * (q_des, qd_des, tau_ff, kp, kd) of a joint, and the device block that carries a batch's command rows to the persistent step
 * kernel.  Compiles with the product's gq_device.h and with the host emulator's shim (tests/simt_emu).
 */
#pragma once
#include <gq_device.h> /* angle brackets: the include path decides (csrc/ for the product, tests/simt_emu/ for the emulator) */
#include <cstdint>

namespace gq {

/* torque = kp (q_des - q) + kd (qd_des - qd) + tau_ff, every operation rounded on its own: the elementwise float32 expression
 * kp * (q_des - q) + kd * (qd_des - qd) + tau_ff gives the same bits.  With qd_des = 0 and tau_ff = 0 these are the bits of the
 * closed-loop rollout's pd_law, kp * (q_des - q) - kd * qd: up + kd * (0 - qd) = up - kd * qd in IEEE arithmetic, as is adding +0. */
__device__ __forceinline__ float joint_cmd_law(const float q_des, const float qd_des, const float tau_ff, const float kp, const float kd, const float q, const float qd) {
#pragma clang fp contract(off)
  const float e = q_des - q;
  const float ev = qd_des - qd;
  const float up = kp * e;
  const float ud = kd * ev;
  float u = up + ud;
  u = u + tau_ff;
  return u;
}

/* The command rows of one gq_step_joint_cmd call (device pointers): a block of its own in device memory, reached through
 * StepCall::policy with the pointer's tag bit set (gq_step_kernel.h). */
struct JointCmdDev {
  const float* q_des;          /* [N][12] */
  const float* qd_des;         /* [N][12] or NULL (= 0) */
  const float* tau_ff;         /* [N][12] or NULL (= 0) */
  const float* kp; const float* kd; /* [12] (gain_stride 0) or [N][12] (gain_stride 12) */
  float* tau_out;              /* [N][12] torque of the window's last substep, or NULL */
  uint8_t* term_any;           /* [N] OR of `terminated` over the window, or NULL */
  int32_t gain_stride, pad_;
};
}  // namespace gq
