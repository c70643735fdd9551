/*
 * gq_foot_cmd.h - foot-space actions (gq_step_foot_cmd): the law that turns a foot's virtual force and Cartesian impedance command into
 * the three torques of its leg, tau_leg = J^T F + tau_ff, and the device block that carries a batch's command rows to the persistent
 * step kernel.  Compiles with the product's gq_device.h and with the host emulator's shim (tests/simt_emu), like gq_joint_cmd.h; the
 * small math (quaternions, sincos_small) is gq_step_kernel.h's, the routines stage S1 uses.
 */
#pragma once
#include "gq_step_kernel.h"

namespace gq {

/* one foot's words of the command rows: p_des, v_des, f_ff and the gains per axis (x, y, z in the axes of the frame), tau_ff per hinge of
 * the foot's leg (hip, thigh, calf) */
struct FootCmd { float p_des[3], v_des[3], f_ff[3], kp[3], kd[3], tau_ff[3]; };

/* One leg.  Forward kinematics of the chain alone, in the BASE frame (base at the origin, identity orientation), link by link as stage
 * S1 (stage_kinematics) forms the transforms: ql = body_quat * rot(axis, q - qpos0), child origin = anchor - R(ql) jnt_pos, world anchor /
 * axis of hinge i in its parent's frame, the quaternion product normalised at every link.
 *   p_B  = calf origin + R(calf) foot        foot geom centre relative to the base origin
 *   J_B  column i = a_i x (p_B - o_i)        a_i / o_i: axis / anchor of the leg's i-th hinge
 *   A    = I (frame 0: base)  or  R(qb) (frame 1: world AXES, origin still at the base - no world coordinate enters float32)
 *   p = A p_B,  J = A J_B,  v = J qd         (foot velocity relative to the base, from the leg's joint rates only)
 *   F = f_ff + kp .* (p_des - p) + kd .* (v_des - v)
 *   tau = J^T F + tau_ff
 * Only J^T is used: no pose is singular.  Contraction is the compiler's (the law is held to an fp64 evaluation within a rounding
 * bound, tests/test_foot_cmd_host.py - not to the bits of an expression).
 * It comes in two halves, as S1 does its kinematics: the link's local transform (every link on a lane of its own in the kernel), then
 * the chain (lane = foot), with the 13 words per link handed over in between - through LDS in the kernel, so that no lane ever holds three
 * link records next to the chain's intermediates.  foot_cmd_law below is the two put together over plain arguments. */
#define GQ_FOOT_LINK_WORDS 13 /* ql (4), child origin (3), hinge anchor (3), hinge axis (3): all in the parent's frame */
__device__ __forceinline__ void foot_cmd_link(const GqDevLinkRec& L, const float q, float* o) {
  float R1[9], sn, cs;
  sincos_small(0.5f * (q - L.qpos0), sn, cs);
  const Q4 bq = {L.bq[0], L.bq[1], L.bq[2], L.bq[3]};
  const Q4 qr = {cs, L.ax[0] * sn, L.ax[1] * sn, L.ax[2] * sn};
  const Q4 ql = qmul(bq, qr);
  q2mat(R1, ql);
  const V3 aloc = ld3(L.aloc);
  const V3 ploc = aloc - matvec(R1, ld3(L.jp)); /* child origin: rotation about the anchor keeps it fixed */
  o[0] = ql.w; o[1] = ql.x; o[2] = ql.y; o[3] = ql.z;
  st3(o + 4, ploc); st3(o + 7, aloc); st3(o + 10, ld3(L.r0ax));
}
__device__ __forceinline__ void foot_cmd_chain(const float* o0, const float* o1, const float* o2, const float* foot /* [3] calf frame */, const float* qd /* [3] */,
                                               const float* qb /* [4] */, const FootCmd& c, const int frame, float* tau /* [3] out */) {
  V3 anchor[3], axis[3];
  float Rp[9];
  /* hip: the parent is the base - identity */
  anchor[0] = ld3(o0 + 7); axis[0] = ld3(o0 + 10);
  V3 pp = ld3(o0 + 4);
  Q4 pq = qnormalize(Q4{o0[0], o0[1], o0[2], o0[3]});
  q2mat(Rp, pq);
#pragma unroll
  for (int i = 1; i < 3; i++) {
    const float* o = i == 1 ? o1 : o2;
    anchor[i] = pp + matvec(Rp, ld3(o + 7));
    axis[i] = matvec(Rp, ld3(o + 10));
    pp = pp + matvec(Rp, ld3(o + 4));
    pq = qnormalize(qmul(pq, Q4{o[0], o[1], o[2], o[3]}));
    q2mat(Rp, pq);
  }
  V3 p = pp + matvec(Rp, ld3(foot));
  V3 J[3];
#pragma unroll
  for (int i = 0; i < 3; i++) J[i] = cross(axis[i], p - anchor[i]);
  if (frame) {
    float A[9];
    const Q4 qn = qnormalize(Q4{qb[0], qb[1], qb[2], qb[3]});
    q2mat(A, qn);
    p = matvec(A, p);
#pragma unroll
    for (int i = 0; i < 3; i++) J[i] = matvec(A, J[i]);
  }
  const V3 v = qd[0] * J[0] + (qd[1] * J[1] + qd[2] * J[2]);
  const V3 F = v3(c.f_ff[0] + c.kp[0] * (c.p_des[0] - p.x) + c.kd[0] * (c.v_des[0] - v.x),
                  c.f_ff[1] + c.kp[1] * (c.p_des[1] - p.y) + c.kd[1] * (c.v_des[1] - v.y),
                  c.f_ff[2] + c.kp[2] * (c.p_des[2] - p.z) + c.kd[2] * (c.v_des[2] - v.z));
#pragma unroll
  for (int i = 0; i < 3; i++) tau[i] = dot(J[i], F) + c.tau_ff[i];
}
/* The two halves put together over plain arguments: the entry of the host test (tests/test_foot_cmd_host.py).  The kernel calls the halves
 * itself, with LDS in between (foot_cmd_inline, gq_step_driver.h); that hand-over is covered by the GPU law-value test and, under the host
 * emulator, by tests/test_window_emulated.py - not by that host run. */
__device__ __forceinline__ void foot_cmd_law(const GqDevLinkRec& L0, const GqDevLinkRec& L1, const GqDevLinkRec& L2, const float* foot /* [3] calf frame */,
                                             const float* q /* [3] */, const float* qd /* [3] */, const float* qb /* [4] */, const FootCmd& c, const int frame,
                                             float* tau /* [3] out */) {
  float o[3][GQ_FOOT_LINK_WORDS];
  foot_cmd_link(L0, q[0], o[0]); foot_cmd_link(L1, q[1], o[1]); foot_cmd_link(L2, q[2], o[2]);
  foot_cmd_chain(o[0], o[1], o[2], foot, qd, qb, c, frame, tau);
}

/* The command rows of one gq_step_foot_cmd call (device pointers): a block of its own in device memory, reached through
 * StepCall::policy with tag bit 1 set.  Foot rows are [foot k: FL FR RL RR][xyz]; tau_ff / tau_out are in hinge order. */
struct FootCmdDev {
  const float* p_des;          /* [N][12] */
  const float* v_des;          /* [N][12] or NULL (= 0) */
  const float* f_ff;           /* [N][12] or NULL (= 0) */
  const float* tau_ff;         /* [N][12] or NULL (= 0), hinge order */
  const float* kp; const float* kd; /* [12] (gain_stride 0) or [N][12] (gain_stride 12) */
  float* tau_out;              /* [N][12] torque of the window's last substep, or NULL */
  uint8_t* term_any;           /* [N] OR of `terminated` over the window, or NULL */
  int32_t gain_stride, frame;  /* frame: 0 base, 1 world axes */
};
/* StepCall::policy, tag bit 1: a FootCmdDev (bit 0: a JointCmdDev, gq_step_kernel.h; the blocks come from hipMalloc, 256-byte aligned).
 * The launch reads the tag on the host and picks the persistent variants that hold the foot-space law (step_kernel_foot): the kernels
 * of the other policies never see such a block, and these never see another. */
#define GQ_POLICY_FOOT_CMD ((uintptr_t)2)
__host__ __device__ inline const PolicyPdDev* policy_tag_foot_cmd(const FootCmdDev* f) { return reinterpret_cast<const PolicyPdDev*>(reinterpret_cast<uintptr_t>(f) | GQ_POLICY_FOOT_CMD); }
__host__ __device__ inline bool policy_is_foot_cmd(const PolicyPdDev* p) { return (reinterpret_cast<uintptr_t>(p) & GQ_POLICY_FOOT_CMD) != 0; }
__host__ __device__ inline const FootCmdDev* policy_foot_cmd(const PolicyPdDev* p) { return reinterpret_cast<const FootCmdDev*>(reinterpret_cast<uintptr_t>(p) & ~GQ_POLICY_FOOT_CMD); }
}  // namespace gq
