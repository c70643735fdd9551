/*
 * gq_step_driver.h - the driver of the step kernel: the persistent step loop, the re-spawn loop around reset_wave / step_wave and the
 * inline policies of the persistent variants.  A header, so that the one definition serves both the __global__ kernels of gq_kernels.hip
 * (each a one-line call of step_kernel_body) and the tests' host emulator (tests/simt_emu), which cannot include a .hip file.
 */
#pragma once
#include <gq_device.h>
#include "gq_step_body.h"
#include "gq_foot_cmd.h"

namespace gq {

/* joint-space PD law of the closed-loop rollouts, every operation rounded on its own (the elementwise torch expression
 * kp * (q_des - q) - kd * qd gives the same bits) */
__device__ __forceinline__ float pd_law(float kp, float kd, float qdes, float q, float qd) {
#pragma clang fp contract(off)
  const float e = qdes - q;
  const float up = kp * e;
  const float ud = kd * qd;
  return up - ud;
}
/* the built-in policy's action for joint j of env `gid` at step `k` of the rollout: the PD law + exploration noise */
__device__ __forceinline__ float pd_action(const GQ_MODEL PolicyPdDev& P, const int j, const float q, const float qd, const int k, const uint32_t gid) {
#pragma clang fp contract(off)
  float u = pd_law(P.kp[j], P.kd[j], P.qdes[j], q, qd);
  if (P.sigma > 0.0f) {
    const float z = philox_normal((uint32_t)j, (uint32_t)(P.step0 + k), gid, 0x9011u, P.seed_lo, P.seed_hi);
    const float nz = P.sigma * z;
    u = u + nz;
  }
  return u;
}
/* inline mode of the closed-loop rollout: lanes 0-11 turn the observation row this wavefront published at the end of its previous
 * step (global memory, the batch's own layout) into the control of the step that starts now; replaces what load_rows left in W.ctrl */
__device__ __forceinline__ void pd_inline(const GQ_MODEL PolicyPdDev& P, const StepArgs& a, const StepCall& c, WaveMem& W, const int env, const int kstep,
                                          const bool apply /* false: the env spends this step on its re-spawn and ignores the action */) {
  const int lane = lane_id();
  if (lane < 12) {
    const int od = mptr(a.batch)->obs_dim;
    const GQ_GLOBAL float* row = gptr(a.obs) + (size_t)env * od;
    const float u = pd_action(P, lane, row[P.col_q[lane]], row[P.col_qd[lane]], kstep, (uint32_t)(env + P.env_id_offset));
    if (apply) W.ctrl[lane] = u;
    if (c.act_seq) gptr(c.act_seq)[((size_t)kstep * a.n_envs + env) * 12 + lane] = u;
  }
}

/* the second inline policy of the persistent kernel: lanes 0-11 fetch their joint's words of the env's command rows (absent rows -
 * qd_des, tau_ff - read as 0) and evaluate the joint-impedance law on the joint state load_rows has just staged in LDS (W.qj, W.qvel -
 * not the observation row: any observation layout works); the same command at every substep of the window (zero-order hold);
 * replaces what load_rows left in W.ctrl.  Everything happens here, behind load_rows: nothing of it is live in the prologue that
 * every persistent launch shares. */
__device__ __forceinline__ void joint_cmd_inline(const GQ_MODEL JointCmdDev& J, const StepArgs& a, const StepCall& c, WaveMem& W, const int env,
                                                 const int kstep, const bool last, const bool apply /* false: the env spends this substep on its re-spawn and ignores the torque */) {
  const int lane = lane_id();
  wave_barrier(); /* W.qj / W.qvel were stored by other lanes (load_rows: lane = word of the row) */
  if (lane < 12) {
    const size_t r = (size_t)env * 12 + lane, g = (size_t)env * (size_t)J.gain_stride + lane;
    const float q_des = gptr(J.q_des)[r];
    const float qd_des = J.qd_des ? gptr(J.qd_des)[r] : 0.0f;
    const float tau_ff = J.tau_ff ? gptr(J.tau_ff)[r] : 0.0f;
    const float kp = gptr(J.kp)[g], kd = gptr(J.kd)[g];
    const float u = joint_cmd_law(q_des, qd_des, tau_ff, kp, kd, W.qj[lane], W.qvel[6 + lane]);
    if (apply) W.ctrl[lane] = u;
    if (c.act_seq) gptr(c.act_seq)[((size_t)kstep * a.n_envs + env) * 12 + lane] = u;
    if (last && J.tau_out) gptr(J.tau_out)[(size_t)env * 12 + lane] = u;
  }
}

/* the third inline policy: foot-space actions (gq_step_foot_cmd, the law: gq_foot_cmd.h), on the joint state and the base quaternion
 * load_rows has just staged in LDS.  Three phases through the `u` overlay, which is dead between load_rows and S1:
 *   lane = link (12): the link's record and its local transform -> W.u.dyn.fkloc (the words S1's first phase leaves there);
 *   lane = foot (4, FL FR RL RR): the foot's command words, the chain of its leg, tau_leg = J^T F + tau_ff -> the leg's hinges in
 *     W.u.dyn.anchor (no lane ever holds three link records next to the chain's intermediates: the persistent variants have no
 *     register to spare);
 *   lane = hinge (12): W.ctrl / act_seq / tau_out, exactly as joint_cmd_inline.
 * Fetched at every substep, nothing carried across step_wave (profiles/joint_cmd_kernel_resources.md).  W.force[0..1] are not
 * touched: they carry the clock and GQ_LIFT_DUE (force[2 .. 40) are written and read inside step_wave only: gq_boxes.h GQ_XE_MASK). */
__device__ __forceinline__ void foot_cmd_inline(const GQ_MODEL FootCmdDev& F, const GQ_MODEL GqDevModel& m, const StepArgs& a, const StepCall& c, WaveMem& W,
                                                const int env, const int kstep, const bool last, const bool apply) {
  const int lane = lane_id();
  static_assert(sizeof(W.u.dyn.fkloc[0]) == GQ_FOOT_LINK_WORDS * sizeof(float), "foot_cmd_link's words fit a row of fkloc");
  float* const tq = &W.u.dyn.anchor[0][0]; /* [12], hinge order (anchor does not overlay fkloc) */
  wave_barrier(); /* W.qj / W.qvel / W.qb were stored by other lanes (load_rows: lane = word of the row) */
  if (lane < GQ_NJ) {
    const GqDevLinkRec L = link_fetch(m, lane);
    foot_cmd_link(L, W.qj[lane], W.u.dyn.fkloc[lane]);
  }
  wave_barrier();
  if (lane < 4) {
    const int leg = m.foot_leg[lane];
    const size_t r = (size_t)env * 12 + 3 * lane, g = (size_t)env * (size_t)F.gain_stride + 3 * lane, h = (size_t)env * 12 + 3 * leg;
    FootCmd cmd;
    float foot[3], tau[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      cmd.p_des[i] = gptr(F.p_des)[r + i];
      cmd.v_des[i] = F.v_des ? gptr(F.v_des)[r + i] : 0.0f;
      cmd.f_ff[i] = F.f_ff ? gptr(F.f_ff)[r + i] : 0.0f;
      cmd.tau_ff[i] = F.tau_ff ? gptr(F.tau_ff)[h + i] : 0.0f;
      cmd.kp[i] = gptr(F.kp)[g + i]; cmd.kd[i] = gptr(F.kd)[g + i];
      foot[i] = m.foot_pos[lane][i];
    }
    foot_cmd_chain(W.u.dyn.fkloc[3 * leg], W.u.dyn.fkloc[3 * leg + 1], W.u.dyn.fkloc[3 * leg + 2], foot, &W.qvel[6 + 3 * leg], W.qb, cmd, F.frame, tau);
#pragma unroll
    for (int i = 0; i < 3; i++) tq[3 * leg + i] = tau[i];
  }
  wave_barrier();
  if (lane < 12) {
    const float u = tq[lane];
    if (apply) W.ctrl[lane] = u;
    if (c.act_seq) gptr(c.act_seq)[((size_t)kstep * a.n_envs + env) * 12 + lane] = u;
    if (last && F.tau_out) gptr(F.tau_out)[(size_t)env * 12 + lane] = u;
  }
}

/* step (+ in-kernel auto-reset).  Same-step mode: a terminated env is re-spawned by the same wavefront - reset_wave,
 * then the reset's own mj_step as a second pass through step_wave; no extra launches, but the launch lasts as long as
 * its two-pass waves.  Next-step mode: the env waits (pending flag) and spends its next launch on reset_wave + the
 * reset's mj_step instead of a user step - every wave runs exactly one mj_step per launch.
 * The body of step_kernel and of step_kernel_prim below, which differ in CVX alone (gq_step_kernel.h scene_cvx): the scenes that existed
 * before the flat self-collision scene was split keep their kernels' names, template arguments included. */
template <int SOLVER, int MODE, bool CONE, bool BOXES, bool SELF, bool PRIM, bool PERSIST, bool CVX, bool FOOT = false /* the persistent variants of
          * gq_step_foot_cmd (step_kernel_foot below): the foot-space law is their ONLY inline policy, and no other kernel holds it */>
__device__ __forceinline__ void step_kernel_body(const FusedArgs* __restrict__ A, const StepCall c) {
  const long long t_entry = (GQ_TICKSET && MODE == 1) ? cycles() : 0; /* sub-stage builds (gq_step_kernel.h GQ_TICKSET) count from here */
  const int env = wave_index() + c.env0;
  if (c.mask && !gptr(c.mask)[env]) return; /* wave-uniform */
  __shared__ WaveMem W;
#if GQ_TICKSET
  if (lane_id() == 0) W.tk_T = nullptr;
#endif
  for (int kstep = 0;;) { /* one trip, except in a persistent rollout (PERSIST variants, StepCall::n_steps; a variant of their own:
                           * merely compiling the loop in cost the single-step kernel 2.7 %) */
  StepCall ck = c;
  if constexpr (PERSIST) { /* wave-uniform */
    ck.ctrl = c.ctrl ? c.ctrl + (size_t)kstep * c.ctrl_stride : nullptr; /* NULL: inline policy (or zero control) */
    if (c.obs_seq) ck.obs_seq = c.obs_seq + (size_t)kstep * A->s.n_envs * mptr(A->s.batch)->obs_dim;
  }
  const StepCall& c = ck; /* the body below sees this step's call */
  int pass = c.first_pass;
  /* the flags and the env's rows are fetched together: one memory round trip in front of the step (a respawning env - rare -
   * throws the rows away and fetches the ones reset_wave wrote) */
  WaveCtx C;
  int hint = load_rows<SOLVER>(A->s, c, W, env, pass == 0, C);
  bool respawn = c.auto_reset == 2 && C.pend; /* wave-uniform */
  /* (the reset's own step after an explicit gq_reset: the reset kernel left word whether the lift loop is still due - load_rows put it in W.lift_due) */
  /* the inline policies (PERSIST variants).  The tag bit of the policy pointer - a kernel argument - tells them apart: the built-in PD
   * policy pays nothing for the second one.  gq_step_joint_cmd (Newton only): the env's command words are fetched here at every
   * substep, not carried through the window - the kernel has no register to spare (one carried register was 4 to 8 more scratch
   * bytes per lane in every persistent variant, re-read from there at every substep anyway); the rows stay in the L2 for the window */
  if constexpr (FOOT) { /* gq_step_foot_cmd launches these variants with its command block and nothing else (launch_variant) */
    foot_cmd_inline(*mptr(policy_foot_cmd(c.policy)), *mptr(C.model), A->s, c, W, env, kstep, kstep + 1 >= c.n_steps, !respawn);
  } else if constexpr (PERSIST) if (c.policy) { /* wave-uniform */
    bool jc = false;
    if constexpr (SOLVER == 1) jc = policy_is_joint_cmd(c.policy);
    if (jc) joint_cmd_inline(*mptr(policy_joint_cmd(c.policy)), A->s, c, W, env, kstep, kstep + 1 >= c.n_steps, !respawn);
    else pd_inline(*mptr(c.policy), A->s, c, W, env, kstep, !respawn);
  }
  for (;;) { /* one call site each for reset_wave / step_wave: both are large and fully inlined */
    if (respawn) {
      wave_priority(3); /* reset + step in one launch: this wave is the longest of its SIMD */
      wave_barrier();   /* the rows just staged in LDS are dead: reset_wave reuses the region */
      reset_wave<BOXES, PRIM>(A->r, W, c.env0);
      pass = c.auto_reset;
      hint = load_rows<SOLVER>(A->s, c, W, env, false, C, true);
    }
    const int term = step_wave<SOLVER, MODE, CONE, BOXES, SELF, PRIM, false, CVX>(A->s, c, W, pass, hint, C, t_entry);
    if constexpr (FOOT) { /* the window's OR of `terminated`, as for gq_step_joint_cmd below */
      const int t = pass == 0 ? term : 0;
      if (kstep == 0 || t) { /* wave-uniform */
        uint8_t* const any = mptr(policy_foot_cmd(c.policy))->term_any;
        if (any && lane_id() == 0) gptr(any)[env] = (uint8_t)t;
      }
    } else
    if constexpr (PERSIST && SOLVER == 1) { /* gq_step_joint_cmd: the window's OR of `terminated`, kept in memory - stored by the first
                                             * substep, set by a later one that terminates (a re-spawn's own step reports none) */
      const int t = pass == 0 ? term : 0;
      if ((kstep == 0 || t) && policy_is_joint_cmd(c.policy)) { /* wave-uniform; an ordinary substep stops at the first test */
        uint8_t* const any = mptr(policy_joint_cmd(c.policy))->term_any;
        if (any && lane_id() == 0) gptr(any)[env] = (uint8_t)t;
      }
    }
    if (pass != 0 || c.auto_reset != 1 || !term) break;
    respawn = true;
  }
  if (!PERSIST || ++kstep >= c.n_steps) break;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); /* the next step reads the rows this one stored (same wave, same addresses) */
  wave_barrier();
  }
}

}  // namespace gq
