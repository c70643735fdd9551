/* TEST INFRASTRUCTURE - runs the unmodified step kernels under the host SIMT emulator: their driver gq::step_kernel_body
 * (csrc/gq_step_driver.h: the persistent step loop, the re-spawn loop, the inline policies) around the step itself (csrc/gq_step_body.h), one
 * wavefront after the other.  Two C entry points over host memory: emu_step, the instrumented kernel (mode 1) with the tensors of gq_step,
 * and emu_step_window, the production kernels (mode 0) as launch_variant (csrc/gq_kernels.hip) picks them - single step, persistent window,
 * foot-space window.  Both take the caller's dynamics and contact rows (gq_batch_set_outputs) as two trailing arrays, so the kernels' own
 * row-writing code runs emulated in either variant.  The argument blocks are filled by the library's gq_step_call.h; the instantiation comes from its step_key /
 * for_variant / kernel_cvx (gq_step_kernel.h).  Not here: the mailbox side and the policy kernels, whose protocol needs concurrent wavefronts. */
#include <functional>
#include <vector>
#include <cstdio>

#include "gq_device.h"          /* the emulator shim (this directory comes first on the include path) */
#include "gq_step_call.h"
#include "gq_step_driver.h"
#include "emu_model.h"
#include "hfield_probe.h"
#include <cstring>

void emu_run_wave(unsigned block, unsigned nblocks, const std::function<void()>& body);

/* the convex pair exchange (gq_exchange.h) under emulation: wavefronts run one after the other, so an owner ends up claiming its own items -
 * every queue operation is exercised, concurrency is not (tests/test_gpu_parity.py compares exchange on / off on the device) */
static int g_emu_xq_on = 0;
extern "C" void emu_set_exchange(int on) { g_emu_xq_on = on; }
extern "C" void emu_exchange_stats(int* out) { out[0] = gq::g_emu_cas_ok; out[1] = out[2] = out[3] = 0; }

/* the emulator's batch has neither resampling nor a step-time height map, and no solver-load hint; dyn / contacts: the caller's rows of
 * gq_batch_set_outputs ([N][GQ_DYN_STRIDE] / [N][GQ_CON_STRIDE] floats), or NULL */
static gq::BatchPtrs emu_ptrs(EmuModel& m, GqDevBatch* B, float* friction_next, uint8_t* pending, uint8_t* lift_pending, float* imu_bias,
                              float* dyn = nullptr, float* contacts = nullptr) {
  gq::BatchPtrs p{};
  p.model = &m.M; p.batch = B; p.vx = m.vx.data(); p.vy = m.vy.data(); p.vz = m.vz.data();
  p.friction_next = friction_next; p.pending = pending; p.lift_pending = lift_pending; p.imu_bias = imu_bias;
  p.dyn = dyn; p.contacts = contacts;
  return p;
}

/* What the two step entries share: the model, the batch (both kept across calls, with the batch's own memory) and the argument block of a
 * launch over the caller's host tensors.  Returns the model, NULL on error; *obs_dim: floats per observation row. */
static const GqDevModel* emu_bind(const GqModelDesc* desc, int n_envs, const int32_t* obs_ids, int n_obs, const int32_t* legs_order, int debug_envs,
                                  const GqState& st, const GqObsOut& out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed,
                                  float* friction_next, const GqImuCfg* imu, float* imu_bias, uint8_t* pending, uint8_t* lift_pending,
                                  float* dyn, float* contacts, gq::FusedArgs* f, int* obs_dim, char* err, int errlen) {
  static EmuModel m;
  static GqDevBatch B;
  if (emu_build_model(desc, m, err, errlen)) return nullptr;
  const GqDevModel& M = m.M;
  if (gq_build_dev_batch(n_envs, obs_ids, n_obs, legs_order, &B, err, (size_t)errlen)) return nullptr;
  B.debug_envs = debug_envs;
  if (imu) gq_fill_imu(&B, imu);
  static std::vector<int32_t> xq;
  static std::vector<float> sepc; /* the separating-axis cache (GqDevBatch::sepc): kept across calls like the batch's own */
  if (M.ncvx_self > 0) {
    if (sepc.size() != (size_t)n_envs * M.ncvx_self * 3) sepc.assign((size_t)n_envs * M.ncvx_self * 3, 0.0f);
    B.sepc = sepc.data(); B.sepc_stride = M.ncvx_self * 3;
  }
  if (g_emu_xq_on && M.ncvx_self > 0) {
    const int slots = 256;
    if (xq.empty()) xq.assign((size_t)slots * (1 + GQ_XQ_ITEM), 0);
    B.xq = xq.data(); B.xq_slots = slots;
  }
  const gq::BatchPtrs p = emu_ptrs(m, &B, friction_next, pending, lift_pending, imu ? imu_bias : nullptr, dyn, contacts);
  *f = gq::FusedArgs{};
  gq::fill_step_args(&f->s, p, M, n_envs, st, out, episode, lift_failed);
  if (auto_reset) gq::fill_reset_args(&f->r, p, B.rs_cmd_reset, auto_reset, st, out, episode, lift_failed);
  *obs_dim = B.obs_dim;
  return &M;
}
/* a launch with grid = n_envs: the wavefronts one after the other (a masked env's returns at once, as on the device) */
template <class Kernel>
static void emu_launch(int n_envs, Kernel&& kernel) {
  for (int e = 0; e < n_envs; e++) emu_run_wave((unsigned)e, (unsigned)n_envs, kernel);
}

/* gq_step with the inspection record: the instrumented variant of the model's key (mode 1), whether or not a record is asked for */
extern "C" int emu_step(const GqModelDesc* desc, int n_envs, const int32_t* obs_ids, int n_obs, const int32_t* legs_order,
                        const float* ctrl, const uint8_t* mask, double* qpos, float* qvel, float* qacc, float* warm,
                        float* applied, float* time, float* friction, float* cmd, float* obs,
                        float* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* invalid_contact,
                        int32_t* step_num, float* debug, int debug_envs, const GqResetCfg* auto_reset, int32_t* episode,
                        uint8_t* lift_failed, float* friction_next, int first_pass, const GqImuCfg* imu, float* imu_bias,
                        uint8_t* pending, uint8_t* lift_pending, char* err, int errlen, float* dyn, float* contacts) {
  gq::FusedArgs f;
  int obs_dim = 0;
  const GqDevModel* const M = emu_bind(desc, n_envs, obs_ids, n_obs, legs_order, debug_envs, GqState{qpos, qvel, qacc, warm, applied, time, friction, cmd},
                                       GqObsOut{obs, reward, terminated, truncated, invalid_contact, step_num, nullptr, nullptr}, auto_reset, episode, lift_failed,
                                       friction_next, imu, imu_bias, pending, lift_pending, dyn, contacts, &f, &obs_dim, err, errlen);
  if (!M) return -1;
  gq::StepCall call{};
  call.ctrl = ctrl; call.mask = mask; call.debug = debug; call.auto_reset = gq::auto_reset_mode(auto_reset); call.first_pass = first_pass;
  const bool known = gq::for_variant(gq::step_key(M->solver, M->cone, gq::model_scene(*M), true, 0, 0), [&](auto S, auto MODE, auto CONE, auto SC, auto MB) {
    if constexpr (MODE != 1 || MB != 0) return false;
    else {
      constexpr gq::Scene sc = gq::Scene(int(SC));
      emu_launch(n_envs, [&]() { gq::step_kernel_body<S, 1, CONE != 0, gq::scene_boxes(sc), gq::scene_self(sc), gq::scene_prim(sc), false, gq::kernel_cvx(sc)>(&f, call); });
      return true;
    }
  });
  if (!known) { std::snprintf(err, (size_t)errlen, "emu_step: no step-kernel variant for solver %d cone %d", M->solver, M->cone); return -1; }
  return obs_dim;
}

/* The production launches (mode 0), as launch_variant (csrc/gq_kernels.hip) makes them: with n_steps > 1 or a policy the PERSIST variant - for
 * a foot-space policy the FOOT variant - otherwise the single-step kernel with n_steps = 1.  Takes what a StepCall of gq_step, gq_rollout,
 * gq_rollout_closed (inline mode), gq_step_joint_cmd and gq_step_foot_cmd carries: ctrl [n_steps][n_envs][12] rows ctrl_stride floats apart (or
 * NULL), obs_seq, act_seq, and policy: NULL, or a block of the kind policy_kind names - 0 PolicyPdDev, 1 JointCmdDev, 2 FootCmdDev - which is
 * tagged here with the library's policy_tag_*; a JointCmdDev or FootCmdDev needs the Newton solver, as in the library (persistent_ok).
 * Every key's variants are built in: the emulator's build takes 80 s with them against 45 s without (profiles/step_driver_move.md). */
extern "C" int emu_step_window(const GqModelDesc* desc, int n_envs, const int32_t* obs_ids, int n_obs, const int32_t* legs_order,
                               const float* ctrl, const uint8_t* mask, double* qpos, float* qvel, float* qacc, float* warm,
                               float* applied, float* time, float* friction, float* cmd, float* obs,
                               float* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* invalid_contact,
                               int32_t* step_num, const GqResetCfg* auto_reset, int32_t* episode,
                               uint8_t* lift_failed, float* friction_next, int first_pass, const GqImuCfg* imu, float* imu_bias,
                               uint8_t* pending, uint8_t* lift_pending, int ctrl_stride, int n_steps, float* obs_seq, float* act_seq,
                               int policy_kind, const void* policy, char* err, int errlen, float* dyn, float* contacts) {
  gq::FusedArgs f;
  int obs_dim = 0;
  const GqDevModel* const M = emu_bind(desc, n_envs, obs_ids, n_obs, legs_order, 0, GqState{qpos, qvel, qacc, warm, applied, time, friction, cmd},
                                       GqObsOut{obs, reward, terminated, truncated, invalid_contact, step_num, nullptr, nullptr}, auto_reset, episode, lift_failed,
                                       friction_next, imu, imu_bias, pending, lift_pending, dyn, contacts, &f, &obs_dim, err, errlen);
  if (!M) return -1;
  gq::StepCall call{};
  call.ctrl = ctrl; call.mask = mask; call.auto_reset = gq::auto_reset_mode(auto_reset); call.first_pass = first_pass;
  call.ctrl_stride = ctrl_stride; call.n_steps = n_steps; call.obs_seq = obs_seq; call.act_seq = act_seq;
  if (policy) {
    if (policy_kind == 0) call.policy = static_cast<const gq::PolicyPdDev*>(policy);
    else if (policy_kind == 1) call.policy = gq::policy_tag_joint_cmd(static_cast<const gq::JointCmdDev*>(policy));
    else if (policy_kind == 2) call.policy = gq::policy_tag_foot_cmd(static_cast<const gq::FootCmdDev*>(policy));
    else { std::snprintf(err, (size_t)errlen, "emu_step_window: policy_kind %d", policy_kind); return -1; }
    if (policy_kind != 0 && M->solver != 1) { std::snprintf(err, (size_t)errlen, "emu_step_window: policy_kind %d needs the Newton solver", policy_kind); return -1; }
  }
  const bool known = gq::for_variant(gq::step_key(M->solver, M->cone, gq::model_scene(*M), false, 0, 0), [&](auto S, auto MODE, auto CONE, auto SC, auto MB) {
    if constexpr (MODE != 0 || MB != 0) return false;
    else {
      constexpr gq::Scene sc = gq::Scene(int(SC));
      constexpr bool C = CONE != 0, B = gq::scene_boxes(sc), SF = gq::scene_self(sc), P = gq::scene_prim(sc), CVX = gq::kernel_cvx(sc);
      if (call.n_steps > 1 || call.policy) {
        if constexpr (S == 1) if (gq::policy_is_foot_cmd(call.policy)) {
          emu_launch(n_envs, [&]() { gq::step_kernel_body<1, 0, C, B, SF, P, true, CVX, true>(&f, call); });
          return true;
        }
        emu_launch(n_envs, [&]() { gq::step_kernel_body<S, 0, C, B, SF, P, true, CVX>(&f, call); });
        return true;
      }
      call.n_steps = 1;
      emu_launch(n_envs, [&]() { gq::step_kernel_body<S, 0, C, B, SF, P, false, CVX>(&f, call); });
      return true;
    }
  });
  if (!known) { std::snprintf(err, (size_t)errlen, "emu_step_window: no step-kernel variant for solver %d cone %d", M->solver, M->cone); return -1; }
  return obs_dim;
}
/* sizes of the policy blocks, for the ctypes mirrors of tests/helpers.py: PolicyPdDev, JointCmdDev, FootCmdDev */
extern "C" void emu_policy_sizes(int* out) { out[0] = (int)sizeof(gq::PolicyPdDev); out[1] = (int)sizeof(gq::JointCmdDev); out[2] = (int)sizeof(gq::FootCmdDev); }

extern "C" int emu_reset(const GqModelDesc* desc, int n_envs, const uint8_t* mask, const double* qpos_new, const float* qvel_new,
                         const GqResetCfg* cfg, double* qpos, float* qvel, float* qacc, float* warm, float* applied,
                         float* time, float* cmd, float* friction_next, int32_t* step_num, int32_t* episode,
                         uint8_t* lift_failed, uint8_t* lift_pending, char* err, int errlen) {
  static EmuModel m;
  if (emu_build_model(desc, m, err, errlen)) return -1;
  const gq::BatchPtrs p = emu_ptrs(m, nullptr, friction_next, nullptr, lift_pending, nullptr);
  const GqState st{qpos, qvel, qacc, warm, applied, time, /* friction */ nullptr, cmd};
  GqObsOut out{}; out.step_num = step_num;
  gq::ResetArgs a{};
  gq::fill_reset_args(&a, p, 0, cfg, st, out, episode, lift_failed);
  a.mask = mask; a.qpos_new = qpos_new; a.qvel_new = qvel_new; a.lift_pending = p.lift_pending; /* as gq_reset (no flags to clear here) */
  a.friction_next = friction_next; /* this entry point takes no friction tensor and always wants the draw */
  const bool boxes = gq::scene_boxes(gq::model_scene(m.M));
  for (int e = 0; e < n_envs; e++) {
    if (mask && !mask[e]) continue;
    emu_run_wave((unsigned)e, (unsigned)n_envs, [&]() { /* as gq::reset_kernel */
      __shared__ gq::WaveMem W;
      if (boxes) gq::reset_wave<true>(a, W); else gq::reset_wave<false>(a, W);
    });
  }
  return 0;
}

/* the kernel's pair routines (csrc/gq_pairs.h) called directly, for a side-by-side with the oracle's restatement
 * (tests/test_kernel_emulated.py::test_pair_routines_kernel_equals_oracle): out = n x [dist, pos[3], nrm[3]] */
extern "C" int emu_capsule_box(const float* p0, const float* p1, float r, const float* bc, const float* bR, const float* bh, float margin, float* out) {
  gq::PairHit H;
  gq::capsule_box(gq::v3(p0[0], p0[1], p0[2]), gq::v3(p1[0], p1[1], p1[2]), r, gq::v3(bc[0], bc[1], bc[2]), bR, gq::v3(bh[0], bh[1], bh[2]), margin, H);
  for (int q = 0; q < H.n; q++) { out[7 * q] = H.dist[q]; out[7 * q + 1] = H.pos[q].x; out[7 * q + 2] = H.pos[q].y; out[7 * q + 3] = H.pos[q].z; out[7 * q + 4] = gq::hit_nrm(H, q).x; out[7 * q + 5] = gq::hit_nrm(H, q).y; out[7 * q + 6] = gq::hit_nrm(H, q).z; }
  return H.n;
}
extern "C" int emu_box_box(const float* ca, const float* Ra, const float* ha, const float* cb, const float* Rb, const float* hb, float margin, float* out) {
  gq::PairHit H;
  gq::box_box(gq::v3(ca[0], ca[1], ca[2]), Ra, gq::v3(ha[0], ha[1], ha[2]), gq::v3(cb[0], cb[1], cb[2]), Rb, gq::v3(hb[0], hb[1], hb[2]), margin, H);
  for (int q = 0; q < H.n; q++) { out[7 * q] = H.dist[q]; out[7 * q + 1] = H.pos[q].x; out[7 * q + 2] = H.pos[q].y; out[7 * q + 3] = H.pos[q].z; out[7 * q + 4] = gq::hit_nrm(H, q).x; out[7 * q + 5] = gq::hit_nrm(H, q).y; out[7 * q + 6] = gq::hit_nrm(H, q).z; }
  return H.n;
}
/* the kernel's height-field routines (csrc/gq_boxes.h: closest_on_triangle, hf_triangle_under, sphere_hfield) called directly, one case
 * after the other through the bodies the GPU probe launches (tests/device_probe/hfield_probe.h: argument layouts there) */
extern "C" int emu_closest_on_triangle(const float* in, int n, float* out, int32_t* interior) {
  for (int i = 0; i < n; i++) hfprobe::hfp_triangle_case(i, in, out, interior);
  return 0;
}
extern "C" int emu_sphere_hfield(const double* grid, const float* raw, const double* base, const float* q, int n, int32_t* hit, float* out, float* under) {
  static GqDevModel M;
  std::vector<float> heights;
  memset(&M, 0, sizeof M);
  hfprobe::hfp_fill(M, grid, raw, heights);
  M.hf_data = heights.data();
  for (int i = 0; i < n; i++) hfprobe::hfp_sphere_case(i, M, base, q, hit, out, under);
  return 0;
}
/* the kernel's convex routine (csrc/gq_convex.h: GJK + EPA, one wavefront per pair) called directly on two shapes - vertex clouds (h = NULL)
 * or analytic boxes (V = NULL) - for a side-by-side with the oracle's restatement: out = dist, pos[3], nrm[3] */
extern "C" int emu_convex(const float* VA, int na, const float* hA, const float* RA, const float* tA, float rA,
                          const float* VB, int nb, const float* hB, const float* RB, const float* tB, float rB, float margin, float* out) {
  std::vector<float> vx, vy, vz;
  for (int i = 0; i < na; i++) { vx.push_back(VA[3 * i]); vy.push_back(VA[3 * i + 1]); vz.push_back(VA[3 * i + 2]); }
  for (int i = 0; i < nb; i++) { vx.push_back(VB[3 * i]); vy.push_back(VB[3 * i + 1]); vz.push_back(VB[3 * i + 2]); }
  if (vx.empty()) { vx.push_back(0); vy.push_back(0); vz.push_back(0); }
  static float shp[GQ_CVX_SHP_WORDS], poly[GQ_CVX_POLY_WORDS];
  int hit = 0;
  emu_run_wave(0, 1, [&]() {
    gq::CvxShape A, B;
    A.kind = VA ? 0 : 1; A.adr = 0; A.num = na; A.pm = -1; A.r = rA; A.t = gq::v3(tA[0], tA[1], tA[2]); A.h = hA ? gq::v3(hA[0], hA[1], hA[2]) : gq::v3(0, 0, 0);
    B.kind = VB ? 0 : 1; B.adr = na; B.num = nb; B.pm = -1; B.r = rB; B.t = gq::v3(tB[0], tB[1], tB[2]); B.h = hB ? gq::v3(hB[0], hB[1], hB[2]) : gq::v3(0, 0, 0);
    for (int i = 0; i < 9; i++) { A.R[i] = RA[i]; B.R[i] = RB[i]; }
    gq::cvx_shape_store(shp, A); gq::cvx_shape_store(shp + GQ_CVX_SHAPE_WORDS, B);
    gq::wave_barrier();
    const bool h = gq::cvx_pair_wave(shp, poly, vx.data(), vy.data(), vz.data(), margin);
    if (gq::lane_id() == 0) hit = h ? 1 : 0;
  });
  if (hit) { const float* o = shp + 2 * GQ_CVX_SHAPE_WORDS; out[0] = o[0]; out[1] = o[4]; out[2] = o[5]; out[3] = o[6]; out[4] = o[1]; out[5] = o[2]; out[6] = o[3]; }
  return hit;
}
