/* TEST INFRASTRUCTURE - runs the unmodified step kernel body (csrc/gq_step_body.h) under the host SIMT emulator.
 * Exposes a C entry point with the same tensors as gq_step, operating on host memory.  The argument blocks are filled by the library's
 * gq_step_call.h and the instantiation is picked by its step_key / for_variant (gq_step_kernel.h).  The re-spawn loop around step_wave is
 * still written out here: shared with gq::step_kernel as a function it changed the instruction streams of that kernel's variants. */
#include <functional>
#include <vector>
#include <cstdio>

#include "gq_device.h"          /* the emulator shim (this directory comes first on the include path) */
#include "gq_step_call.h"
#include "emu_model.h"
#include "hfield_probe.h"
#include <cstring>

void emu_run_wave(unsigned block, unsigned nblocks, const std::function<void()>& body);

/* the convex pair exchange (gq_exchange.h) under emulation: wavefronts run one after the other, so an owner ends up claiming its own items -
 * every queue operation is exercised, concurrency is not (tests/test_gpu_parity.py compares exchange on / off on the device) */
static int g_emu_xq_on = 0;
extern "C" void emu_set_exchange(int on) { g_emu_xq_on = on; }
extern "C" void emu_exchange_stats(int* out) { out[0] = gq::g_emu_cas_ok; out[1] = out[2] = out[3] = 0; }

/* the emulator's batch has neither resampling, a step-time height map nor dyn / contact rows, and no solver-load hint */
static gq::BatchPtrs emu_ptrs(EmuModel& m, GqDevBatch* B, float* friction_next, uint8_t* pending, uint8_t* lift_pending, float* imu_bias) {
  gq::BatchPtrs p{};
  p.model = &m.M; p.batch = B; p.vx = m.vx.data(); p.vy = m.vy.data(); p.vz = m.vz.data();
  p.friction_next = friction_next; p.pending = pending; p.lift_pending = lift_pending; p.imu_bias = imu_bias;
  return p;
}

extern "C" int emu_step(const GqModelDesc* desc, int n_envs, const int32_t* obs_ids, int n_obs, const int32_t* legs_order,
                        const float* ctrl, const uint8_t* mask, double* qpos, float* qvel, float* qacc, float* warm,
                        float* applied, float* time, float* friction, float* cmd, float* obs,
                        float* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* invalid_contact,
                        int32_t* step_num, float* debug, int debug_envs, const GqResetCfg* auto_reset, int32_t* episode,
                        uint8_t* lift_failed, float* friction_next, int first_pass, const GqImuCfg* imu, float* imu_bias,
                        uint8_t* pending, uint8_t* lift_pending, char* err, int errlen) {
  static EmuModel m;
  static GqDevBatch B;
  if (emu_build_model(desc, m, err, errlen)) return -1;
  const GqDevModel& M = m.M;
  if (gq_build_dev_batch(n_envs, obs_ids, n_obs, legs_order, &B, err, (size_t)errlen)) return -1;
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
  const gq::BatchPtrs p = emu_ptrs(m, &B, friction_next, pending, lift_pending, imu ? imu_bias : nullptr);
  const GqState st{qpos, qvel, qacc, warm, applied, time, friction, cmd};
  const GqObsOut out{obs, reward, terminated, truncated, invalid_contact, step_num, nullptr, nullptr};
  gq::FusedArgs f{};
  gq::fill_step_args(&f.s, p, M, n_envs, st, out, episode, lift_failed);
  if (auto_reset) gq::fill_reset_args(&f.r, p, B.rs_cmd_reset, auto_reset, st, out, episode, lift_failed);
  gq::StepCall call{};
  call.ctrl = ctrl; call.mask = mask; call.debug = debug; call.auto_reset = gq::auto_reset_mode(auto_reset); call.first_pass = first_pass;
  /* the instrumented variant of the model's key (mode 1: the one with the debug record), whether or not a record is asked for */
  const bool known = gq::for_variant(gq::step_key(M.solver, M.cone, gq::model_scene(M), true, 0, 0), [&](auto S, auto MODE, auto CONE, auto SC, auto MB) {
    if constexpr (MODE != 1 || MB != 0) return false;
    else {
      constexpr gq::Scene sc = gq::Scene(int(SC));
      for (int e = 0; e < n_envs; e++) {
        if (mask && !mask[e]) continue;
        emu_run_wave((unsigned)e, (unsigned)n_envs, [&]() { /* the loop of gq::step_kernel (csrc/gq_kernels.hip), kept in step with it by hand */
          constexpr bool BOXES = gq::scene_boxes(sc), SELF = gq::scene_self(sc), PRIM = gq::scene_prim(sc);
          __shared__ gq::WaveMem W;
          gq::WaveCtx C;
          int pass = call.first_pass;
          int hint = gq::load_rows<S>(f.s, call, W, e, pass == 0, C);
          bool respawn = call.auto_reset == 2 && C.pend;
          for (;;) {
            if (respawn) {
              gq::wave_barrier();
              gq::reset_wave<BOXES, PRIM>(f.r, W);
              pass = call.auto_reset;
              hint = gq::load_rows<S>(f.s, call, W, e, false, C, true);
            }
            const int term = gq::step_wave<S, 1, CONE != 0, BOXES, SELF, PRIM>(f.s, call, W, pass, hint, C);
            if (pass != 0 || call.auto_reset != 1 || !term) break;
            respawn = true;
          }
        });
      }
      return true;
    }
  });
  if (!known) { std::snprintf(err, (size_t)errlen, "emu_step: no step-kernel variant for solver %d cone %d", M.solver, M.cone); return -1; }
  return B.obs_dim;
}

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
