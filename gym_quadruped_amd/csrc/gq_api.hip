/*
 * gq_api.hip - the C-ABI of libgq (include/gq.h): handle management, model upload, launches.
 * No torch types, no hidden synchronisation; every tensor is a caller-owned device pointer.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "gq.h"
#include "gq_host_model.h"
#include <gq_device.h>
#include "gq_step_kernel.h"
#include "gq_step_body.h"
#include "gq_foot_cmd.h"
#include "gq_policy_dev.h"
#include "gq_learn.h"
#include "gq_step_call.h"
#include "gq_camera_call.h"
#include "gq_host_res.h"

extern "C" void gq_launch_step(const gq::FusedArgs* dev_args, const gq::StepCall* c, int n_envs, int solver, int cone, gq::Scene scene, hipStream_t stream);
extern "C" void gq_launch_reset(const gq::ResetArgs* a, int n_envs, gq::Scene scene, hipStream_t stream);
extern "C" void gq_launch_jac(const GqDevModel* model, const double* qpos, int body, const double* point, float* jacp, float* jacr, int n_envs, hipStream_t stream);
extern "C" void gq_launch_camera(const GqDevModel* model, const gq::CamCall* c, const gq::CamShade* s, const gq::CamLayers* l, int n_envs, hipStream_t stream);
static_assert(GQ_CAM_NLAYER == GQ_CAM_MAXLAYER, "the pixel pass composites GQ_CAM_MAXLAYER layers");
static_assert(GQ_CLOSED_ABORT_STEP_DEADLINE == gq::MB_ABORT_STEP_DEADLINE && GQ_CLOSED_ABORT_POLICY_DEADLINE == gq::MB_ABORT_POLICY_DEADLINE &&
              GQ_CLOSED_ABORT_POLICY_ABSENT == gq::MB_ABORT_POLICY_ABSENT && GQ_CLOSED_ABORT_XCD_NO_POLICY == gq::MB_ABORT_XCD_NO_POLICY,
              "include/gq.h names the abort codes of gq_mailbox.h");
extern "C" void gq_launch_ray(const GqDevModel* model, const double* origin, const float* dir, int total, float* dist, int32_t* geom, hipStream_t stream);
extern "C" void gq_launch_heightmap(const GqDevModel* model, const double* center, int center_stride, const float* yaw, int yaw_stride, int n_envs, int rows, int cols,
                                    float dist_x, float dist_y, float* out, hipStream_t stream);

extern "C" void gq_launch_xcc_probe(int32_t* mask, hipStream_t stream);
extern "C" void gq_launch_policy_pd(const gq::MailboxDev* mb, const gq::PolicyPdDev* pd, const float* obs, int od, int waves, hipStream_t stream);
extern "C" int gq_launch_policy(const gq::MailboxDev* mb, const gq::PolicyDev* dev, const float* obs, int od, int waves, int mode, hipStream_t stream);
extern "C" void gq_launch_reward_eval(const gq::LearnFeetDev* learn, const float* rows, int od, const float* torques, const float* act, const float* act_prev,
                                      const uint8_t* terminated, const float* air_in, int n, float* out, float* air_out, int feet, hipStream_t stream);
extern "C" void gq_launch_policy_mlp_eval(const gq::PolicyDev* dev, const float* rows, int n_rows, int impl, float* out, hipStream_t stream);
extern "C" void gq_launch_policy_gru_eval(const gq::PolicyDev* dev, const float* rows, int n_rows, int impl, float* out, hipStream_t stream);
extern "C" void gq_launch_height_scan_eval(const gq::ScanLaw* law, const float* hits, const float* z, int n, int cells, float* out, hipStream_t stream);
extern "C" void gq_launch_obs_noise_eval(const gq::NoiseLaw* law, int in_obs, int cells, int in_dim, const float* rows, const int32_t* steps, const int32_t* env_ids, int n,
                                         float* out, hipStream_t stream);
extern "C" int gq_launch_mailbox_step(const gq::FusedArgs* dev_args, const gq::StepCall* c, const gq::MailboxDev* mb, int waves, int solver, int cone, gq::Scene scene, hipStream_t stream);

static thread_local char g_err[512] = "";
#define SET_ERR(...) std::snprintf(g_err, sizeof g_err, __VA_ARGS__)
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) { SET_ERR("%s: %s", #expr, hipGetErrorString(e_)); return GQ_EDEVICE; } \
  } while (0)
/* every block that carries its own size (include/gq.h: struct_size) must be there, and a binding written against another header is refused by name */
template <class T>
static bool fresh(const T* blk, const char* type, const char* who) {
  if (!blk) { SET_ERR("%s: bad argument", who); return false; }
  if (blk->struct_size == (int32_t)sizeof(T)) return true;
  SET_ERR("%s: %s.struct_size is %d, this library's struct has %d bytes: stale binding", who, type, blk->struct_size, (int)sizeof(T));
  return false;
}
/* the head gq_step_joint_cmd and gq_step_foot_cmd share: the command block is there and this library's, the batch is there, the window has a step */
template <class Cmd>
static bool cmd_window_args(const GqBatch* b, const Cmd* cmd, const char* type, int decimation, const char* who) {
  if (!fresh(cmd, type, who)) return false;
  if (!b) { SET_ERR("%s: bad argument", who); return false; }
  if (decimation < 1) { SET_ERR("%s: decimation must be >= 1 (got %d)", who, decimation); return false; }
  return true;
}

using gq::Buf;
/* every device / pinned block, stream and event below is owned by its holder (gq_host_res.h): deleting the handle frees it */
struct GqModel {
  int device;
  GqDevModel host;
  Buf<GqDevModel> dev;
  Buf<float> vx, vy, vz;
  Buf<float> hf;        /* device elevations of the scene's height field (empty: none) */
  int nvert;
  gq::Scene scene;      /* the step-kernel variants the model runs (gq_step_call.h model_scene) */
  int ngeom, ncloud;
  int32_t lg_cloud[GQ_MAXLG]; /* GqModelDesc cloud of lg[i] (gq_camera's face-plane table is indexed by cloud) */
};
/* closed-loop persistent rollout (gq_rollout_closed): mailboxes, ready queues, the policy's stream; built as a whole on first use (mailbox_setup) */
struct Mailbox {
  gq::MailboxDev host{};    /* what the device block holds: the plain pointers of the buffers below */
  Buf<float> act;
  Buf<int32_t> steps_done, issued, q_items, q_ctr, status;
  Buf<gq::MailboxDev> dev; Buf<gq::MailboxDev, gq::PinnedMem> staging;
  Buf<int32_t, gq::PinnedMem> alive, status_host; /* the word the policy workgroups count themselves into; a copy of the status words (gq_rollout_closed_status) */
  gq::Staged<gq::PolicyPdDev> policy;       /* the built-in policy's parameters (both modes read them from device memory) */
  /* the in-loop policy's block (gq_policy_dev.h): every gq_rollout_policy* call and gq_policy_mlp_eval / gq_policy_gru_eval fill the parts
   * they use and zero the others.  One ring of GQ_ARG_SLOTS slots serves all of them, where each kind of call had its own: it wraps after
   * fewer calls, and a caller that mixes them drains its stream once more often than before (Staged::push). */
  gq::Staged<gq::PolicyDev> net;
  Buf<float> held, last;                    /* [N][12] each: the action an env tracks until its next policy step; its previous policy action */
  gq::Staged<gq::LearnFeetDev> learn;       /* gq_rollout_policy_learn's / gq_reward_eval's block (its first member), and the foot terms' behind it */
  Buf<float> learn_acc, learn_prev;         /* [N], [N][12]: the reward window's sum, the policy action before the held one */
  Buf<int32_t> learn_state;                 /* [N] the window's flags (gq_learn.h LEARN_*) */
  gq::Stream stream; gq::Event fork, join;
  bool ready = false;
};
struct GqBatch {
  GqModel* model;
  GqDevBatch host;
  gq::BatchPtrs p;    /* device: the batch block and the scratch rows this batch owns, the model's blocks, the rows callers registered */
  Buf<float> friction_next; Buf<uint8_t> pending, lift_pending, load_hint; /* the scratch rows behind p */
  Buf<float> debug;     /* device, >= debug_envs * GQ_DBG_SIZE floats (lazily allocated) */
  Buf<int32_t> xq;      /* device: convex pair exchange (gq_exchange.h) - models with convex self pairs only, else empty */
  int xq_slots; bool xq_on;
  Buf<float> sepc;      /* device: separating-axis cache of the convex self pairs (GqDevBatch::sepc) */
  Buf<float> cam_rec;   /* device: gq_camera's pose-pass records [N][GQ_CAM_REC] (lazily allocated, together with cam_pos) */
  Buf<double> cam_pos;  /* device: ... and camera origins [N][3] */
  Buf<float> cam_grec;  /* device: gq_camera_layered's ghost records [N][n_ghost][GQ_CAM_GREC] (lazily allocated, grown with n_ghost) */
  int stop_stage;       /* profiling aid: GQ_STOP_STAGE at batch creation */
  gq::Staged<gq::FusedArgs> args;   /* argument block of step_kernel; re-uploaded (rarely) when a launch's tensors differ: ensure_args */
  /* the batch constants (p.batch): a setter's change travels with the NEXT launch, on that launch's stream, behind what the caller has queued there (flush_batch) */
  gq::Staged<GqDevBatch> batch;
  bool batch_dirty;
  gq::Stream shard_stream[8]; gq::Event shard_event[8], fork_event; int n_shard_streams; /* gq_rollout */
  Mailbox mb;
  gq::Staged<gq::JointCmdDev> jc;   /* gq_step_joint_cmd: the call's command pointers (StepCall::policy, tagged) */
  gq::Staged<gq::FootCmdDev> fc;    /* gq_step_foot_cmd: the same for a foot-space command (tag bit 1) */
};

/* the launches must be issued with the batch's device current (the caller's stream belongs to it); restore the caller's
 * device afterwards so that a framework sharing the thread is not surprised */
struct DeviceGuard {
  int prev = -1, dev;
  explicit DeviceGuard(int d) : dev(d) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) hipSetDevice(dev); else prev = -1; }
  ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};

extern "C" {

const char* gq_last_error(void) { return g_err; }
int gq_version(void) { return GQ_ABI_VERSION; }
int gq_struct_sizes(int32_t out[8]) {
  if (!out) { SET_ERR("gq_struct_sizes: null argument"); return GQ_EINVAL; }
  out[0] = (int32_t)sizeof(GqModelDesc); out[1] = (int32_t)sizeof(GqState); out[2] = (int32_t)sizeof(GqObsOut);
  out[3] = (int32_t)sizeof(GqResetCfg); out[4] = (int32_t)sizeof(GqResampleCfg); out[5] = (int32_t)sizeof(GqImuCfg);
  out[6] = (int32_t)sizeof(GqPolicyPd); out[7] = (int32_t)sizeof(GqMailboxView);
  return GQ_OK;
}
int gq_obs_dim(int obs_id) { return gq_obs_dim_host(obs_id); }
/* create: the half-built handle sits in a local owner, so a plain HIP_TRY return frees it - with its device current, the DeviceGuard being declared first */
int gq_model_create(const GqModelDesc* desc, int device, GqModel** out) {
  if (!desc || !out) { SET_ERR("gq_model_create: null argument"); return GQ_EINVAL; }
  if (desc->struct_size != (int32_t)sizeof(GqModelDesc)) {
    SET_ERR("gq_model_create: GqModelDesc.struct_size is %d, this library (ABI %d) expects %d - header and library do not match", desc->struct_size, GQ_ABI_VERSION, (int)sizeof(GqModelDesc));
    return GQ_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { SET_ERR("no HIP device visible"); return GQ_ENODEVICE; }
  if (device < 0 || device >= ndev) { SET_ERR("device %d out of range (have %d)", device, ndev); return GQ_EINVAL; }
  DeviceGuard guard(device);
  std::unique_ptr<GqModel> m(new (std::nothrow) GqModel());   /* value-initialised */
  if (!m) return GQ_ENOMEM;
  std::vector<float> vx, vy, vz;
  if (gq_build_dev_model(desc, &m->host, &vx, &vy, &vz, g_err, sizeof g_err)) return GQ_EINVAL;
  m->device = device; m->nvert = (int)vx.size(); m->scene = gq::model_scene(m->host);
  m->ngeom = desc->ngeom; m->ncloud = desc->ncloud;
  gq::cam_lg_cloud(m->lg_cloud, m->host, desc);
  if (m->host.hf_nrow > 0) {
    std::vector<float> hf;
    gq_hfield_heights(desc, &hf);
    HIP_TRY(m->hf.ensure(hf.size(), false));
    HIP_TRY(hipMemcpy(m->hf.get(), hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice));
    m->host.hf_data = m->hf.get();
  }
  HIP_TRY(m->dev.ensure(1, false));
  HIP_TRY(hipMemcpy(m->dev.get(), &m->host, sizeof(GqDevModel), hipMemcpyHostToDevice));
  const size_t nv = vx.size(), vb = nv * sizeof(float);
  HIP_TRY(m->vx.ensure(nv, false));
  HIP_TRY(m->vy.ensure(nv, false));
  HIP_TRY(m->vz.ensure(nv, false));
  HIP_TRY(hipMemcpy(m->vx.get(), vx.data(), vb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->vy.get(), vy.data(), vb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->vz.get(), vz.data(), vb, hipMemcpyHostToDevice));
  *out = m.release();
  return GQ_OK;
}

int gq_model_destroy(GqModel* m) {
  if (m) { DeviceGuard guard(m->device); delete m; } /* the frees run with the model's device current */
  return GQ_OK;
}

int gq_batch_create(GqModel* m, int n_envs, const int32_t* obs_ids, int n_obs, const int32_t* legs_order, GqBatch** out) {
  if (!m || !out || n_envs <= 0) { SET_ERR("gq_batch_create: bad argument"); return GQ_EINVAL; }
  DeviceGuard guard(m->device);
  std::unique_ptr<GqBatch> b(new (std::nothrow) GqBatch());   /* value-initialised */
  if (!b) return GQ_ENOMEM;
  b->model = m;
  b->p.model = m->dev.get(); b->p.vx = m->vx.get(); b->p.vy = m->vy.get(); b->p.vz = m->vz.get();
  if (gq_build_dev_batch(n_envs, obs_ids, n_obs, legs_order, &b->host, g_err, sizeof g_err)) return GQ_EINVAL;
  const size_t n = (size_t)n_envs;
  HIP_TRY(b->batch.dev.ensure(1, false));
  b->p.batch = b->batch.dev.get();
  HIP_TRY(hipMemcpy(b->p.batch, &b->host, sizeof(GqDevBatch), hipMemcpyHostToDevice));
  HIP_TRY(b->friction_next.ensure(n, true));
  HIP_TRY(b->pending.ensure(n, true));
  HIP_TRY(b->lift_pending.ensure(n, true));
  HIP_TRY(b->load_hint.ensure(n, true));
  b->p.friction_next = b->friction_next.get(); b->p.pending = b->pending.get(); b->p.lift_pending = b->lift_pending.get(); b->p.load_hint = b->load_hint.get();
  if (m->host.ncvx_self > 0) { /* the pair exchange: two slots per env, rounded up to a power of two (an env publishes what it has beyond its first pair - 0.45 pairs
                                * per env-step on the benchmark's states: the table stays sparse, which is what its hashing wants) */
    int slots = 256;
    while (slots < 2 * n_envs && slots < (1 << 21)) slots <<= 1;
    HIP_TRY(b->xq.ensure((size_t)slots * (1 + GQ_XQ_ITEM), true));
    b->xq_slots = slots;
    b->xq_on = true;
    b->host.xq = b->xq.get(); b->host.xq_slots = slots;
    HIP_TRY(b->sepc.ensure(n * m->host.ncvx_self * 3, true));
    b->host.sepc = b->sepc.get(); b->host.sepc_stride = m->host.ncvx_self * 3;
    HIP_TRY(hipMemcpy(b->p.batch, &b->host, sizeof(GqDevBatch), hipMemcpyHostToDevice));
  }
  /* profiling knobs of development builds (tools/dev_build.sh defines GQ_DEV_KNOBS; tools/stage_insts.sh, stage_cuts.py): the product library
   * reads no environment variable (tests/test_host_and_abi.py checks its objects for getenv) */
#ifdef GQ_DEV_KNOBS
  { const char* s = getenv("GQ_STOP_STAGE"); b->stop_stage = s ? atoi(s) : 0; }
#else
  b->stop_stage = 0;
#endif
  HIP_TRY(b->args.dev.ensure(1, false));
  HIP_TRY(b->args.ring.ensure(GQ_ARG_SLOTS, false));
  HIP_TRY(b->batch.ring.ensure(GQ_ARG_SLOTS, false));
  HIP_TRY(b->jc.create());
  HIP_TRY(b->fc.create());
  *out = b.release();
  return GQ_OK;
}

int gq_batch_destroy(GqBatch* b) {
  if (b) { DeviceGuard guard(b->model->device); delete b; }
  return GQ_OK;
}

int gq_batch_obs_dim(const GqBatch* b) { return b ? b->host.obs_dim : GQ_EINVAL; }

int gq_batch_set_imu(GqBatch* b, const GqImuCfg* cfg, float* bias_state) {
  if (!b || !cfg || !bias_state) { SET_ERR("gq_batch_set_imu: null argument"); return GQ_EINVAL; }
  gq_fill_imu(&b->host, cfg);
  b->p.imu_bias = bias_state;
  b->batch_dirty = true; /* uploaded by the next launch, stream-ordered (ensure_args) */
  return GQ_OK;
}

int gq_batch_set_pair_exchange(GqBatch* b, int on) {
  if (!b) { SET_ERR("gq_batch_set_pair_exchange: null batch"); return GQ_EINVAL; }
  if (on && !b->xq.get()) { SET_ERR("gq_batch_set_pair_exchange: the model has no convex self pairs - nothing to exchange"); return GQ_EINVAL; }
  b->xq_on = on != 0;
  b->host.xq = b->xq_on ? b->xq.get() : nullptr; b->host.xq_slots = b->xq_on ? b->xq_slots : 0;
  b->batch_dirty = true; /* uploaded by the next launch, stream-ordered (ensure_args) */
  return GQ_OK;
}

int gq_batch_set_heightmap(GqBatch* b, int rows, int cols, float dist_x, float dist_y, float* out) {
  if (!b) { SET_ERR("gq_batch_set_heightmap: null batch"); return GQ_EINVAL; }
  if (!out) { b->p.heightmap = nullptr; b->host.hm_rows = b->host.hm_cols = 0; b->batch_dirty = true; return GQ_OK; }
  if (rows <= 0 || cols <= 0 || rows > 4096 || cols > 4096 || rows * cols > 4096 || !(dist_x > 0.0f) || !(dist_y > 0.0f)) { SET_ERR("gq_batch_set_heightmap: bad grid (%d x %d cells of %g x %g m)", rows, cols, (double)dist_x, (double)dist_y); return GQ_EINVAL; }
  if (!gq::scene_boxes(b->model->scene)) { SET_ERR("gq_batch_set_heightmap: the scene has no world boxes / height field - every ray ends on the floor plane; use gq_heightmap"); return GQ_EINVAL; }
  b->p.heightmap = out;
  b->host.hm_rows = rows; b->host.hm_cols = cols; b->host.hm_dx = dist_x; b->host.hm_dy = dist_y;
  b->batch_dirty = true; /* uploaded by the next launch, stream-ordered (ensure_args) */
  return GQ_OK;
}

int gq_batch_set_resampling(GqBatch* b, const GqResampleCfg* cfg, const GqResetCfg* cmd_cfg, int32_t* counters, float* ext_dist) {
  if (!b) { SET_ERR("gq_batch_set_resampling: null batch"); return GQ_EINVAL; }
  GqDevBatch& h = b->host;
  if (!cfg) { h.rs_cmd_reset = 0; h.rs_dist_reset = 0; b->p.h9 = nullptr; b->p.ext_dist = nullptr; }
  else {
    if (!counters || ((cfg->cmd_reset != 0) && !cmd_cfg) || ((cfg->dist_reset != 0) && !ext_dist)) {
      SET_ERR("gq_batch_set_resampling: counters (and the command knobs / wrench tensor of the enabled parts) are required"); return GQ_EINVAL;
    }
    h.rs_cmd_reset = cfg->cmd_reset != 0; h.rs_dist_reset = cfg->dist_reset != 0; h.rs_env_id_offset = cfg->env_id_offset;
    for (int k = 0; k < 6; k++) { h.rs_dist_kind[k] = cfg->dist_kind[k]; h.rs_dist_range[k][0] = cfg->dist_range[k][0]; h.rs_dist_range[k][1] = cfg->dist_range[k][1]; }
    if (cmd_cfg) {
      for (int k = 0; k < 2; k++) { h.rs_lin_vel_range[k] = cmd_cfg->lin_vel_range[k]; h.rs_ang_vel_range[k] = cmd_cfg->ang_vel_range[k]; }
      h.rs_cmd_forward = cmd_cfg->cmd_forward; h.rs_cmd_random = cmd_cfg->cmd_random; h.rs_cmd_rotate = cmd_cfg->cmd_rotate;
    }
    h.rs_seed_lo = (uint32_t)(cfg->seed & 0xffffffffu); h.rs_seed_hi = (uint32_t)(cfg->seed >> 32);
    b->p.h9 = counters; b->p.ext_dist = ext_dist;
  }
  b->batch_dirty = true; /* uploaded by the next launch, stream-ordered (ensure_args) */
  return GQ_OK;
}

int gq_batch_set_outputs(GqBatch* b, float* dyn, float* contacts) {
  if (!b) { SET_ERR("gq_batch_set_outputs: null batch"); return GQ_EINVAL; }
  b->p.dyn = dyn; b->p.contacts = contacts;   /* picked up by the next launch's argument block (ensure_args) */
  return GQ_OK;
}

int gq_contact_force(GqBatch* b, int id, float* result, void* hip_stream) {
  if (!b || !result) { SET_ERR("gq_contact_force: null argument"); return GQ_EINVAL; }
  if (!b->p.contacts) { SET_ERR("gq_contact_force: no contact rows registered (gq_batch_set_outputs)"); return GQ_EINVAL; }
  if (id < 0 || id >= GQ_CON_MAX) { SET_ERR("gq_contact_force: contact id %d out of range (0..%d)", id, GQ_CON_MAX - 1); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  /* records past an env's contact count are written as zeros by the kernel */
  HIP_TRY(hipMemcpy2DAsync(result, 6 * sizeof(float), b->p.contacts + 8 + id * GQ_CON_REC + 16, GQ_CON_STRIDE * sizeof(float), 6 * sizeof(float),
                           (size_t)b->host.n_envs, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return GQ_OK;
}

int gq_debug_enable(GqBatch* b, int n_debug_envs) {
  if (!b) return GQ_EINVAL;
  if (n_debug_envs > b->host.n_envs) n_debug_envs = b->host.n_envs;
  DeviceGuard guard(b->model->device);
  if (n_debug_envs > 0) HIP_TRY(b->debug.ensure((size_t)n_debug_envs * GQ_DBG_SIZE, true));
  b->host.debug_envs = n_debug_envs;
  b->batch_dirty = true; /* uploaded by the next launch, stream-ordered (ensure_args) */
  return GQ_OK;
}

/* batch constants changed since the last launch (gq_batch_set_resampling / _set_imu / gq_debug_enable): stream-ordered upload */
static int flush_batch(GqBatch* b, hipStream_t stream) {
  if (!b->batch_dirty) return GQ_OK;
  HIP_TRY(b->batch.push(b->host, stream, true)); /* the dirty flag is the gate: no memcmp of the block */
  b->batch_dirty = false;
  return GQ_OK;
}
/* Make the device argument block describe (st, out, episode, lift_failed[, auto-reset cfg]).  Steady state: a memcmp (Staged::push).
 * reset_cfg NULL keeps whatever auto-reset block the device holds. */
static int ensure_args(GqBatch* b, const GqState& st, const GqObsOut& out, int32_t* episode, uint8_t* lift_failed,
                       const GqResetCfg* reset_cfg, hipStream_t stream) {
  if (const int rc = flush_batch(b, stream); rc != GQ_OK) return rc;
  gq::FusedArgs want = b->args.shadow; /* a copy of the shadow, then the fields: see Staged */
  gq::fill_step_args(&want.s, b->p, b->model->host, b->host.n_envs, st, out, episode, lift_failed);
  if (reset_cfg) gq::fill_reset_args(&want.r, b->p, b->host.rs_cmd_reset, reset_cfg, st, out, episode, lift_failed);
  HIP_TRY(b->args.push(want, stream, false));
  return GQ_OK;
}

/* one launch of the step kernel over n_envs envs from c->env0: the variant follows the batch's model (solver, cone, scene); returns the launch's error */
static hipError_t launch_step_kernel(const GqBatch* b, const gq::StepCall* c, int n_envs, hipStream_t stream) {
  gq_launch_step(b->args.dev.get(), c, n_envs, b->model->host.solver, b->model->host.cone, b->model->scene, stream);
  return hipGetLastError();
}
/* the checks that several entry points share: one definition each, the entry point's name (who) in front of the text */
static bool have_tensors(const GqState& st, const GqObsOut& out) {
  return st.qpos && st.qvel && st.qacc && st.qacc_warmstart && st.time && out.obs && out.reward && out.terminated && out.truncated && out.invalid_contact && out.step_num;
}
/* what the persistent production launches (several steps per env in one launch, the policy inline) need */
static bool persistent_ok(const GqBatch* b, const GqResetCfg* auto_reset, const char* who) {
  if (auto_reset && !auto_reset->autoreset_next_step) { SET_ERR("%s needs next-step auto-reset or none", who); return false; }
  if (b->model->host.solver != 1) { SET_ERR("%s needs the Newton solver (solver = 1)", who); return false; }
  if (b->host.debug_envs > 0 || b->stop_stage != 0) { SET_ERR("%s runs the production kernel: switch the inspection record / stage cut off first", who); return false; }
  return true;
}
/* validate a launch's tensors and make the device argument block describe them (ensure_args), stream-ordered; launches nothing */
static int bind(GqBatch* b, const GqState& st, const GqObsOut& out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, hipStream_t stream,
                const char* who) {
  if (!b || !have_tensors(st, out)) { SET_ERR("%s: null tensor", who); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (auto_reset && (!episode || !st.cmd)) { SET_ERR("%s: auto-reset needs the episode counters and the command tensor", who); return GQ_EINVAL; }
  if (b->host.rs_cmd_reset && !st.cmd) { SET_ERR("%s: command resampling is on (gq_batch_set_resampling) but the state has no command tensor", who); return GQ_EINVAL; }
  return ensure_args(b, st, out, episode, lift_failed, auto_reset, stream);
}
static int step_launch(GqBatch* b, int env0, int count, const float* ctrl, const uint8_t* mask, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
                       int32_t* episode, uint8_t* lift_failed, void* hip_stream, const char* who) {
  if (b && have_tensors(st, out) && (env0 < 0 || count < 0 || env0 + count > b->host.n_envs)) { /* a missing tensor is reported first (bind) */
    SET_ERR("%s: env range [%d, %d) outside the batch of %d", who, env0, env0 + count, b->host.n_envs); return GQ_EINVAL;
  }
  const int rc = bind(b, st, out, auto_reset, episode, lift_failed, (hipStream_t)hip_stream, who);
  if (rc != GQ_OK || count == 0) return rc;
  DeviceGuard guard(b->model->device);
  gq::StepCall c{};
  c.ctrl = ctrl; c.mask = mask; c.debug = b->host.debug_envs > 0 ? b->debug.get() : nullptr; c.env0 = env0;
  c.auto_reset = gq::auto_reset_mode(auto_reset); c.first_pass = 0; c.stop_stage = b->stop_stage;
  HIP_TRY(launch_step_kernel(b, &c, count, (hipStream_t)hip_stream));
  return GQ_OK;
}

int gq_step(GqBatch* b, const float* ctrl, const uint8_t* mask, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
            int32_t* episode, uint8_t* lift_failed, void* hip_stream) {
  return step_launch(b, 0, b ? b->host.n_envs : 0, ctrl, mask, st, out, auto_reset, episode, lift_failed, hip_stream, "gq_step");
}

int gq_step_range(GqBatch* b, int env0, int count, const float* ctrl, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
                  int32_t* episode, uint8_t* lift_failed, void* hip_stream) {
  return step_launch(b, env0, count, ctrl, nullptr, st, out, auto_reset, episode, lift_failed, hip_stream, "gq_step_range");
}

int gq_rollout(GqBatch* b, const float* ctrl_seq, int n_steps, int shards, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
               int32_t* episode, uint8_t* lift_failed, float* obs_seq, void* hip_stream) {
  if (!b || !ctrl_seq || n_steps < 0) { SET_ERR("gq_rollout: bad argument"); return GQ_EINVAL; }
  /* the persistent kernel exists for the production variant only: with the inspection record or a stage cut active the rollout is
   * played as the step loop (one shard), so that the record describes the last step and the cut applies to every step */
  if (shards == 0 && (b->host.debug_envs > 0 || b->stop_stage != 0)) shards = 1;
  if (shards == 0 && auto_reset && !auto_reset->autoreset_next_step) { SET_ERR("gq_rollout: the persistent rollout (shards = 0) needs next-step auto-reset or none"); return GQ_EINVAL; }
  const hipStream_t stream = (hipStream_t)hip_stream;
  if (const int rc = bind(b, st, out, auto_reset, episode, lift_failed, stream, "gq_rollout"); rc != GQ_OK) return rc;
  DeviceGuard guard(b->model->device);
  if (shards == 0) { /* persistent: ONE launch, every wavefront plays the whole sequence of its env (StepCall::n_steps) */
    if (n_steps == 0) return GQ_OK;
    gq::StepCall c{};
    c.ctrl = ctrl_seq; c.n_steps = n_steps; c.ctrl_stride = b->host.n_envs * 12; c.obs_seq = obs_seq;
    c.auto_reset = gq::auto_reset_mode(auto_reset); c.stop_stage = b->stop_stage;
    HIP_TRY(launch_step_kernel(b, &c, b->host.n_envs, stream));
    return GQ_OK;
  }
  shards = std::clamp(shards, 1, std::min(8, b->host.n_envs));
  while (b->n_shard_streams < shards) {
    const int i = b->n_shard_streams;
    if (i == 0) HIP_TRY(hipEventCreateWithFlags(b->fork_event.put(), hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(b->shard_stream[i].put(), hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(b->shard_event[i].put(), hipEventDisableTiming));
    b->n_shard_streams = i + 1;
  }
  const int N = b->host.n_envs, od = b->host.obs_dim;
  HIP_TRY(hipEventRecord(b->fork_event.get(), stream));
  /* from here on work may sit on the library's shard streams: whatever fails, the caller's stream is made to wait for them
   * before the error is returned - the caller may free ctrl_seq / obs_seq as soon as ITS stream is done with them */
  hipError_t herr = hipSuccess;
  const char* what = "";
#define RO_TRY(x) do { if (herr == hipSuccess) { herr = (x); if (herr != hipSuccess) what = #x; } } while (0)
  for (int s = 0; s < shards; s++) RO_TRY(hipStreamWaitEvent(b->shard_stream[s].get(), b->fork_event.get(), 0));
  gq::StepCall c{};
  c.debug = b->host.debug_envs > 0 ? b->debug.get() : nullptr;
  c.auto_reset = gq::auto_reset_mode(auto_reset); c.stop_stage = b->stop_stage;
  for (int k = 0; k < n_steps && herr == hipSuccess; k++) {
    c.ctrl = ctrl_seq + (size_t)k * N * 12;
    for (int s = 0; s < shards && herr == hipSuccess; s++) {
      const int e0 = (int)((long long)s * N / shards), e1 = (int)((long long)(s + 1) * N / shards);
      c.env0 = e0;
      RO_TRY(launch_step_kernel(b, &c, e1 - e0, b->shard_stream[s].get()));
      if (obs_seq) RO_TRY(hipMemcpyAsync(obs_seq + ((size_t)k * N + e0) * od, out.obs + (size_t)e0 * od, (size_t)(e1 - e0) * od * sizeof(float), hipMemcpyDeviceToDevice, b->shard_stream[s].get()));
    }
  }
  for (int s = 0; s < shards; s++) { /* join - also on the error path (a stream that cannot even record its event is drained on the host) */
    hipError_t j = hipEventRecord(b->shard_event[s].get(), b->shard_stream[s].get());
    if (j == hipSuccess) j = hipStreamWaitEvent(stream, b->shard_event[s].get(), 0);
    if (j != hipSuccess) { (void)hipStreamSynchronize(b->shard_stream[s].get()); if (herr == hipSuccess) { herr = j; what = "joining the shard streams"; } }
  }
#undef RO_TRY
  if (herr != hipSuccess) { SET_ERR("gq_rollout: HIP error '%s' at %s", hipGetErrorString(herr), what); return GQ_EDEVICE; }
  return GQ_OK;
}

/* mailboxes, queues and the policy stream of a batch; which XCDs the device exposes (one probe launch).  Built in a local block that the batch
 * takes over when it is complete: a failed setup keeps nothing, the next call starts from scratch */
static int mailbox_setup(GqBatch* b) {
  if (b->mb.ready) return GQ_OK;
  const size_t N = (size_t)b->host.n_envs;
  Mailbox t;
  gq::MailboxDev& h = t.host;
  int qcap = 64;
  while ((size_t)qcap < N) qcap <<= 1;
  /* which XCC ids do the workgroups of this device report?  (8 on an MI355X in SPX mode; a partitioned device shows fewer) */
  Buf<int32_t> mask_dev;
  HIP_TRY(mask_dev.ensure(1, true));
  gq_launch_xcc_probe(mask_dev.get(), 0);
  int32_t mask = 0;
  HIP_TRY(hipMemcpy(&mask, mask_dev.get(), sizeof mask, hipMemcpyDeviceToHost));
  mask_dev.reset();
  if (mask == 0) { SET_ERR("gq_rollout_closed: the XCD probe saw no workgroup"); return GQ_EDEVICE; }
  int nq = 0;
  for (int x = 0; x < 16; x++) h.xcc_queue[x] = ((mask >> x) & 1) ? nq++ : 0;
  h.nq = nq; h.qcap = qcap; h.n_envs = (int)N;
  HIP_TRY(t.act.ensure(12 * N, false));
  HIP_TRY(t.steps_done.ensure(N, false));
  HIP_TRY(t.issued.ensure(N, false));
  HIP_TRY(t.q_items.ensure((size_t)nq * qcap, false));
  HIP_TRY(t.q_ctr.ensure(gq::mb_ctr_words(nq), false));
  HIP_TRY(t.status.ensure(8, true));
  HIP_TRY(t.dev.ensure(1, false));
  HIP_TRY(t.policy.create());
  HIP_TRY(t.net.create());
  HIP_TRY(t.held.ensure(12 * N, true));
  HIP_TRY(t.last.ensure(12 * N, true));
  HIP_TRY(t.learn.create());
  HIP_TRY(t.learn_acc.ensure(N, true));
  HIP_TRY(t.learn_prev.ensure(12 * N, true));
  HIP_TRY(t.learn_state.ensure(N, true));
  HIP_TRY(t.staging.ensure(1, false));
  HIP_TRY(t.alive.ensure(1, false));
  HIP_TRY(t.status_host.ensure(8, false));
  h.act = t.act.get(); h.steps_done = t.steps_done.get(); h.issued = t.issued.get(); h.q_items = t.q_items.get(); h.q_ctr = t.q_ctr.get();
  h.status = t.status.get(); h.alive = t.alive.get();
  HIP_TRY(hipStreamCreateWithFlags(t.stream.put(), hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(t.fork.put(), hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(t.join.put(), hipEventDisableTiming));
  t.ready = true;
  b->mb = std::move(t);
  return GQ_OK;
}

int gq_mailbox_get(GqBatch* b, GqMailboxView* out) {
  if (!b || !out) { SET_ERR("gq_mailbox_get: null argument"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (const int rc = mailbox_setup(b); rc != GQ_OK) return rc;
  const gq::MailboxDev& h = b->mb.host;
  out->action = h.act; out->steps_done = h.steps_done; out->queue_items = h.q_items; out->queue_counters = h.q_ctr; out->status = h.status;
  out->n_queues = h.nq; out->queue_capacity = h.qcap; out->counter_stride = GQ_MB_QSTRIDE;
  for (int x = 0; x < 16; x++) out->xcc_queue[x] = h.xcc_queue[x];
  return GQ_OK;
}

/* ---- what the closed-loop rollouts (gq_rollout_closed, gq_rollout_policy) share ---- */
/* in front of everything: the requirements of the persistent kernels, the tensors, the mailbox, the bound of the ticket counters.  The caller
 * holds the DeviceGuard. */
static int closed_begin(GqBatch* b, int n_steps, const GqState& st, const GqObsOut& out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed,
                        hipStream_t stream, const char* who) {
  if (!persistent_ok(b, auto_reset, who)) return GQ_EINVAL;
  if (const int rc = bind(b, st, out, auto_reset, episode, lift_failed, stream, who); rc != GQ_OK) return rc;
  if (const int rc = mailbox_setup(b); rc != GQ_OK) return rc;
  const int N = b->host.n_envs;
  const gq::MailboxDev& h = b->mb.host;
  /* items carry env + 1 in 24 bits, and queue tickets are 32-bit: the env-steps that pass through queue 0, which holds the most envs */
  if (!gq::mb_rollout_fits(N, h.nq, n_steps)) { /* (mb_queue_tickets against the bound) */
    SET_ERR("%s: %d envs x %d steps over %d queues overflows the 32-bit ticket counters: split the rollout", who, N, n_steps, h.nq); return GQ_EINVAL;
  }
  return GQ_OK;
}
/* the columns of the joint angles / velocities in this batch's observation row (what both built-in policies read) */
static int joint_columns(const GqBatch* b, int32_t col_q[12], int32_t col_qd[12], const char* who, const char* what) {
  const int od = b->host.obs_dim;
  for (int j = 0; j < 12; j++) {
    col_q[j] = -1; col_qd[j] = -1;
    for (int c = 0; c < od; c++) {
      const int src = b->host.obs_map[c];
      if (col_q[j] < 0 && (src == gq::OB_QPOS_JS + j || src == gq::OB_QPOS + 7 + j)) col_q[j] = c;
      if (col_qd[j] < 0 && (src == gq::OB_QVEL_JS + j || src == gq::OB_QVEL + 6 + j)) col_qd[j] = c;
    }
    if (col_q[j] < 0 || col_qd[j] < 0) { SET_ERR("%s: the %s policy reads qpos_js / qvel_js (or qpos / qvel): not in this batch's observation row", who, what); return GQ_EINVAL; }
  }
  return GQ_OK;
}
/* fresh rollout state, ordered on the caller's stream, and the device block that describes the rollout; step_waves: the grid it will get */
static int mailbox_start(GqBatch* b, int n_steps, int& step_waves, double timeout_s, float* obs_seq, float* act_seq, hipStream_t stream) {
  Mailbox& mb = b->mb;
  gq::MailboxDev& h = mb.host;
  const int N = b->host.n_envs;
  step_waves = gq::mb_step_waves(step_waves, N, h.nq);
  h.n_steps = n_steps; h.obs_seq = obs_seq; h.act_seq = act_seq;
  h.timeout_ticks = (int64_t)((timeout_s > 0.0 ? timeout_s : 5.0) * 1e8);
  HIP_TRY(hipMemsetAsync(h.steps_done, 0, sizeof(int32_t) * (size_t)N, stream));
  HIP_TRY(hipMemsetAsync(h.issued, 0, sizeof(int32_t) * (size_t)N, stream));
  HIP_TRY(hipMemsetAsync(h.q_items, 0, sizeof(int32_t) * (size_t)h.nq * h.qcap, stream));
  HIP_TRY(hipMemsetAsync(h.q_ctr, 0, sizeof(int32_t) * gq::mb_ctr_words(h.nq), stream));
  HIP_TRY(hipMemsetAsync(h.status, 0, sizeof(int32_t) * 8, stream));
  HIP_TRY(hipStreamSynchronize(stream)); /* the pinned staging block below is reused per call; a rollout is thousands of launches' worth of work */
  std::memcpy(mb.staging.get(), &h, sizeof h);
  HIP_TRY(hipMemcpyAsync(mb.dev.get(), mb.staging.get(), sizeof h, hipMemcpyHostToDevice, stream));
  return GQ_OK;
}
/* the policy must be RESIDENT before the step wavefronts take every slot of the device: it is launched first, on its own stream
 * (policy_fork, the launch, policy_resident), and awaited until each of its workgroups has reported in */
static int policy_fork(Mailbox& mb, hipStream_t stream) {
  *(volatile int32_t*)mb.alive.get() = 0;
  HIP_TRY(hipEventRecord(mb.fork.get(), stream));
  HIP_TRY(hipStreamWaitEvent(mb.stream.get(), mb.fork.get(), 0));
  return GQ_OK;
}
static int policy_resident(Mailbox& mb, int policy_waves, hipStream_t stream, const char* who) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(mb.join.get(), mb.stream.get()));
  volatile int32_t* alive = mb.alive.get();
  const auto t0 = std::chrono::steady_clock::now();
  while (*alive < policy_waves) {
    std::this_thread::yield();
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) {
      /* it cannot start: tell it to leave as soon as it does, and report */
      mb.status_host.get()[0] = gq::MB_ABORT_POLICY_ABSENT; /* pinned: the source of an asynchronous copy must outlive this frame */
      (void)hipMemcpyAsync(mb.host.status, mb.status_host.get(), sizeof(int32_t), hipMemcpyHostToDevice, stream);
      (void)hipStreamSynchronize(stream);
      (void)hipStreamSynchronize(mb.stream.get()); /* the policy kernel has left (or never ran): nothing of this call touches `alive` later */
      SET_ERR("%s: the policy kernel did not become resident within 2 s (%d of %d workgroups)", who, (int)*alive, policy_waves);
      return GQ_EDEVICE;
    }
  }
  return GQ_OK;
}
/* the stepping side; join: the caller's stream resumes when both kernels are done */
static int mailbox_steps(GqBatch* b, const GqResetCfg* auto_reset, int step_waves, bool join, hipStream_t stream, const char* who) {
  gq::StepCall c{};
  c.auto_reset = gq::auto_reset_mode(auto_reset);
  if (!gq_launch_mailbox_step(b->args.dev.get(), &c, b->mb.dev.get(), step_waves, b->model->host.solver, b->model->host.cone, b->model->scene, stream)) {
    SET_ERR("%s: no mailbox variant of the step kernel for this model in this build", who); return GQ_EINVAL;
  }
  HIP_TRY(hipGetLastError());
  if (join) HIP_TRY(hipStreamWaitEvent(stream, b->mb.join.get(), 0));
  return GQ_OK;
}

int gq_rollout_closed(GqBatch* b, int n_steps, int mode, const GqPolicyPd* pd, int policy_waves, int step_waves, double timeout_s, GqState st, GqObsOut out,
                      const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, void* hip_stream) {
  const char* const who = "gq_rollout_closed";
  if (!b || n_steps < 0 || (mode != GQ_CLOSED_MAILBOX && mode != GQ_CLOSED_INLINE)) { SET_ERR("gq_rollout_closed: bad argument"); return GQ_EINVAL; }
  if (mode == GQ_CLOSED_INLINE && !pd) { SET_ERR("gq_rollout_closed: the inline mode runs the built-in policy: pd must be given"); return GQ_EINVAL; }
  hipStream_t stream = (hipStream_t)hip_stream;
  DeviceGuard guard(b->model->device);
  if (const int rc = closed_begin(b, n_steps, st, out, auto_reset, episode, lift_failed, stream, who); rc != GQ_OK) return rc;
  if (n_steps == 0) return GQ_OK;
  const int N = b->host.n_envs, od = b->host.obs_dim;
  Mailbox& mb = b->mb;
  gq::MailboxDev& h = mb.host;
  gq::PolicyPdDev P{};
  if (pd) {
    if (const int rc = joint_columns(b, P.col_q, P.col_qd, who, "PD"); rc != GQ_OK) return rc;
    for (int j = 0; j < 12; j++) { P.kp[j] = pd->kp[j]; P.kd[j] = pd->kd[j]; P.qdes[j] = pd->q_des[j]; }
    policy_waves = gq::mb_policy_waves(policy_waves, 64, 256, h.nq); /* lane = env: by default 4096 envs get a lane each */
    P.sigma = pd->noise_sigma; P.seed_lo = (uint32_t)(pd->noise_seed & 0xffffffffu); P.seed_hi = (uint32_t)(pd->noise_seed >> 32);
    P.step0 = pd->noise_step0; P.env_id_offset = auto_reset ? auto_reset->env_id_offset : 0;
    HIP_TRY(mb.policy.push(P, stream, true)); /* sent with every call, as ever */
  }
  if (mode == GQ_CLOSED_INLINE) {
    /* the persistent rollout kernel with the policy evaluated by the stepping wavefront itself: no mailbox, no second kernel */
    HIP_TRY(hipMemsetAsync(h.status, 0, sizeof(int32_t) * 8, stream));
    gq::StepCall ci{};
    ci.n_steps = n_steps; ci.obs_seq = obs_seq; ci.act_seq = act_seq; ci.policy = mb.policy.dev.get();
    ci.auto_reset = gq::auto_reset_mode(auto_reset); ci.stop_stage = 0;
    HIP_TRY(launch_step_kernel(b, &ci, N, stream));
    return GQ_OK;
  }
  if (const int rc = mailbox_start(b, n_steps, step_waves, timeout_s, obs_seq, act_seq, stream); rc != GQ_OK) return rc;
  if (pd) {
    if (const int rc = policy_fork(mb, stream); rc != GQ_OK) return rc;
    gq_launch_policy_pd(mb.dev.get(), mb.policy.dev.get(), out.obs, od, policy_waves, mb.stream.get());
    if (const int rc = policy_resident(mb, policy_waves, stream, who); rc != GQ_OK) return rc;
  }
  return mailbox_steps(b, auto_reset, step_waves, pd != nullptr, stream, who);
}

/* the shape of the network and what the law needs, checked and copied into the seat's part of the device block: what the MLP and the
 * recurrent policy's head share.  head: the network is a GRU's head (at most GQ_GRU_HEAD_MAXL layers) - the messages then say "head" where
 * they say "network", and "cell" for whatever the input row feeds.  scan_cells: the columns of a height scan between the observation columns
 * and the last action (0: none); hist_words: the columns of an observation history behind the last action (0: none).  P.net.in_dim is the
 * INPUT ROW's width on return. */
static int net_describe(const GqPolicyMlp* mlp, gq::PolicyMlpDev& P, const char* who, const bool head, const int scan_cells, const int hist_words) {
  const char* const net = head ? "head" : "network";
  const char* const fed = head ? "cell" : "network";
  const int max_layers = head ? GQ_GRU_HEAD_MAXL : GQ_MLP_MAXL;
  if (mlp->n_layers < 1 || mlp->n_layers > max_layers) {
    if (head) SET_ERR("%s: the head has %d linear layers: 1 to %d are supported", who, mlp->n_layers, max_layers);
    else SET_ERR("%s: %d linear layers: 1 to %d are supported (3 hidden layers and the output)", who, mlp->n_layers, max_layers);
    return GQ_EINVAL;
  }
  const int in_dim = gq::policy_row_dim(mlp->in_obs, scan_cells, mlp->feed_last_action, hist_words);
  if (mlp->in_obs < 0) { SET_ERR("%s: in_obs = %d", who, mlp->in_obs); return GQ_EINVAL; }
  if (in_dim < 1 || in_dim > GQ_MLP_MAXW) { SET_ERR("%s: the %s's input has %d columns: 1 to %d are supported", who, fed, in_dim, GQ_MLP_MAXW); return GQ_EINVAL; }
  for (int l = 0; l < mlp->n_layers; l++)
    if (mlp->width[l] < 1 || mlp->width[l] > GQ_MLP_MAXW) { SET_ERR("%s: layer %d%s has %d outputs: 1 to %d are supported", who, l, head ? " of the head" : "", mlp->width[l], GQ_MLP_MAXW); return GQ_EINVAL; }
  if (mlp->width[mlp->n_layers - 1] != 12) { SET_ERR("%s: the %s has %d outputs: 12 (one per hinge) are needed", who, net, mlp->width[mlp->n_layers - 1]); return GQ_EINVAL; }
  if (mlp->activation < GQ_ACT_RELU || mlp->activation > GQ_ACT_TANH) { SET_ERR("%s: activation %d: relu (1), elu (2) or tanh (3)", who, mlp->activation); return GQ_EINVAL; }
  if (mlp->out_activation != GQ_ACT_NONE && mlp->out_activation != GQ_ACT_TANH) { SET_ERR("%s: out_activation %d: none (0) or tanh (3)", who, mlp->out_activation); return GQ_EINVAL; }
  P.net.n_layers = mlp->n_layers; P.net.in_dim = in_dim; P.net.act = mlp->activation; P.net.out_act = mlp->out_activation;
  for (int l = 0; l < GQ_MLP_MAXL; l++) P.net.width[l] = l < mlp->n_layers ? mlp->width[l] : 0;
  P.in_obs = mlp->in_obs; P.feed_last = mlp->feed_last_action ? 1 : 0; P.decimation = mlp->decimation; P.pad_ = 0; P.pad2_ = 0;
  P.shift = mlp->obs_shift; P.scale = mlp->obs_scale;
  return GQ_OK;
}
/* what every caller starts from: a copy of the staged block's shadow (see Staged) with the feature parts at fixed zeros - a call then fills
 * the ones it uses, and nothing of an earlier call's scan, history, cell or flags travels with it */
static gq::PolicyDev policy_block(const Mailbox& mb) {
  gq::PolicyDev D = mb.net.shadow;
  D.gru = gq::GruDev{}; D.episode = gq::EpisodeDev{}; D.scan = gq::ScanDev{}; D.hist = gq::HistDev{}; D.noise = gq::NoiseDev{};
  return D;
}
/* the MLP policy: the block's seat part */
static int mlp_describe(const GqPolicyMlp* mlp, gq::PolicyDev& D, const char* who, const int scan_cells = 0, const int hist_words = 0) {
  gq::PolicyMlpDev& P = D.seat;
  if (const int rc = net_describe(mlp, P, who, false, scan_cells, hist_words); rc != GQ_OK) return rc;
  if (!mlp->blob) { SET_ERR("%s: blob is null", who); return GQ_EINVAL; }
  if (mlp->blob_floats != (int64_t)gq::mlp_blob_floats(P.net)) { SET_ERR("%s: blob_floats is %lld, this network's blob has %lld", who, (long long)mlp->blob_floats, (long long)gq::mlp_blob_floats(P.net)); return GQ_EINVAL; }
  P.blob = mlp->blob;
  return GQ_OK;
}
/* the recurrent policy: `mlp` describes the cell's input row and the HEAD (its input width is gru->hidden), `gru` the cell and the blob of
 * both.  Fills the gru part's cell and blob and the seat's network part (net = the head, blob = the head's layers). */
static int gru_describe(const GqPolicyMlp* mlp, const GqPolicyGru* gru, gq::PolicyDev& D, const char* who, const int scan_cells = 0) {
  gq::PolicyMlpDev& P = D.seat;
  gq::GruDev& G = D.gru;
  if (gru->hidden < 1 || gru->hidden > GQ_GRU_MAXH) { SET_ERR("%s: hidden = %d: 1 to %d are supported", who, gru->hidden, GQ_GRU_MAXH); return GQ_EINVAL; }
  if (const int rc = net_describe(mlp, P, who, true, scan_cells, 0); rc != GQ_OK) return rc;
  if (!gru->blob) { SET_ERR("%s: GqPolicyGru.blob is null", who); return GQ_EINVAL; }
  G.cell.in_dim = P.net.in_dim; G.cell.hidden = gru->hidden; /* the row feeds the cell, the cell the head */
  P.net.in_dim = gru->hidden;
  const long long want = (long long)gq::gru_blob_floats(G.cell, P.net);
  if (gru->blob_floats != want) { SET_ERR("%s: GqPolicyGru.blob_floats is %lld, this cell and head have %lld", who, (long long)gru->blob_floats, want); return GQ_EINVAL; }
  G.blob = gru->blob; P.blob = gru->blob + gq::gru_cell_floats(G.cell);
  return GQ_OK;
}

/* ---- the reward law's block (gq_reward.h) from the C block: weights checked, columns resolved by observable in this batch's row ---- */
static int obs_column(const GqBatch* b, int canonical) {
  for (int c = 0; c < b->host.obs_dim; c++)
    if (b->host.obs_map[c] == canonical) return c;
  return -1;
}
/* the column resolver of both laws: the column of an observable, or -1 when nothing that is on reads it; a weighted term whose observable is
 * absent is refused by name (the first one of a call: ok) */
static int term_column(const GqBatch* b, const bool needed, const char* term, const int canonical, const char* obs_name, bool& ok, const char* who) {
  if (!needed) return -1;
  const int c = obs_column(b, canonical);
  if (c < 0 && ok) { SET_ERR("%s: the reward term %s reads %s: not in this batch's observation row", who, term, obs_name); ok = false; }
  return c;
}
static int reward_describe(const GqBatch* b, const GqLearn* learn, gq::RewardLaw& R, bool& on, const char* who) {
  static const char* const names[GQ_REWARD_TERMS] = {"track_lin_vel", "track_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "base_height", "torques", "joint_vel",
                                                     "power", "action_rate", "alive", "termination"};
  const float w[GQ_REWARD_TERMS] = {learn->w_track_lin_vel, learn->w_track_ang_vel, learn->w_lin_vel_z, learn->w_ang_vel_xy, learn->w_orientation, learn->w_base_height,
                                    learn->w_torques, learn->w_joint_vel, learn->w_power, learn->w_action_rate, learn->w_alive, learn->w_termination};
  on = false;
  for (int i = 0; i < GQ_REWARD_TERMS; i++) {
    if (!std::isfinite(w[i])) { SET_ERR("%s: the weight of the reward term %s is not finite", who, names[i]); return GQ_EINVAL; }
    R.w[i] = w[i];
    on = on || w[i] != 0.0f;
  }
  if (w[gq::RW_TRACK_LIN_VEL] != 0.0f && !(learn->sigma_lin > 0.0f && std::isfinite(learn->sigma_lin))) { SET_ERR("%s: sigma_lin = %g with track_lin_vel on: it must be positive", who, (double)learn->sigma_lin); return GQ_EINVAL; }
  if (w[gq::RW_TRACK_ANG_VEL] != 0.0f && !(learn->sigma_ang > 0.0f && std::isfinite(learn->sigma_ang))) { SET_ERR("%s: sigma_ang = %g with track_ang_vel on: it must be positive", who, (double)learn->sigma_ang); return GQ_EINVAL; }
  if (w[gq::RW_BASE_HEIGHT] != 0.0f && !std::isfinite(learn->base_height_target)) { SET_ERR("%s: base_height_target is not finite", who); return GQ_EINVAL; }
  R.inv_sigma_lin = w[gq::RW_TRACK_LIN_VEL] != 0.0f ? 1.0f / learn->sigma_lin : 0.0f; /* IEEE divisions, here and nowhere else: gq_reward.h */
  R.inv_sigma_ang = w[gq::RW_TRACK_ANG_VEL] != 0.0f ? 1.0f / learn->sigma_ang : 0.0f;
  R.base_height_target = w[gq::RW_BASE_HEIGHT] != 0.0f ? learn->base_height_target : 0.0f;
  R.dt = b->model->host.timestep;
  R.pad_ = 0;
  bool ok = true;
  auto col = [&](const int term, const int canonical, const char* obs_name) { return term_column(b, w[term] != 0.0f, names[term], canonical, obs_name, ok, who); };
  R.col_lin_err[0] = col(gq::RW_TRACK_LIN_VEL, gq::OB_LIN_VEL_ERR_B + 0, "base_lin_vel_err:base"); R.col_lin_err[1] = col(gq::RW_TRACK_LIN_VEL, gq::OB_LIN_VEL_ERR_B + 1, "base_lin_vel_err:base");
  R.col_ang_err_z = col(gq::RW_TRACK_ANG_VEL, gq::OB_ANG_VEL_ERR_B + 2, "base_ang_vel_err:base");
  R.col_vz = col(gq::RW_LIN_VEL_Z, gq::OB_LIN_VEL_B + 2, "base_lin_vel:base");
  R.col_wxy[0] = col(gq::RW_ANG_VEL_XY, gq::OB_ANG_VEL_B + 0, "base_ang_vel:base"); R.col_wxy[1] = col(gq::RW_ANG_VEL_XY, gq::OB_ANG_VEL_B + 1, "base_ang_vel:base");
  R.col_gxy[0] = col(gq::RW_ORIENTATION, gq::OB_GRAV_B + 0, "gravity_vector:base"); R.col_gxy[1] = col(gq::RW_ORIENTATION, gq::OB_GRAV_B + 1, "gravity_vector:base");
  R.col_z = col(gq::RW_BASE_HEIGHT, gq::OB_BASE_POS + 2, "base_pos");
  const bool need_qd = gq::reward_needs_qd(R);
  for (int j = 0; j < 12; j++) {
    R.col_qd[j] = -1;
    if (!need_qd) continue;
    int c = obs_column(b, gq::OB_QVEL_JS + j);
    if (c < 0) c = obs_column(b, gq::OB_QVEL + 6 + j);
    if (c < 0 && ok) { SET_ERR("%s: the reward term %s reads qvel_js (or qvel): not in this batch's observation row", who, w[gq::RW_JOINT_VEL] != 0.0f ? "joint_vel" : "power"); ok = false; }
    R.col_qd[j] = c;
  }
  return ok ? GQ_OK : GQ_EINVAL;
}

/* ---- the foot terms' block (gq_reward_feet.h) from the C block: parameters checked, columns resolved per CANONICAL foot (obs_map holds the
 * canonical index of every column, so legs_order is already undone) ---- */
static int foot_describe(const GqBatch* b, const GqFootReward* feet, gq::FootLaw& F, const char* who) {
  static const char* const names[GQ_FOOT_TERMS] = {"air_time", "slip", "impact", "clearance"};
  const float w[GQ_FOOT_TERMS] = {feet->w_air_time, feet->w_slip, feet->w_impact, feet->w_clearance};
  for (int i = 0; i < GQ_FOOT_TERMS; i++) {
    if (!std::isfinite(w[i])) { SET_ERR("%s: the weight of the reward term %s is not finite", who, names[i]); return GQ_EINVAL; }
    F.w[i] = w[i];
  }
  if (w[gq::FW_AIR_TIME] != 0.0f && !std::isfinite(feet->air_time_target)) { SET_ERR("%s: air_time_target is not finite with air_time on", who); return GQ_EINVAL; }
  if (!(feet->min_cmd_speed >= 0.0f && std::isfinite(feet->min_cmd_speed))) { SET_ERR("%s: min_cmd_speed = %g: it must be finite and >= 0", who, (double)feet->min_cmd_speed); return GQ_EINVAL; }
  if (w[gq::FW_IMPACT] != 0.0f && !(feet->impact_limit > 0.0f && std::isfinite(feet->impact_limit))) { SET_ERR("%s: impact_limit = %g with impact on: it must be positive and finite", who, (double)feet->impact_limit); return GQ_EINVAL; }
  if (w[gq::FW_CLEARANCE] != 0.0f && !std::isfinite(feet->clearance_target)) { SET_ERR("%s: clearance_target is not finite with clearance on", who); return GQ_EINVAL; }
  F.air_time_target = w[gq::FW_AIR_TIME] != 0.0f ? feet->air_time_target : 0.0f;
  F.min_cmd_speed2 = w[gq::FW_AIR_TIME] != 0.0f ? feet->min_cmd_speed * feet->min_cmd_speed : 0.0f; /* squared once, here */
  F.impact_limit = w[gq::FW_IMPACT] != 0.0f ? feet->impact_limit : 0.0f;
  F.clearance_target = w[gq::FW_CLEARANCE] != 0.0f ? feet->clearance_target : 0.0f;
  bool ok = true;
  auto col = [&](const bool needed, const int term, const int canonical, const char* obs_name) { return term_column(b, needed, names[term], canonical, obs_name, ok, who); };
  const bool air = w[gq::FW_AIR_TIME] != 0.0f, slip = w[gq::FW_SLIP] != 0.0f, impact = w[gq::FW_IMPACT] != 0.0f, clear = w[gq::FW_CLEARANCE] != 0.0f;
  const bool gate = gq::foot_needs_cmd(F);
  for (int i = 0; i < 4; i++) {
    F.col_c[i] = col(air || slip, air ? gq::FW_AIR_TIME : gq::FW_SLIP, gq::OB_CONTACT_STATE + i, "contact_state");
    F.col_vx[i] = col(slip || clear, slip ? gq::FW_SLIP : gq::FW_CLEARANCE, gq::OB_FEET_VEL + 3 * i + 0, "feet_vel");
    F.col_vy[i] = col(slip || clear, slip ? gq::FW_SLIP : gq::FW_CLEARANCE, gq::OB_FEET_VEL + 3 * i + 1, "feet_vel");
    F.col_fz[i] = col(impact, gq::FW_IMPACT, gq::OB_CONTACT_F + 3 * i + 2, "contact_forces");
    F.col_zb[i] = col(clear, gq::FW_CLEARANCE, gq::OB_FEET_POS_B + 3 * i + 2, "feet_pos:base");
  }
  for (int k = 0; k < 2; k++) {
    F.col_cmd_err[k] = col(gate, gq::FW_AIR_TIME, gq::OB_LIN_VEL_ERR_B + k, "base_lin_vel_err:base");
    F.col_cmd_vel[k] = col(gate, gq::FW_AIR_TIME, gq::OB_LIN_VEL_B + k, "base_lin_vel:base");
  }
  return ok ? GQ_OK : GQ_EINVAL;
}

/* ---- the height scan's block (gq_policy_scan.h) from the C block: the law's parameters checked; with a batch, the grid held to the batch's
 * base-following map and the base's z column resolved in its observation row (b null: gq_height_scan_eval, the law alone) ---- */
static int scan_describe(const GqBatch* b, const GqPolicyScan* scan, gq::ScanDev& S, const char* who) {
  if (!std::isfinite(scan->offset) || !std::isfinite(scan->clip) || !std::isfinite(scan->scale)) { SET_ERR("%s: the height scan's offset, clip and scale must be finite (got %g, %g, %g)", who, (double)scan->offset, (double)scan->clip, (double)scan->scale); return GQ_EINVAL; }
  if (!(scan->clip > 0.0f)) { SET_ERR("%s: the height scan's clip = %g: it must be positive", who, (double)scan->clip); return GQ_EINVAL; }
  if (scan->rows <= 0 || scan->cols <= 0 || scan->rows > 4096 || scan->cols > 4096 || scan->rows * scan->cols > 4096) { SET_ERR("%s: the height scan's grid is %d x %d", who, scan->rows, scan->cols); return GQ_EINVAL; }
  S.law.offset = scan->offset; S.law.clip = scan->clip; S.law.scale = scan->scale;
  S.cells = scan->rows * scan->cols; S.col_z = -1; S.pad_[0] = S.pad_[1] = S.pad_[2] = 0; S.hits = nullptr;
  if (!b) return GQ_OK;
  if (!b->p.heightmap || b->host.hm_rows <= 0) { SET_ERR("%s: the height scan reads the batch's base-following height map: none is set (gq_batch_set_heightmap; a flat scene has none)", who); return GQ_EINVAL; }
  if (b->host.hm_rows != scan->rows || b->host.hm_cols != scan->cols) { SET_ERR("%s: the height scan is %d x %d, the batch's base-following height map %d x %d", who, scan->rows, scan->cols, b->host.hm_rows, b->host.hm_cols); return GQ_EINVAL; }
  int c = obs_column(b, gq::OB_BASE_POS + 2);
  if (c < 0) c = obs_column(b, gq::OB_QPOS + 2);
  if (c < 0) { SET_ERR("%s: the height scan reads the base's z from base_pos (or qpos): not in this batch's observation row", who); return GQ_EINVAL; }
  S.col_z = c; S.hits = b->p.heightmap;
  return GQ_OK;
}

/* ---- the observation history's law (gq_policy_hist.h) from the C block, for an MLP whose scan (if any) has scan_cells cells ---- */
static int hist_describe(const GqPolicyMlp* mlp, const GqPolicyHist* hist, const int scan_cells, gq::HistLaw& H, const char* who) {
  if (hist->frames < 1) { SET_ERR("%s: the observation history has frames = %d: at least 1 is needed", who, hist->frames); return GQ_EINVAL; }
  if (hist->cols < 1 || hist->cols > mlp->in_obs) { SET_ERR("%s: the observation history's cols = %d: 1 to in_obs = %d", who, hist->cols, mlp->in_obs); return GQ_EINVAL; }
  const int f12 = mlp->feed_last_action ? 12 : 0, col0 = mlp->in_obs + scan_cells + f12;
  const long long want = (long long)col0 + (long long)hist->frames * (hist->cols + f12);
  if (hist->in_dim != want) {
    SET_ERR("%s: the observation history's in_dim = %d: in_obs + scan cells + 12 feed_last_action + frames * (cols + 12 feed_last_action) = %d + %d + %d + %d * %d = %lld", who,
            hist->in_dim, mlp->in_obs, scan_cells, f12, hist->frames, hist->cols + f12, want);
    return GQ_EINVAL;
  }
  if (want > GQ_MLP_MAXW) { SET_ERR("%s: the network's input has %lld columns with the observation history: 1 to %d are supported", who, want, GQ_MLP_MAXW); return GQ_EINVAL; }
  if (!hist->state || !hist->ctl) { SET_ERR("%s: GqPolicyHist.state (device [N][2][frames][F], in / out) or .ctl (device [N]) is null", who); return GQ_EINVAL; }
  H = gq::hist_law(hist->frames, hist->cols, f12 != 0, col0);
  return GQ_OK;
}

/* ---- the sensor noise's law (gq_policy_noise.h) from the C block, for an input row with in_obs observation columns and scan_cells scan columns.
 * The amplitudes are a device table: their values are the caller's ---- */
static int noise_describe(const GqPolicyNoise* noise, const int in_obs, const int scan_cells, gq::NoiseLaw& Z, const char* who) {
  if (noise->kind != GQ_OBS_NOISE_UNIFORM && noise->kind != GQ_OBS_NOISE_NORMAL) { SET_ERR("%s: the sensor noise's kind is %d: uniform (0) or normal (1)", who, noise->kind); return GQ_EINVAL; }
  if (noise->n_amp != in_obs) { SET_ERR("%s: the sensor noise has n_amp = %d amplitudes, the policy in_obs = %d observation columns", who, noise->n_amp, in_obs); return GQ_EINVAL; }
  if (in_obs > 0 && !noise->amp) { SET_ERR("%s: GqPolicyNoise.amp (device [n_amp]) is null", who); return GQ_EINVAL; }
  if (!(noise->scan_amp >= 0.0f) || !std::isfinite(noise->scan_amp)) { SET_ERR("%s: the sensor noise's scan_amp = %g: it must be finite and >= 0", who, (double)noise->scan_amp); return GQ_EINVAL; }
  if (noise->scan_amp != 0.0f && scan_cells == 0) { SET_ERR("%s: the sensor noise's scan_amp = %g, and the policy has no height scan", who, (double)noise->scan_amp); return GQ_EINVAL; }
  Z.amp = noise->amp; Z.kind = noise->kind == GQ_OBS_NOISE_NORMAL ? gq::OBS_NOISE_NORMAL : gq::OBS_NOISE_UNIFORM; Z.scan_amp = noise->scan_amp;
  return GQ_OK;
}

/* gru: null for the MLP (the three entry points as they were), else the recurrent policy's block (gq_rollout_policy_gru); scan: null, or the
 * height scan's block (gq_rollout_policy_scan); hist: null, or the observation history's (gq_rollout_policy_hist, the MLP alone); noise: null,
 * or the sensor noise's (gq_rollout_policy_noise) */
static int rollout_policy(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, const GqPolicyGru* gru, const GqPolicyScan* scan, const GqPolicyHist* hist, const GqPolicyNoise* noise, int policy_waves, int step_waves, double timeout_s, GqState st, GqObsOut out,
                          const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, const GqLearn* learn,
                          const GqFootReward* feet, void* hip_stream, const char* const who) {
  if (feet && !fresh(feet, "GqFootReward", who)) return GQ_EINVAL;
  if (!fresh(mlp, "GqPolicyMlp", who)) return GQ_EINVAL;
  if (gru && !fresh(gru, "GqPolicyGru", who)) return GQ_EINVAL;
  if (scan && !fresh(scan, "GqPolicyScan", who)) return GQ_EINVAL;
  if (hist && !fresh(hist, "GqPolicyHist", who)) return GQ_EINVAL;
  if (noise && !fresh(noise, "GqPolicyNoise", who)) return GQ_EINVAL;
  if (gru && hist) { SET_ERR("%s: the observation history is the MLP's: a recurrent policy has its hidden state", who); return GQ_EINVAL; }
  if (learn && !fresh(learn, "GqLearn", who)) return GQ_EINVAL;
  if (feet && !learn) { SET_ERR("%s: the foot terms continue the learn block's sum: learn is null", who); return GQ_EINVAL; }
  if (!b || n_steps < 0) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  if (mlp->in_obs > b->host.obs_dim) { SET_ERR("%s: in_obs = %d, the observation row has %d columns", who, mlp->in_obs, b->host.obs_dim); return GQ_EINVAL; }
  gq::PolicyDev PD = policy_block(b->mb);
  gq::PolicyMlpDev& P = PD.seat;
  if (scan) {
    if (const int rc = scan_describe(b, scan, PD.scan, who); rc != GQ_OK) return rc;
  }
  const int scan_cells = PD.scan.cells;
  if (hist) {
    if (const int rc = hist_describe(mlp, hist, scan_cells, PD.hist.law, who); rc != GQ_OK) return rc;
    PD.hist.state = hist->state; PD.hist.ctl = hist->ctl;
  }
  const int hist_words = hist ? gq::hist_words(PD.hist.law) : 0;
  if (gru) {
    if (const int rc = gru_describe(mlp, gru, PD, who, scan_cells); rc != GQ_OK) return rc;
    if (!gru->hidden_state) { SET_ERR("%s: GqPolicyGru.hidden_state (device [N][hidden], in / out) is null", who); return GQ_EINVAL; }
    PD.gru.hidden_state = gru->hidden_state; PD.gru.hidden_seq = gru->hidden_seq;
  } else if (const int rc = mlp_describe(mlp, PD, who, scan_cells, hist_words); rc != GQ_OK) return rc;
  if (noise) { /* (its seed, step0 and env id offset are the seat's, filled below) */
    gq::NoiseLaw Z{};
    if (const int rc = noise_describe(noise, mlp->in_obs, scan_cells, Z, who); rc != GQ_OK) return rc;
    if (noise->policy_obs_clean && !(learn && learn->policy_obs)) { SET_ERR("%s: GqPolicyNoise.policy_obs_clean is recorded next to GqLearn.policy_obs: there is none", who); return GQ_EINVAL; }
    PD.noise.amp = Z.amp; PD.noise.kind = Z.kind; PD.noise.scan_amp = Z.scan_amp; PD.noise.rec_clean = noise->policy_obs_clean;
  }
  if (mlp->decimation < 1) { SET_ERR("%s: decimation must be >= 1 (got %d)", who, mlp->decimation); return GQ_EINVAL; }
  if (n_steps % mlp->decimation != 0) { SET_ERR("%s: n_steps = %d is no multiple of decimation = %d (no held action crosses calls)", who, n_steps, mlp->decimation); return GQ_EINVAL; }
  if (const int rc = joint_columns(b, P.col_q, P.col_qd, who, gru ? "GRU" : "MLP"); rc != GQ_OK) return rc;
  gq::LearnFeetDev LF = b->mb.learn.shadow;
  gq::LearnDev& L = LF.learn;
  bool reward_on = false;
  if (learn) {
    if (const int rc = reward_describe(b, learn, L.law, reward_on, who); rc != GQ_OK) return rc;
  }
  bool feet_on = false;
  if (feet) {
    if (const int rc = foot_describe(b, feet, LF.feet, who); rc != GQ_OK) return rc;
    feet_on = gq::foot_on(LF.feet) && (learn->rewards || learn->dones); /* without a weighted foot term, or with no reward asked for, the call is gq_rollout_policy_learn's */
    if (LF.feet.w[gq::FW_AIR_TIME] != 0.0f && !feet->air_time) { SET_ERR("%s: air_time is on and GqFootReward.air_time (the state, device [N][4]) is null", who); return GQ_EINVAL; }
    LF.air_time = feet->air_time;
  }
  hipStream_t stream = (hipStream_t)hip_stream;
  DeviceGuard guard(b->model->device);
  if (const int rc = closed_begin(b, n_steps, st, out, auto_reset, episode, lift_failed, stream, who); rc != GQ_OK) return rc;
  if (n_steps == 0) return GQ_OK;
  const int N = b->host.n_envs, od = b->host.obs_dim;
  Mailbox& mb = b->mb;
  gq::MailboxDev& h = mb.host;
  /* a wavefront takes its ready envs through the network 16 at a time; a recurrent one holds 48 KB of LDS: 512 of them are resident on any device the mailbox runs on */
  policy_waves = gq::mb_policy_waves(policy_waves, 128, gru ? 512 : 1024, h.nq);
  for (int j = 0; j < 12; j++) {
    P.kp[j] = mlp->kp[j]; P.kd[j] = mlp->kd[j]; P.q_default[j] = mlp->q_default[j]; P.action_scale[j] = mlp->action_scale[j]; P.sigma[j] = mlp->noise_sigma[j];
  }
  P.clip = mlp->action_clip;
  P.seed_lo = (uint32_t)(mlp->noise_seed & 0xffffffffu); P.seed_hi = (uint32_t)(mlp->noise_seed >> 32);
  P.step0 = mlp->noise_step0; P.env_id_offset = auto_reset ? auto_reset->env_id_offset : 0;
  P.issued = h.issued; P.held = mb.held.get(); P.last = mb.last.get(); P.policy_actions = mlp->policy_actions;
  P.learn = learn ? mb.learn.dev.get() : nullptr;
  if (gru || hist) { PD.episode.terminated = out.terminated; PD.episode.pending = b->p.pending; } /* both episode rules read them */
  HIP_TRY(mb.net.push(PD, stream, true));
  HIP_TRY(hipMemsetAsync(mb.last.get(), 0, sizeof(float) * 12 * (size_t)N, stream)); /* the first policy step of a call sees zeros */
  if (learn) {
    /* the reward is evaluated when anything of it is asked for (a spec without a weighted term is a reward of zero) */
    L.has_reward = (learn->rewards || learn->dones) ? 1 : 0; L.pad_ = 0;
    L.terminated = out.terminated; L.pending = b->p.pending;
    L.acc = mb.learn_acc.get(); L.wstate = mb.learn_state.get(); L.prev = mb.learn_prev.get();
    L.rewards = learn->rewards; L.dones = learn->dones; L.policy_obs = learn->policy_obs; L.policy_means = learn->policy_means;
    HIP_TRY(mb.learn.push(LF, stream, true));
    HIP_TRY(hipMemsetAsync(L.acc, 0, sizeof(float) * (size_t)N, stream));
    HIP_TRY(hipMemsetAsync(L.wstate, 0, sizeof(int32_t) * (size_t)N, stream));
  }
  if (const int rc = mailbox_start(b, n_steps, step_waves, timeout_s, obs_seq, act_seq, stream); rc != GQ_OK) return rc;
  if (const int rc = policy_fork(mb, stream); rc != GQ_OK) return rc;
  const int mode = (feet_on ? 2 : (learn ? 1 : 0)) | (gru ? 4 : 0) | (scan ? 8 : 0) | (hist ? 16 : 0) | (noise ? 32 : 0); /* policy_mlp_kernel's MODE */
  if (!gq_launch_policy(mb.dev.get(), mb.net.dev.get(), out.obs, od, policy_waves, mode, mb.stream.get())) {
    SET_ERR("%s: no policy kernel for this combination of recurrent policy, height scan, observation history and sensor noise (mode %d)", who, mode); return GQ_EINVAL;
  }
  if (const int rc = policy_resident(mb, policy_waves, stream, who); rc != GQ_OK) return rc;
  return mailbox_steps(b, auto_reset, step_waves, true, stream, who);
}
int gq_rollout_policy_gru(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, const GqPolicyGru* gru, int policy_waves, int step_waves, double timeout_s, GqState st,
                          GqObsOut out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, const GqLearn* learn,
                          const GqFootReward* feet, void* hip_stream) {
  const char* const who = "gq_rollout_policy_gru";
  if (!gru) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  return rollout_policy(b, n_steps, mlp, gru, nullptr, nullptr, nullptr, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, learn, feet, hip_stream, who);
}
int gq_rollout_policy_scan(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, const GqPolicyGru* gru, const GqPolicyScan* scan, int policy_waves, int step_waves,
                           double timeout_s, GqState st, GqObsOut out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq,
                           float* act_seq, const GqLearn* learn, const GqFootReward* feet, void* hip_stream) {
  const char* const who = "gq_rollout_policy_scan";
  if (!scan) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  return rollout_policy(b, n_steps, mlp, gru, scan, nullptr, nullptr, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, learn, feet, hip_stream, who);
}
int gq_rollout_policy_hist(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, const GqPolicyScan* scan, const GqPolicyHist* hist, int policy_waves, int step_waves,
                           double timeout_s, GqState st, GqObsOut out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq,
                           float* act_seq, const GqLearn* learn, const GqFootReward* feet, void* hip_stream) {
  const char* const who = "gq_rollout_policy_hist";
  if (!hist) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  return rollout_policy(b, n_steps, mlp, nullptr, scan, hist, nullptr, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, learn, feet, hip_stream, who);
}
int gq_rollout_policy_noise(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, const GqPolicyGru* gru, const GqPolicyScan* scan, const GqPolicyHist* hist,
                            const GqPolicyNoise* noise, int policy_waves, int step_waves, double timeout_s, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
                            int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, const GqLearn* learn, const GqFootReward* feet, void* hip_stream) {
  const char* const who = "gq_rollout_policy_noise";
  if (!noise) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  return rollout_policy(b, n_steps, mlp, gru, scan, hist, noise, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, learn, feet, hip_stream, who);
}
int gq_rollout_policy(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, int policy_waves, int step_waves, double timeout_s, GqState st, GqObsOut out,
                      const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, void* hip_stream) {
  return rollout_policy(b, n_steps, mlp, nullptr, nullptr, nullptr, nullptr, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, nullptr, nullptr, hip_stream, "gq_rollout_policy");
}
int gq_rollout_policy_learn(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, int policy_waves, int step_waves, double timeout_s, GqState st, GqObsOut out,
                            const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, const GqLearn* learn,
                            void* hip_stream) {
  return rollout_policy(b, n_steps, mlp, nullptr, nullptr, nullptr, nullptr, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, learn, nullptr, hip_stream,
                        learn ? "gq_rollout_policy_learn" : "gq_rollout_policy");
}
int gq_rollout_policy_learn_feet(GqBatch* b, int n_steps, const GqPolicyMlp* mlp, int policy_waves, int step_waves, double timeout_s, GqState st, GqObsOut out,
                                 const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, const GqLearn* learn,
                                 const GqFootReward* feet, void* hip_stream) {
  const char* const who = "gq_rollout_policy_learn_feet";
  if (!feet) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  return rollout_policy(b, n_steps, mlp, nullptr, nullptr, nullptr, nullptr, policy_waves, step_waves, timeout_s, st, out, auto_reset, episode, lift_failed, obs_seq, act_seq, learn, feet, hip_stream, who);
}

/* gq_reward_eval (feet null) and gq_reward_eval_feet */
static int reward_eval(GqBatch* b, const GqLearn* learn, const GqFootReward* feet, const float* rows, const float* torques, const float* act, const float* act_prev,
                       const uint8_t* terminated, const float* air_in, int n, float* out, float* air_out, void* hip_stream, const char* const who) {
  if (!learn) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  if ((feet && !fresh(feet, "GqFootReward", who)) || !fresh(learn, "GqLearn", who)) return GQ_EINVAL;
  if (!b || !rows || !out || n < 0) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (const int rc = mailbox_setup(b); rc != GQ_OK) return rc;
  gq::LearnFeetDev LF = b->mb.learn.shadow;
  bool on = false;
  if (const int rc = reward_describe(b, learn, LF.learn.law, on, who); rc != GQ_OK) return rc;
  if (feet) {
    if (const int rc = foot_describe(b, feet, LF.feet, who); rc != GQ_OK) return rc;
  }
  if (gq::reward_needs_u(LF.learn.law) && !torques) { SET_ERR("%s: a weighted term reads the torques: torques is null", who); return GQ_EINVAL; }
  if (gq::reward_needs_a(LF.learn.law) && (!act || !act_prev)) { SET_ERR("%s: action_rate reads act and act_prev: null", who); return GQ_EINVAL; }
  if (feet && LF.feet.w[gq::FW_AIR_TIME] != 0.0f && (!air_in || !air_out)) { SET_ERR("%s: air_time is on: air_in and air_out (the state before and after, device [n][4]) must not be null", who); return GQ_EINVAL; }
  if (n == 0) return GQ_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(b->mb.learn.push(LF, stream, true));
  gq_launch_reward_eval(b->mb.learn.dev.get(), rows, b->host.obs_dim, torques, act, act_prev, terminated, air_in, n, out, air_out, feet != nullptr, stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}
int gq_reward_eval(GqBatch* b, const GqLearn* learn, const float* rows, const float* torques, const float* act, const float* act_prev, const uint8_t* terminated,
                   int n, float* out, void* hip_stream) {
  return reward_eval(b, learn, nullptr, rows, torques, act, act_prev, terminated, nullptr, n, out, nullptr, hip_stream, "gq_reward_eval");
}
int gq_reward_eval_feet(GqBatch* b, const GqLearn* learn, const GqFootReward* feet, const float* rows, const float* torques, const float* act, const float* act_prev,
                        const uint8_t* terminated, const float* air_in, int n, float* out, float* air_out, void* hip_stream) {
  const char* const who = "gq_reward_eval_feet";
  if (!feet) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  return reward_eval(b, learn, feet, rows, torques, act, act_prev, terminated, air_in, n, out, air_out, hip_stream, who);
}

int gq_policy_mlp_eval(GqBatch* b, const GqPolicyMlp* mlp, const float* rows, int n_rows, int impl, float* out, void* hip_stream) {
  const char* const who = "gq_policy_mlp_eval";
  if (!fresh(mlp, "GqPolicyMlp", who)) return GQ_EINVAL;
  if (!b || !rows || !out || n_rows < 0 || (impl != 0 && impl != 1)) { SET_ERR("gq_policy_mlp_eval: bad argument"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (const int rc = mailbox_setup(b); rc != GQ_OK) return rc;
  gq::PolicyDev PD = policy_block(b->mb);
  if (const int rc = mlp_describe(mlp, PD, who); rc != GQ_OK) return rc;
  if (n_rows == 0) return GQ_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(b->mb.net.push(PD, stream, true));
  gq_launch_policy_mlp_eval(b->mb.net.dev.get(), rows, n_rows, impl, out, stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_height_scan_eval(GqBatch* b, const GqPolicyScan* scan, const float* hits, const float* z, int n, float* out, void* hip_stream) {
  const char* const who = "gq_height_scan_eval";
  if (!fresh(scan, "GqPolicyScan", who)) return GQ_EINVAL;
  if (!b || !hits || !z || !out || n < 0) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  gq::ScanDev S{};
  if (const int rc = scan_describe(nullptr, scan, S, who); rc != GQ_OK) return rc;
  if (n == 0) return GQ_OK;
  DeviceGuard guard(b->model->device);
  gq_launch_height_scan_eval(&S.law, hits, z, n, S.cells, out, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_obs_noise_eval(GqBatch* b, const GqPolicyNoise* noise, int in_obs, int scan_cells, int in_dim, uint64_t noise_seed, const float* rows, const int32_t* steps,
                      const int32_t* env_ids, int n, float* out, void* hip_stream) {
  const char* const who = "gq_obs_noise_eval";
  if (!fresh(noise, "GqPolicyNoise", who)) return GQ_EINVAL;
  if (!b || !rows || !steps || !env_ids || !out || n < 0) { SET_ERR("%s: bad argument", who); return GQ_EINVAL; }
  if (in_obs < 0 || scan_cells < 0 || in_dim < 1 || in_dim > GQ_MLP_MAXW || in_obs + scan_cells > in_dim) {
    SET_ERR("%s: an input row of in_dim = %d columns (1 to %d) with in_obs = %d and %d scan cells", who, in_dim, GQ_MLP_MAXW, in_obs, scan_cells); return GQ_EINVAL;
  }
  gq::NoiseLaw Z{};
  if (const int rc = noise_describe(noise, in_obs, scan_cells, Z, who); rc != GQ_OK) return rc;
  Z.seed_lo = (uint32_t)(noise_seed & 0xffffffffu); Z.seed_hi = (uint32_t)(noise_seed >> 32);
  if (n == 0) return GQ_OK;
  DeviceGuard guard(b->model->device);
  gq_launch_obs_noise_eval(&Z, in_obs, scan_cells, in_dim, rows, steps, env_ids, n, out, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_policy_gru_eval(GqBatch* b, const GqPolicyMlp* mlp, const GqPolicyGru* gru, const float* rows, const float* h_in, int n_rows, int impl, float* out, float* h_out,
                       void* hip_stream) {
  const char* const who = "gq_policy_gru_eval";
  if (!fresh(mlp, "GqPolicyMlp", who) || !fresh(gru, "GqPolicyGru", who)) return GQ_EINVAL;
  if (!b || !rows || !h_in || !out || !h_out || n_rows < 0 || (impl != 0 && impl != 1)) { SET_ERR("gq_policy_gru_eval: bad argument"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (const int rc = mailbox_setup(b); rc != GQ_OK) return rc;
  gq::PolicyDev PD = policy_block(b->mb);
  if (const int rc = gru_describe(mlp, gru, PD, who); rc != GQ_OK) return rc;
  if (n_rows == 0) return GQ_OK;
  PD.gru.hidden_state = const_cast<float*>(h_in); PD.gru.hidden_seq = h_out; /* the kernels read the first, write the second */
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(b->mb.net.push(PD, stream, true));
  gq_launch_policy_gru_eval(b->mb.net.dev.get(), rows, n_rows, impl, out, stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

/* gq_step_joint_cmd / gq_step_foot_cmd: what both check (cmd_window_args above, before each one's own fields, and the gain layout) */
static bool cmd_gain_stride_ok(int gain_stride, const char* who) {
  if (gain_stride != 0 && gain_stride != 12) { SET_ERR("%s: gain_stride must be 0 (one row of 12) or 12 ([N][12]), got %d", who, gain_stride); return false; }
  return true;
}
/* ... and the tail: `decimation` substeps in the persistent step kernel, the law selected by the tagged pointer to its device block */
static int cmd_window_launch(GqBatch* b, int decimation, const gq::PolicyPdDev* policy, const GqResetCfg* auto_reset, float* obs_seq, float* act_seq, hipStream_t stream) {
  gq::StepCall c{};
  c.n_steps = decimation; c.obs_seq = obs_seq; c.act_seq = act_seq; c.policy = policy;
  c.auto_reset = gq::auto_reset_mode(auto_reset); c.stop_stage = 0;
  HIP_TRY(launch_step_kernel(b, &c, b->host.n_envs, stream));
  return GQ_OK;
}

int gq_step_joint_cmd(GqBatch* b, const GqJointCmd* cmd, int decimation, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
                      int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, void* hip_stream) {
  const char* const who = "gq_step_joint_cmd";
  if (!cmd_window_args(b, cmd, "GqJointCmd", decimation, who)) return GQ_EINVAL;
  if (!cmd->q_des || !cmd->kp || !cmd->kd) { SET_ERR("%s: q_des, kp and kd must be given", who); return GQ_EINVAL; }
  if (!cmd_gain_stride_ok(cmd->gain_stride, who)) return GQ_EINVAL;
  if (!persistent_ok(b, auto_reset, who)) return GQ_EINVAL;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (const int rc = bind(b, st, out, auto_reset, episode, lift_failed, stream, who); rc != GQ_OK) return rc;
  DeviceGuard guard(b->model->device);
  /* the command pointers travel in a device block of their own: uploaded, stream-ordered, only when one of them changed */
  gq::JointCmdDev J = b->jc.shadow; /* a copy of the shadow, then the fields: see Staged */
  J.q_des = cmd->q_des; J.qd_des = cmd->qd_des; J.tau_ff = cmd->tau_ff; J.kp = cmd->kp; J.kd = cmd->kd;
  J.tau_out = cmd->tau_out; J.term_any = cmd->terminated_any; J.gain_stride = cmd->gain_stride; J.pad_ = 0;
  HIP_TRY(b->jc.push(J, stream, false));
  return cmd_window_launch(b, decimation, gq::policy_tag_joint_cmd(b->jc.dev.get()), auto_reset, obs_seq, act_seq, stream);
}

int gq_step_foot_cmd(GqBatch* b, const GqFootCmd* cmd, int decimation, GqState st, GqObsOut out, const GqResetCfg* auto_reset,
                     int32_t* episode, uint8_t* lift_failed, float* obs_seq, float* act_seq, void* hip_stream) {
  const char* const who = "gq_step_foot_cmd";
  if (!cmd_window_args(b, cmd, "GqFootCmd", decimation, who)) return GQ_EINVAL;
  if (!cmd->p_des || !cmd->kp || !cmd->kd) { SET_ERR("%s: p_des, kp and kd must be given", who); return GQ_EINVAL; }
  if (!cmd_gain_stride_ok(cmd->gain_stride, who)) return GQ_EINVAL;
  if (cmd->frame != 0 && cmd->frame != 1) { SET_ERR("%s: frame must be 0 (base) or 1 (world axes), got %d", who, cmd->frame); return GQ_EINVAL; }
  if (!persistent_ok(b, auto_reset, who)) return GQ_EINVAL;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (const int rc = bind(b, st, out, auto_reset, episode, lift_failed, stream, who); rc != GQ_OK) return rc;
  DeviceGuard guard(b->model->device);
  gq::FootCmdDev F = b->fc.shadow; /* a copy of the shadow, then the fields: see Staged */
  F.p_des = cmd->p_des; F.v_des = cmd->v_des; F.f_ff = cmd->f_ff; F.tau_ff = cmd->tau_ff; F.kp = cmd->kp; F.kd = cmd->kd;
  F.tau_out = cmd->tau_out; F.term_any = cmd->terminated_any; F.gain_stride = cmd->gain_stride; F.frame = cmd->frame;
  HIP_TRY(b->fc.push(F, stream, false));
  return cmd_window_launch(b, decimation, gq::policy_tag_foot_cmd(b->fc.dev.get()), auto_reset, obs_seq, act_seq, stream);
}

int gq_rollout_closed_status(GqBatch* b, int32_t out[4], void* hip_stream) {
  if (!b || !out) { SET_ERR("gq_rollout_closed_status: null argument"); return GQ_EINVAL; }
  if (!b->mb.ready) { out[0] = out[1] = out[2] = out[3] = 0; return GQ_OK; }
  DeviceGuard guard(b->model->device);
  HIP_TRY(hipMemcpyAsync(b->mb.status_host.get(), b->mb.host.status, sizeof(int32_t) * 8, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  for (int i = 0; i < 4; i++) out[i] = b->mb.status_host.get()[i];
  if (out[0] == 0) return GQ_OK;
  char why[96];
  switch (out[0]) { /* gq_mailbox.h: the codes, and who stands in out[1] for each */
    case gq::MB_ABORT_STEP_DEADLINE: std::snprintf(why, sizeof why, "a step wavefront waited past the deadline for ticket %d", out[1]); break;
    case gq::MB_ABORT_POLICY_DEADLINE: std::snprintf(why, sizeof why, "policy lane %d waited past the deadline", out[1]); break;
    case gq::MB_ABORT_POLICY_ABSENT: std::snprintf(why, sizeof why, "policy not resident"); break;
    case gq::MB_ABORT_XCD_NO_POLICY: std::snprintf(why, sizeof why, "no policy wavefront on XCD queue %d", out[1]); break;
    default: std::snprintf(why, sizeof why, "unknown code, detail %d", out[1]); break;
  }
  SET_ERR("closed-loop rollout aborted: code %d (%s), %d env-steps were played", out[0], why, out[2]);
  return GQ_EDEVICE;
}

int gq_batch_bind(GqBatch* b, GqState st, GqObsOut out, const GqResetCfg* auto_reset, int32_t* episode, uint8_t* lift_failed, void* hip_stream) {
  return bind(b, st, out, auto_reset, episode, lift_failed, (hipStream_t)hip_stream, "gq_batch_bind");
}

int gq_reset(GqBatch* b, const uint8_t* mask, const double* qpos_new, const float* qvel_new, const GqResetCfg* cfg,
             GqState st, GqObsOut out, int32_t* episode, uint8_t* lift_failed, void* hip_stream) {
  if (!b || !cfg || !have_tensors(st, out)) { SET_ERR("gq_reset: null tensor"); return GQ_EINVAL; }
  if ((qpos_new == nullptr) != (qvel_new == nullptr)) { SET_ERR("gq_reset: qpos_new and qvel_new must be given together"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  gq::ResetArgs r{};
  gq::fill_reset_args(&r, b->p, b->host.rs_cmd_reset, cfg, st, out, episode, lift_failed);
  r.mask = mask; r.qpos_new = qpos_new; r.qvel_new = qvel_new;
  r.clear_terminated = out.terminated; r.clear_truncated = out.truncated; r.clear_invalid = out.invalid_contact;
  r.lift_pending = b->p.lift_pending;
  if (const int rc = flush_batch(b, (hipStream_t)hip_stream); rc != GQ_OK) return rc;
  gq_launch_reset(&r, b->host.n_envs, b->model->scene, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  /* the reset's own mj_step with zero control (quadruped_env.py:334, :397); friction committed after it (:403-404) */
  if (const int rc = ensure_args(b, st, out, episode, lift_failed, nullptr, (hipStream_t)hip_stream); rc != GQ_OK) return rc;
  gq::StepCall c{};
  c.mask = mask; c.first_pass = 1; c.debug = b->host.debug_envs > 0 ? b->debug.get() : nullptr;
  HIP_TRY(launch_step_kernel(b, &c, b->host.n_envs, (hipStream_t)hip_stream));
  return GQ_OK;
}

int gq_batch_set_pending(GqBatch* b, const uint8_t* flags, void* hip_stream) {
  if (!b) { SET_ERR("gq_batch_set_pending: null batch"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (flags) HIP_TRY(hipMemcpyAsync(b->p.pending, flags, (size_t)b->host.n_envs, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  else HIP_TRY(hipMemsetAsync(b->p.pending, 0, (size_t)b->host.n_envs, (hipStream_t)hip_stream));
  return GQ_OK;
}

int gq_heightmap(GqBatch* b, const double* center, const float* yaw, int rows, int cols, float dist_x, float dist_y,
                 float* out, void* hip_stream) {
  if (!b || !center || !yaw || !out || rows <= 0 || cols <= 0) { SET_ERR("gq_heightmap: bad argument"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  gq_launch_heightmap(b->model->dev.get(), center, 3, yaw, 1, b->host.n_envs, rows, cols, dist_x, dist_y, out, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_heightmap_strided(GqBatch* b, const double* center, int center_stride, const float* yaw, int yaw_stride, int rows, int cols, float dist_x,
                         float dist_y, float* out, void* hip_stream) {
  if (!b || !center || !yaw || !out || rows <= 0 || cols <= 0 || center_stride < 0 || yaw_stride < 0) { SET_ERR("gq_heightmap_strided: bad argument"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  gq_launch_heightmap(b->model->dev.get(), center, center_stride, yaw, yaw_stride, b->host.n_envs, rows, cols, dist_x, dist_y, out, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_jac(GqBatch* b, const double* qpos, int body, const double* point, float* jacp, float* jacr, void* hip_stream) {
  if (!b || !qpos || !point || (!jacp && !jacr)) { SET_ERR("gq_jac: null argument"); return GQ_EINVAL; }
  if (body < 1 || body > GQ_NB) { SET_ERR("gq_jac: body id %d out of range (1 = base .. %d)", body, GQ_NB); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  gq_launch_jac(b->model->dev.get(), qpos, body, point, jacp, jacr, b->host.n_envs, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_ray(GqBatch* b, const double* origin, const float* dir, int n_rays, float* dist, int32_t* geom, void* hip_stream) {
  if (!b || !origin || !dir || !dist || n_rays <= 0) { SET_ERR("gq_ray: bad argument"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  gq_launch_ray(b->model->dev.get(), origin, dir, b->host.n_envs * n_rays, dist, geom, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

/* GqCamShade -> the kernel's CamShade: every field checked (include/gq.h gq_camera_shaded), directions normalised, cutoffs as cosines */
static bool cam_finite(const float* v, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}
static bool cam_unit_range(const float* v, int n) {
  for (int k = 0; k < n; k++)
    if (!(v[k] >= 0.0f && v[k] <= 1.0f)) return false;
  return true;
}
static int camera_shade(const GqCamShade* in, gq::CamShade& s) {
  const char* fn = "gq_camera_shaded";
  if (!in) { SET_ERR("%s: null shade", fn); return GQ_EINVAL; }
  if (!fresh(in, "GqCamShade", fn)) return GQ_EINVAL;
  if (!in->geom_mat) { SET_ERR("%s: null geom_mat", fn); return GQ_EINVAL; }
  if (in->nlight < 0 || in->nlight > GQ_CAM_MAXLIGHT) { SET_ERR("%s: nlight %d is not in [0, %d]", fn, in->nlight, GQ_CAM_MAXLIGHT); return GQ_EINVAL; }
  if (in->head_active != 0 && in->head_active != 1) { SET_ERR("%s: head_active %d is not 0 / 1", fn, in->head_active); return GQ_EINVAL; }
  struct { const char* name; const float* v; int n; } unit[] = {
      {"box_mat", in->box_mat, 7}, {"floor_rgb1", in->floor_rgb1, 3}, {"floor_rgb2", in->floor_rgb2, 3}, {"floor_mark_rgb", in->floor_mark_rgb, 3},
      {"floor_specular", &in->floor_specular, 1}, {"floor_shininess", &in->floor_shininess, 1}, {"floor_emission", &in->floor_emission, 1},
      {"bg_top", in->bg_top, 3}, {"bg_bottom", in->bg_bottom, 3}, {"head_ambient", in->head_ambient, 3}, {"head_diffuse", in->head_diffuse, 3},
      {"head_specular", in->head_specular, 3}};
  for (const auto& u : unit)
    if (!cam_unit_range(u.v, u.n)) { SET_ERR("%s: %s has a value outside [0, 1] (or not finite)", fn, u.name); return GQ_EINVAL; }
  if (!(std::isfinite(in->floor_square) && in->floor_square > 0.0f)) { SET_ERR("%s: floor_square %g is not > 0", fn, (double)in->floor_square); return GQ_EINVAL; }
  if (!(std::isfinite(in->floor_mark_w) && in->floor_mark_w >= 0.0f)) { SET_ERR("%s: floor_mark_w %g is not >= 0", fn, (double)in->floor_mark_w); return GQ_EINVAL; }
  s = gq::CamShade{};
  s.geom_mat = in->geom_mat;
  for (int k = 0; k < 7; k++) s.box_mat[k] = in->box_mat[k];
  for (int k = 0; k < 3; k++) {
    s.rgb1[k] = in->floor_rgb1[k]; s.rgb2[k] = in->floor_rgb2[k]; s.mark_rgb[k] = in->floor_mark_rgb[k];
    s.top[k] = in->bg_top[k]; s.bottom[k] = in->bg_bottom[k];
  }
  s.square = in->floor_square; s.mark_w = in->floor_mark_w;
  s.floor_mat[0] = in->floor_specular; s.floor_mat[1] = in->floor_shininess; s.floor_mat[2] = in->floor_emission;
  if (in->head_active) {
    gq::CamLight& h = s.light[s.nlight++];
    for (int k = 0; k < 3; k++) { h.amb[k] = in->head_ambient[k]; h.dif[k] = in->head_diffuse[k]; h.spe[k] = in->head_specular[k]; }
    h.kind = 0;
  }
  for (int l = 0; l < in->nlight; l++) {
    const GqCamLight& L = in->light[l];
    if (!cam_finite(L.pos, 3) || !cam_finite(L.dir, 3) || !cam_finite(L.attenuation, 3) || !std::isfinite(L.cutoff) || !std::isfinite(L.exponent)) {
      SET_ERR("%s: light %d has a value that is not finite", fn, l); return GQ_EINVAL;
    }
    if (!cam_unit_range(L.ambient, 3) || !cam_unit_range(L.diffuse, 3) || !cam_unit_range(L.specular, 3)) { SET_ERR("%s: light %d has a colour outside [0, 1]", fn, l); return GQ_EINVAL; }
    if (L.directional != 0 && L.directional != 1) { SET_ERR("%s: light %d directional %d is not 0 / 1", fn, l, L.directional); return GQ_EINVAL; }
    if (!(L.cutoff > 0.0f && L.cutoff <= 90.0f)) { SET_ERR("%s: light %d cutoff %g is not in (0, 90] degrees", fn, l, (double)L.cutoff); return GQ_EINVAL; }
    if (!(L.exponent >= 0.0f)) { SET_ERR("%s: light %d exponent %g < 0", fn, l, (double)L.exponent); return GQ_EINVAL; }
    if (L.attenuation[0] < 0.0f || L.attenuation[1] < 0.0f || L.attenuation[2] < 0.0f || L.attenuation[0] + L.attenuation[1] + L.attenuation[2] <= 0.0f) {
      SET_ERR("%s: light %d attenuation must be >= 0 and not all zero", fn, l); return GQ_EINVAL;
    }
    const double dn = std::sqrt((double)L.dir[0] * L.dir[0] + (double)L.dir[1] * L.dir[1] + (double)L.dir[2] * L.dir[2]);
    if (!(dn > 0.0)) { SET_ERR("%s: light %d has a zero direction", fn, l); return GQ_EINVAL; }
    gq::CamLight& o = s.light[s.nlight++];
    for (int k = 0; k < 3; k++) {
      o.pos[k] = L.pos[k]; o.dir[k] = (float)(L.dir[k] / dn); o.att[k] = L.attenuation[k];
      o.amb[k] = L.ambient[k]; o.dif[k] = L.diffuse[k]; o.spe[k] = L.specular[k];
    }
    o.cos_cut = (float)std::cos((double)L.cutoff * 3.14159265358979323846 / 180.0); o.expo = L.exponent;
    o.kind = L.directional ? 1 : 2;
  }
  return GQ_OK;
}

/* gq_camera (mode 0), gq_camera_shaded (1), gq_camera_layered (2): the checks in the order layers, shade, rgba, camera (fn: the entry
 * point's name for the error text), the call record (gq_camera_call.h, shared with the tests' host emulator), the batch's scratch blocks on first
 * use, the launch */
static int camera_run(const char* fn, const int mode, GqBatch* b, const double* qpos, int qpos_stride, int body, const double pos[3], const double quat[4],
                      float fovy_deg, int width, int height, float znear, float zfar, int flags, const float* hull_planes, const int32_t* hull_plane_adr,
                      float* depth, int32_t* seg, double* cam_xpos, float* cam_xmat, const GqCamShade* shade, uint8_t* rgba, const GqCamLayers* layers,
                      void* hip_stream) {
  if (mode >= 2) {
    if (!layers) { SET_ERR("%s: null layers", fn); return GQ_EINVAL; }
    if (!fresh(layers, "GqCamLayers", fn)) return GQ_EINVAL;
    if (layers->n_ghost < 0 || layers->n_ghost > GQ_CAM_MAXGHOST) { SET_ERR("%s: n_ghost %d is not in [0, %d]", fn, layers->n_ghost, GQ_CAM_MAXGHOST); return GQ_EINVAL; }
    if (layers->n_marker < 0 || layers->n_marker > GQ_CAM_MAXMARKER) { SET_ERR("%s: n_marker %d is not in [0, %d]", fn, layers->n_marker, GQ_CAM_MAXMARKER); return GQ_EINVAL; }
    if (layers->n_ghost > 0 && (!layers->ghost_qpos || !layers->ghost_alpha)) { SET_ERR("%s: n_ghost > 0 with a null ghost_qpos or ghost_alpha", fn); return GQ_EINVAL; }
    if (layers->n_ghost > 0 && layers->ghost_stride < 19) { SET_ERR("%s: ghost_stride %d < 19", fn, layers->ghost_stride); return GQ_EINVAL; }
    if (layers->n_marker > 0 && !layers->markers) { SET_ERR("%s: n_marker > 0 with a null markers", fn); return GQ_EINVAL; }
  }
  gq::CamShade s;
  if (mode >= 1) {
    const int rc = camera_shade(shade, s);
    if (rc != GQ_OK) return rc;
    if (!rgba) { SET_ERR("%s: null rgba", fn); return GQ_EINVAL; }
    s.rgba = reinterpret_cast<uint32_t*>(rgba);
  }
  if (!b || !qpos || !pos || !quat || !depth) { SET_ERR("%s: null argument", fn); return GQ_EINVAL; }
  if (qpos_stride < 19) { SET_ERR("%s: qpos_stride %d < 19", fn, qpos_stride); return GQ_EINVAL; }
  if (body < 0 || body > GQ_NB) { SET_ERR("%s: body id %d out of range (0 = world .. %d)", fn, body, GQ_NB); return GQ_EINVAL; }
  if (width <= 0 || height <= 0 || (size_t)width * height > (1u << 24)) { SET_ERR("%s: bad image size %d x %d", fn, width, height); return GQ_EINVAL; }
  if (!(fovy_deg > 0.0f && fovy_deg < 180.0f)) { SET_ERR("%s: fovy %g is not in (0, 180) degrees", fn, (double)fovy_deg); return GQ_EINVAL; }
  if (!(znear > 0.0f && zfar > znear)) { SET_ERR("%s: need 0 < znear < zfar (got %g, %g)", fn, (double)znear, (double)zfar); return GQ_EINVAL; }
  if (flags & ~(GQ_CAM_ROBOT | GQ_CAM_SCENE | GQ_CAM_TRACK)) { SET_ERR("%s: unknown flags 0x%x", fn, flags); return GQ_EINVAL; }
  if ((flags & GQ_CAM_TRACK) && body == 0) { SET_ERR("%s: GQ_CAM_TRACK needs a body camera (body > 0)", fn); return GQ_EINVAL; }
  GqModel* m = b->model;
  gq::CamCall c{};
  if (gq::cam_fill_call(c, fn, m->host, m->lg_cloud, m->ncloud, m->ngeom, qpos, qpos_stride, body, pos, quat, fovy_deg, width, height, znear, zfar, flags,
                        hull_planes, hull_plane_adr, depth, seg, cam_xpos, cam_xmat, g_err, sizeof g_err)) return GQ_EINVAL;
  DeviceGuard guard(m->device);
  const int n = b->host.n_envs;
  HIP_TRY(gq::ensure_both(b->cam_rec, (size_t)GQ_CAM_REC * n, b->cam_pos, (size_t)3 * n, false));
  c.rec = b->cam_rec.get(); c.cpos = b->cam_pos.get();
  gq::CamLayers l{};
  if (mode >= 2) {
    HIP_TRY(b->cam_grec.ensure((size_t)GQ_CAM_GREC * layers->n_ghost * n, false));
    l.ghost_qpos = layers->ghost_qpos; l.ghost_stride = layers->ghost_stride; l.n_ghost = layers->n_ghost;
    l.ghost_alpha = layers->ghost_alpha; l.ghost_rgb = layers->ghost_rgb;
    l.n_marker = layers->n_marker; l.markers = layers->markers; l.grec = b->cam_grec.get();
  }
  gq_launch_camera(m->dev.get(), &c, mode >= 1 ? &s : nullptr, mode >= 2 ? &l : nullptr, n, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return GQ_OK;
}

int gq_camera(GqBatch* b, const double* qpos, int qpos_stride, int body, const double pos[3], const double quat[4], float fovy_deg, int width, int height,
              float znear, float zfar, int flags, const float* hull_planes, const int32_t* hull_plane_adr,
              float* depth, int32_t* seg, double* cam_xpos, float* cam_xmat, void* hip_stream) {
  return camera_run("gq_camera", 0, b, qpos, qpos_stride, body, pos, quat, fovy_deg, width, height, znear, zfar, flags, hull_planes, hull_plane_adr,
                    depth, seg, cam_xpos, cam_xmat, nullptr, nullptr, nullptr, hip_stream);
}
int gq_camera_shaded(GqBatch* b, const double* qpos, int qpos_stride, int body, const double pos[3], const double quat[4], float fovy_deg, int width,
                     int height, float znear, float zfar, int flags, const float* hull_planes, const int32_t* hull_plane_adr,
                     float* depth, int32_t* seg, double* cam_xpos, float* cam_xmat, const GqCamShade* shade, uint8_t* rgba, void* hip_stream) {
  return camera_run("gq_camera_shaded", 1, b, qpos, qpos_stride, body, pos, quat, fovy_deg, width, height, znear, zfar, flags, hull_planes, hull_plane_adr,
                    depth, seg, cam_xpos, cam_xmat, shade, rgba, nullptr, hip_stream);
}
int gq_camera_layered(GqBatch* b, const double* qpos, int qpos_stride, int body, const double pos[3], const double quat[4], float fovy_deg, int width,
                      int height, float znear, float zfar, int flags, const float* hull_planes, const int32_t* hull_plane_adr,
                      float* depth, int32_t* seg, double* cam_xpos, float* cam_xmat, const GqCamShade* shade, uint8_t* rgba,
                      const GqCamLayers* layers, void* hip_stream) {
  return camera_run("gq_camera_layered", 2, b, qpos, qpos_stride, body, pos, quat, fovy_deg, width, height, znear, zfar, flags, hull_planes, hull_plane_adr,
                    depth, seg, cam_xpos, cam_xmat, shade, rgba, layers, hip_stream);
}

int gq_forward(GqBatch* b, int stage, const float* ctrl, GqState st, GqObsOut out, void* hip_stream) {
  if (!b || !have_tensors(st, out)) { SET_ERR("gq_forward: null tensor"); return GQ_EINVAL; }
  if (stage != 0 && stage != 1) { SET_ERR("gq_forward: stage must be 0 (mj_forward) or 1 (mj_step1)"); return GQ_EINVAL; }
  if (b->host.debug_envs <= 0 || !b->debug.get()) { SET_ERR("gq_forward: no inspection record to write to (call gq_debug_enable first)"); return GQ_EINVAL; }
  if (b->model->host.solver != 1) { SET_ERR("gq_forward needs the Newton solver (solver = 1)"); return GQ_EINVAL; }
  DeviceGuard guard(b->model->device);
  if (const int rc = ensure_args(b, st, out, nullptr, nullptr, nullptr, (hipStream_t)hip_stream); rc != GQ_OK) return rc;
  gq::StepCall c{};
  c.ctrl = ctrl; c.debug = b->debug.get(); c.forward = stage == 1 ? 1 : 2;
  HIP_TRY(launch_step_kernel(b, &c, b->host.n_envs, (hipStream_t)hip_stream));
  return GQ_OK;
}

static const struct { const char* name; int off, n; } kDbg[] = {
    {"M", GQ_DBG_M, 324}, {"qfrc_bias", GQ_DBG_BIAS, 18}, {"qfrc_smooth", GQ_DBG_SMOOTH, 18},
    {"qacc_smooth", GQ_DBG_QACC_SMOOTH, 18}, {"qfrc_constraint", GQ_DBG_QFRC_C, 18}, {"xpos", GQ_DBG_XPOS, 39},
    {"xmat", GQ_DBG_XMAT, 117}, {"nefc", GQ_DBG_NEFC, 1}, {"ncon", GQ_DBG_NCON, 1}, {"niter", GQ_DBG_NITER, 1},
    {"efc_J", GQ_DBG_EFC_J, 64 * 18}, {"efc_aref", GQ_DBG_EFC_AREF, 64}, {"efc_R", GQ_DBG_EFC_R, 64},
    {"efc_b", GQ_DBG_EFC_B, 64}, {"efc_force", GQ_DBG_EFC_FORCE, 64}, {"efc_type", GQ_DBG_EFC_TYPE, 64},
    {"contact_dist", GQ_DBG_CON_DIST, GQ_MAXCON}, {"contact_geom", GQ_DBG_CON_GEOM, GQ_MAXCON},
    {"foot_pos", GQ_DBG_FOOT_POS, 12}, {"qacc", GQ_DBG_QACC, 18}, {"timer", GQ_DBG_TIMER, 32}, {"xq", GQ_DBG_XQ, 16}, {"record", 0, GQ_DBG_SIZE}};

int gq_debug_stop_stage(GqBatch* b, int stage) {
  if (!b) { SET_ERR("gq_debug_stop_stage: null batch"); return GQ_EINVAL; }
  b->stop_stage = stage;
  return GQ_OK;
}

int gq_debug_field(const char* name, int32_t* offset, int32_t* count) {
  if (!name || !offset || !count) { SET_ERR("gq_debug_field: null argument"); return GQ_EINVAL; }
  for (const auto& f : kDbg)
    if (!std::strcmp(f.name, name)) { *offset = f.off; *count = f.n; return GQ_OK; }
  SET_ERR("gq_debug_field: unknown field %s", name);
  return GQ_EINVAL;
}

int gq_debug_device_buffer(GqBatch* b, float** dev, int32_t* n_envs, int32_t* stride) {
  if (!b || !dev || !n_envs || !stride) { SET_ERR("gq_debug_device_buffer: null argument"); return GQ_EINVAL; }
  *dev = b->host.debug_envs > 0 ? b->debug.get() : nullptr; *n_envs = b->host.debug_envs; *stride = GQ_DBG_SIZE;
  return GQ_OK;
}

int gq_full_mass(GqBatch* b, int n_envs, float* M, void* hip_stream) {
  if (!b || !M || n_envs <= 0) { SET_ERR("gq_full_mass: null / empty argument"); return GQ_EINVAL; }
  if (!b->debug.get() || n_envs > b->host.debug_envs) {
    SET_ERR("gq_full_mass: the inspection record covers %d envs, %d requested (gq_debug_enable first, then gq_step / gq_forward)", b->host.debug_envs, n_envs);
    return GQ_EINVAL;
  }
  DeviceGuard guard(b->model->device);
  HIP_TRY(hipMemcpy2DAsync(M, 324 * sizeof(float), b->debug.get() + GQ_DBG_M, GQ_DBG_SIZE * sizeof(float), 324 * sizeof(float), (size_t)n_envs,
                           hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return GQ_OK;
}

int gq_debug_get(GqBatch* b, int env, const char* name, double* out, int max_n) {
  if (!b || !name || !out || env < 0 || env >= b->host.debug_envs || !b->debug.get()) { SET_ERR("gq_debug_get: bad argument / debug not enabled"); return GQ_EINVAL; }
  for (const auto& f : kDbg)
    if (!std::strcmp(f.name, name)) {
      int n = f.n < max_n ? f.n : max_n;
      std::vector<float> tmp((size_t)n);
      DeviceGuard guard(b->model->device);
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemcpy(tmp.data(), b->debug.get() + (size_t)env * GQ_DBG_SIZE + f.off, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; i++) out[i] = tmp[(size_t)i];
      return n;
    }
  SET_ERR("gq_debug_get: unknown field %s", name);
  return GQ_EINVAL;
}

}  // extern "C"
