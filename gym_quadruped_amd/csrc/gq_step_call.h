/*
 * gq_step_call.h - the host side of a step / reset call: which kernel variants a model runs, and the caller's tensors plus the batch's own
 * pointers into the argument blocks the kernels read (StepArgs: gq_step_kernel.h, ResetArgs: gq_step_body.h).  gq_api.hip fills its
 * launches with this; so does the host emulator of the tests (tests/simt_emu), over host memory.  Host code only.
 */
#pragma once
#include "gq.h"
#include "gq_step_body.h"

namespace gq {
/* world boxes / height field: the world scenes, split by whether the robot has sphere / capsule / box link geoms (exact pair routines
 * compiled in; gq_step_body.h PRIM); flat: the self-collision stage runs for a model with self-collision pairs, built with the pair
 * routines its pair table names and no others (gq_step_kernel.h Scene).  The table read here, sp[0 .. nsp), is the one pass B of
 * append_self_contacts walks (gq_boxes.h): a kind it holds always has its routine in the kernel.  -DGQ_SCENE_SPLIT_OFF (host code only,
 * for tests and A/B builds): every flat self-collision model runs the kernel with all the routines. */
inline Scene model_scene(const GqDevModel& h) {
  if (h.nbox > 0 || h.hf_nrow > 0) {
    /* lg[] is indexed by link geom (item[] is in contact order: feet and link geoms interleaved by geom id) */
    for (int g = 0; g < h.nlg; g++) { const int t = h.lg[g].ptype; if (t == 2 || t == 3 || t == 6) return SCENE_WORLD_PRIM; }
    return SCENE_WORLD_HULL;
  }
  if (h.nsp <= 0) return SCENE_FLAT;
#ifdef GQ_SCENE_SPLIT_OFF
  return SCENE_FLAT_SELF;
#else
  bool box = false, cvx = h.ncvx_self > 0;
  for (int p = 0; p < h.nsp; p++) {
    const int k = h.sp[p].kind;
    if (k >= 1 && k <= 3) box = true;
    else if (k != 0) cvx = true; /* kind 4 (counted by ncvx_self) - and anything this function does not know gets the full kernel */
  }
  return box && cvx ? SCENE_FLAT_SELF : cvx ? SCENE_FLAT_SELF_HULL : SCENE_FLAT_SELF_PRIM;
#endif
}
/* StepCall::auto_reset of a launch that is given this auto-reset configuration (NULL: none) */
inline int auto_reset_mode(const GqResetCfg* cfg) { return cfg ? (cfg->autoreset_next_step ? 2 : 1) : 0; }
inline void fill_reset_cfg(ResetCfgDev* d, const GqResetCfg* cfg) {
  d->seed_lo = (uint32_t)(cfg->seed & 0xffffffffu); d->seed_hi = (uint32_t)(cfg->seed >> 32);
  d->random = cfg->random; d->q_pos_amp = cfg->q_pos_amp; d->q_vel_amp = cfg->q_vel_amp;
  d->roll_sweep = cfg->roll_sweep; d->pitch_sweep = cfg->pitch_sweep; d->hip_height = cfg->hip_height;
  for (int k = 0; k < 2; k++) { d->lin_vel_range[k] = cfg->lin_vel_range[k]; d->ang_vel_range[k] = cfg->ang_vel_range[k]; d->friction_range[k] = cfg->friction_range[k]; }
  d->cmd_forward = cfg->cmd_forward; d->cmd_random = cfg->cmd_random; d->cmd_rotate = cfg->cmd_rotate; d->cmd_human = cfg->cmd_human;
  d->env_id_offset = cfg->env_id_offset;
}

/* the pointers a batch owns or has been given, in the memory the kernels read (NULL: the batch does not have it) */
struct BatchPtrs {
  GqDevModel* model; GqDevBatch* batch;   /* the model and batch blocks */
  float *vx, *vy, *vz;                    /* cloud vertices SoA */
  float* friction_next;   /* [N]: friction drawn by reset, committed after the reset step */
  uint8_t* pending;       /* [N]: next-step auto-reset flags */
  uint8_t* lift_pending;  /* [N]: reset kernel -> the reset's own step: lift loop still due */
  uint8_t* load_hint;     /* [N]: per-env solver load of the previous step (scheduling hint of the step kernel) */
  float* imu_bias; float* heightmap;  /* caller-owned [N][6] (gq_batch_set_imu), [N][rows * cols][3] (gq_batch_set_heightmap) */
  int32_t* h9; float* ext_dist;       /* caller-owned [N][6] resampling counters and wrench (gq_batch_set_resampling) */
  float* dyn; float* contacts;        /* caller-owned rows (gq_batch_set_outputs) */
};
/* hm: the host copy of p.model */
inline void fill_step_args(StepArgs* a, const BatchPtrs& p, const GqDevModel& hm, int n_envs, const GqState& st, const GqObsOut& out, const int32_t* episode, uint8_t* lift_failed) {
  a->model = p.model; a->batch = p.batch; a->vx = p.vx; a->vy = p.vy; a->vz = p.vz;
  a->qpos = st.qpos; a->qvel = st.qvel; a->qacc = st.qacc; a->warm = st.qacc_warmstart;
  a->applied = st.qfrc_applied; a->time = st.time; a->friction = st.friction; a->cmd = st.cmd;
  a->friction_next = p.friction_next; a->pending = p.pending; a->load_hint = p.load_hint; a->imu_bias = p.imu_bias; a->heightmap = p.heightmap;
  a->h9 = p.h9; a->ext_dist = p.ext_dist; a->dyn = p.dyn; a->contacts = p.contacts;
  a->lift_failed = lift_failed; a->lift_pending = p.lift_pending; a->episode_ro = episode;
  a->obs = out.obs; a->reward = out.reward; a->terminated = out.terminated; a->truncated = out.truncated;
  a->invalid_contact = out.invalid_contact; a->step_num = out.step_num; a->step_prev = out.step_num_prev;
  a->contacts_dropped = out.contacts_dropped; a->n_envs = n_envs;
  a->timestep = hm.timestep; a->nlg = hm.nlg; a->nfl = hm.nfl; a->pad_ = 0;
}
/* The block of a fused auto-reset.  An explicit reset (gq_reset) then adds what only it has: mask, qpos_new / qvel_new, the flags to clear and
 * the lift_pending scratch (inside a fused auto-reset the wave hands that flag to its own step).  cmd_reset: GqDevBatch::rs_cmd_reset.
 * A caller without a friction tensor has nothing to commit a draw to: none is made. */
inline void fill_reset_args(ResetArgs* a, const BatchPtrs& p, int cmd_reset, const GqResetCfg* cfg, const GqState& st, const GqObsOut& out, int32_t* episode, uint8_t* lift_failed) {
  a->model = p.model; a->vx = p.vx; a->vy = p.vy; a->vz = p.vz; a->mask = nullptr; a->qpos_new = nullptr; a->qvel_new = nullptr;
  a->qpos = st.qpos; a->qvel = st.qvel; a->qacc = st.qacc; a->warm = st.qacc_warmstart; a->applied = st.qfrc_applied;
  a->time = st.time; a->cmd = st.cmd; a->friction_next = st.friction ? p.friction_next : nullptr;
  a->step_num = out.step_num; a->episode = episode; a->lift_failed = lift_failed;
  a->h9 = p.h9; a->lift_pending = nullptr;
  fill_reset_cfg(&a->cfg, cfg);
  a->cfg.cmd_reset = cmd_reset;
}
}  // namespace gq
