/*
 * gq_kernels.hip - gfx950 kernels of libgq: one environment per 64-lane wavefront, one wavefront per workgroup
 * (grid = n_envs).  With 4096 envs and <= 128 VGPRs / <= 10 KB LDS per wave the whole batch is resident at once
 * (4 waves per SIMD, 16 per CU); workgroup b lands on XCD b % 8, so consecutive envs spread over all eight L2s and
 * every XCD keeps its own copy of the read-only model block.
 * This file holds the __global__ kernels, the mailbox side of the closed-loop rollout, the policy kernels and the dispatch; the step
 * kernels' driver is gq_step_driver.h, the step itself gq_step_body.h.
 */
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <gq_device.h>
#include "gq_step_body.h"
#include "gq_foot_cmd.h"
#include "gq_learn.h"
#include "gq_policy_dev.h"
#include "gq_camera.h"

/* Parallel build (csrc/Makefile): this file is compiled once per part (-DGQ_PART=k; the variants are 60 large, fully inlined kernels - one
 * unit took 7.5 minutes, the parts build side by side in about one).  part_of() at the end of the file assigns every kernel variant to its
 * part; part 0 holds the non-template kernels, the launch entry points and the dispatch over the parts.  GQ_PART undefined: everything in
 * one unit (make dev, tools/kernel_resources.py, isa_report.py). */
#ifndef GQ_PART
#define GQ_PART (-1)
#endif
#define GQ_IN_MISC (GQ_PART <= 0)

/* the driver every step kernel below calls: step_kernel_body - the persistent step loop, the re-spawn loop around reset_wave / step_wave -
 * and the inline policies (pd_action also serves policy_pd_kernel); a header, because the tests' host emulator runs it too */
#include "gq_step_driver.h"

namespace gq {

template <int SOLVER, int MODE, bool CONE, bool BOXES, bool SELF, bool PRIM, bool PERSIST = false>
__global__ void __launch_bounds__(GQ_WAVE, 4) step_kernel(const FusedArgs* __restrict__ A, const StepCall c) {
  step_kernel_body<SOLVER, MODE, CONE, BOXES, SELF, PRIM, PERSIST, true>(A, c);
}
/* gq_step_foot_cmd: the Newton production persistent variants with the foot-space law (gq_foot_cmd.h) as their inline policy.  Kernels of
 * their own, as PERSIST itself is: one more policy arm in the kernels step_pd and the rollouts run cost those 0.6 - 1 % on some robots
 * (profiles/foot_cmd_kernel_resources.md), so those kernels stay as they were, byte for byte. */
template <bool CONE, bool BOXES, bool SELF, bool PRIM>
__global__ void __launch_bounds__(GQ_WAVE, 4) step_kernel_foot(const FusedArgs* __restrict__ A, const StepCall c) {
  step_kernel_body<1, 0, CONE, BOXES, SELF, PRIM, true, true, true>(A, c);
}
template <bool CONE>
__global__ void __launch_bounds__(GQ_WAVE, 4) step_kernel_prim_foot(const FusedArgs* __restrict__ A, const StepCall c) {
  step_kernel_body<1, 0, CONE, false, true, true, true, false, true>(A, c);
}
/* SCENE_FLAT_SELF_PRIM: the self-collision stage without the convex block and the pair exchange */
template <int SOLVER, int MODE, bool CONE, bool PERSIST = false>
__global__ void __launch_bounds__(GQ_WAVE, 4) step_kernel_prim(const FusedArgs* __restrict__ A, const StepCall c) {
  step_kernel_body<SOLVER, MODE, CONE, false, true, true, PERSIST, false>(A, c);
}

/* Closed-loop persistent rollout, the stepping side (protocol: gq_mailbox.h).  grid = any number of one-wave workgroups:
 * each pops tickets of ITS XCD's ready queue until every env-step of the rollout has been claimed.  Production Newton variants only. */
template <int SOLVER, bool CONE, bool BOXES, bool SELF, bool PRIM, bool CVX>
__device__ __forceinline__ void mailbox_step_body(const FusedArgs* __restrict__ A, const StepCall c0, const MailboxDev* __restrict__ MBp) {
  __shared__ WaveMem W;
#if GQ_TICKSET
  if (lane_id() == 0) W.tk_T = nullptr;
#endif
  const GQ_MODEL MailboxDev& MB = *mptr(MBp);
  const int q = MB.xcc_queue[xcc_id()];
  const int N = MB.n_envs, nq = MB.nq, qmask = MB.qcap - 1, qshift = __builtin_ctz(MB.qcap);
  const int total = mb_queue_envs(N, q, nq) * MB.n_steps; /* mb_queue_tickets of this queue: it fits 32 bits (mb_rollout_fits, checked by the host) */
  int32_t* const head = mb_ctr(MB.q_ctr, q, MB_CTR_POP);
  int32_t* const items = MB.q_items + (size_t)q * MB.qcap;
  int played = 0;
  for (;;) {
    int ticket = 0;
    if (lane_id() == 0) ticket = add_pub(head, 1);
    ticket = uniform(ticket);
    if (ticket >= total) break;
    /* the item of the ticket's own lap; an aborted rollout is left here, with what this wavefront has played */
    GQ_MB_WAIT_ITEM(env, { if (lane_id() == 0 && played) mb_add_played(MB.status, played); return; })
    adopt_fence();
    /* the env's step index is only needed to place the row in obs_seq: otherwise that round trip is not taken */
    const int k = MB.obs_seq ? __builtin_amdgcn_readfirstlane(ld_pub(MB.steps_done + env)) : 0;
    StepCall ck = c0;
    ck.env0 = env - (int)blockIdx.x; /* step_wave / reset_wave address env0 + wave index */
    ck.ctrl = MB.act;
    ck.obs_seq = MB.obs_seq ? MB.obs_seq + (size_t)k * N * mptr(A->s.batch)->obs_dim : nullptr;
    const StepCall& c = ck;
    int pass = 0;
    WaveCtx C;
    int hint = load_rows<SOLVER, true>(A->s, c, W, env, true, C);
    bool respawn = c.auto_reset == 2 && C.pend; /* wave-uniform */
    if (respawn) {
      wave_priority(3);
      wave_barrier();
      reset_wave<BOXES, PRIM, true>(A->r, W, c.env0);
      pass = c.auto_reset;
      hint = load_rows<SOLVER, true>(A->s, c, W, env, false, C, true);
    }
    step_wave<SOLVER, 0, CONE, BOXES, SELF, PRIM, true, CVX>(A->s, c, W, pass, hint, C);
    publish_fence(); /* state rows are in this XCD's L2, the observation row has been written through */
    if (lane_id() == 0) add_pub(MB.steps_done + env, 1);
    wave_barrier();
    played++;
  }
  if (lane_id() == 0 && played) mb_add_played(MB.status, played);
}
template <int SOLVER, bool CONE, bool BOXES, bool SELF, bool PRIM>
__global__ void __launch_bounds__(GQ_WAVE, 4) mailbox_step_kernel(const FusedArgs* __restrict__ A, const StepCall c0, const MailboxDev* __restrict__ MBp) {
  mailbox_step_body<SOLVER, CONE, BOXES, SELF, PRIM, true>(A, c0, MBp);
}
template <int SOLVER, bool CONE> /* SCENE_FLAT_SELF_PRIM, as step_kernel_prim */
__global__ void __launch_bounds__(GQ_WAVE, 4) mailbox_step_kernel_prim(const FusedArgs* __restrict__ A, const StepCall c0, const MailboxDev* __restrict__ MBp) {
  mailbox_step_body<SOLVER, CONE, false, true, true, false>(A, c0, MBp);
}

#if GQ_IN_MISC
/* the built-in policy of the closed-loop rollout.  A policy wavefront serves envs of ITS XCD's queue only (lane = env, strided over the
 * policy wavefronts that landed on the XCD): observation row, action row, count and queue slot of an env are written and read
 * through one L2, like the env's state rows - no hand-off of the rollout depends on coherence between two XCDs' L2s, and none
 * needs a device-scope fence (a device-scope acquire on the stepping side costs 14 % of the throughput: it empties the XCD's L2). */
__global__ void __launch_bounds__(GQ_WAVE) policy_pd_kernel(const MailboxDev* __restrict__ MBp, const PolicyPdDev* __restrict__ Pp, const float* __restrict__ obs, const int od) {
  const GQ_MODEL MailboxDev& MB = *mptr(MBp);
  const GQ_MODEL PolicyPdDev& P = *mptr(Pp);
  const int lane = (int)threadIdx.x, nq = MB.nq, q = MB.xcc_queue[xcc_id()], qmask = MB.qcap - 1, qshift = __builtin_ctz(MB.qcap);
  const int N = MB.n_envs, K = MB.n_steps;
  GQ_MB_POLICY_REGISTER() /* rank, mine, t_last (gq_mailbox.h) */
  const int nmine = mb_queue_envs(N, q, nq);         /* envs of this queue: e = q + nq * i */
  const int g = rank * GQ_WAVE + lane, G = mine * GQ_WAVE;
  int32_t* const tail = mb_ctr(MB.q_ctr, q, MB_CTR_PUSH);
  int32_t* const items = MB.q_items + (size_t)q * MB.qcap;
  t_last = wall_clock64();
  for (;;) {
    bool all_done = true, progress = false;
    for (int i = g; i < nmine; i += G) {
      const int e = q + nq * i;
      const int k = MB.issued[e];
      if (k >= K) continue;
      all_done = false;
      if (ld_pub(MB.steps_done + e) < k) continue; /* the observation after step k - 1 is not out yet */
      /* (the observation words are read AFTER the count has been seen: loads of one batch may be served in any order) */
      const float* row = obs + (size_t)e * od;
      float qj[12], qd[12];
#pragma unroll
      for (int j = 0; j < 12; j++) { qj[j] = ld_pub(row + P.col_q[j]); qd[j] = ld_pub(row + P.col_qd[j]); }
      /* the action row and the push ticket travel together */
      const int s = mb_push_ticket(tail);
#pragma unroll
      for (int j = 0; j < 12; j++) {
        const float a = pd_action(P, j, qj[j], qd[j], k, (uint32_t)(e + P.env_id_offset));
        st_pub(MB.act + (size_t)e * 12 + j, a);
        if (MB.act_seq) MB.act_seq[((size_t)k * N + e) * 12 + j] = a;
      }
      mb_push_item(items, qmask, qshift, s, e); /* after the action is in place */
      MB.issued[e] = k + 1;
      progress = true;
    }
    if (all_done) break;
    if (progress) { t_last = wall_clock64(); continue; }
    GQ_MB_POLICY_IDLE(true, g) /* every lane looks, and speaks, for itself */
  }
}

/* A learned policy in the same seat (gq_rollout_policy): an MLP on the matrix cores (gq_policy_mlp.h) gives the env a joint-target action
 * every `decimation` steps; at EVERY step the env's lane turns the held action into torques with the joint-impedance law and hands them
 * to the step side exactly as policy_pd_kernel does - same registration, same XCD rule, same deadline on every wait.  Lane = env, strided
 * as there; the lanes of a pass whose env is ready AND due for a new action are compacted by ballot into tiles of up to 16 rows, which the
 * whole wavefront stages (device-scope loads: every word of the row is another wavefront's store of this launch) and takes through the
 * layers.  An env that re-spawns ignores the torque of that step (next-step auto-reset); its held and last action are kept.
 * LEARN (MODE != 0, gq_rollout_policy_learn; MODE 0 compiles to the kernel as it was): the same seat also records what a learner needs, where
 * the data passes anyway.  At a fresh policy step the row the network is fed and its output before noise and clip are recorded.  At every
 * visit - the observation after step k - 1 is out, the env waits for this wavefront - learn_visit (gq_learn.h, THE definition of the window
 * law) evaluates the reward of step k - 1 from that row, the torques of step k - 1 (still in the env's mailbox), the held action and the one
 * before it, and the batch's `terminated` byte, every one of them a device-scope load, and carries the window in per-env words that the
 * env's lane alone writes.  Every env gets ONE CLOSING VISIT at k = K, when its last observation is out: it pushes nothing - the step side's
 * ticket count is unchanged, and the wait for that observation is the loop's own wait, with its deadline and the abort word.
 * MODE 1: learn_visit<false>; 2: learn_visit<true>, the foot terms of gq_reward_feet.h and their state, the air times
 * (gq_rollout_policy_learn_feet).  With all foot weights 0 mode 2 computes mode 1's bits, but BOTH instantiations are kept: a learning call
 * without foot terms through mode 2 measured 16.24 - 16.37 M env-steps/s against 16.53 - 16.65 through mode 1 (go2, 4096 envs, K = 96; no
 * overlap in three alternated turns, profiles/learn_window_refactor.md) - the foot law's block and branches stay in the visit's way even when
 * nothing of it is on.  Against the kernels before the fold the visit needs fewer VGPRs in both modes (132 / 160 against 180 / 204); mode 2
 * has 280 SGPR spills (to VGPR lanes, no scratch) against 252: the step's reward now leaves learn_step as a value and is added to acc under
 * a second `if (earns)` in learn_visit, where it was added inside the branch that evaluated it.
 * RECURRENT (MODE & 4, gq_rollout_policy_gru; MODE 0 .. 2 compile to the kernels they were): the network is a GRU cell and a head
 * (gq_policy_gru.h), the block's gru part.  The episode rule runs for every ready lane before the tile loop; the
 * tile stage also loads each row's hidden state (device scope: the row is its env's lane's store of an earlier visit) - a row the rule
 * zeroed in THIS visit is staged as zeros from the lane's own flag, not from memory - and h' is stored by the env's own lane between the
 * cell and the head.  The flags come from the block's episode part: P.learn is not read in mode 4.
 * THE INPUT ROW of every mode is policy_row_value (gq_policy_dev.h, its one definition), called once per staged word with device-scope
 * memory access; the wave-level work around it - which lane's env is which row of the tile, that row's sources - is done here.
 * HEIGHT SCAN (MODE & 8, gq_rollout_policy_scan, with every mode above; MODE 0 .. 6 compile to the kernels they were): the input row has a
 * middle block, the scan law (gq_policy_scan.h) on
 * word 2 of the env's hit points - the batch's base-following HeightMap, whose rays the env's stepping wavefront cast in the step whose
 * observation row is being fed - and the z column of that row.  Both are device-scope loads.  The hit words are plain stores of the stepping
 * wavefront, like the env's state rows: it waits for them (publish_fence, vmcnt(0)) before it raises steps_done, policy and stepping
 * wavefront of an env share one XCD (gq_mailbox.h), so they are in that XCD's L2 when the count is seen and a load that misses the L1 reads
 * them.  The last-action columns follow the scan; scan words are recorded in policy_obs like every other word the network is fed.
 * OBSERVATION HISTORY (MODE & 16, gq_rollout_policy_hist, the MLP's modes with or without the scan; MODE 0 .. 14 compile to the kernels they
 * were): the frames of the env's last L policy steps follow the last action (gq_policy_hist.h: the law, the two-buffer store, the episode
 * rule).  The rule runs for every ready lane before the tile loop and costs one
 * control word; whoever stages a word of the current block also stores it as the newest frame of the env's OTHER buffer, whoever stages a
 * history word moves it one slot on into that buffer - every word has one staging lane, and nobody writes the buffer being read.  History
 * words are stores of another visit of this launch, possibly by another lane of this wavefront: device-scope loads and stores, as for the
 * hidden state (a plain load may hit the line an earlier plain load left in the vector L1).  The control word is the env's own lane's.
 * SENSOR NOISE (MODE & 32, gq_rollout_policy_noise, with every mode above; MODE 0 .. 26 compile to the kernels they were): the observation and
 * scan words the network is fed carry the noise of gq_policy_noise.h, a Philox block per noised word keyed by (column, step0 + k, global env
 * id) under the action noise's seed.  The amplitude table is immutable during the launch: an ordinary load per observation column, nothing
 * of device scope.  Only policy_row_value sees the noise: the torque law below, learn_visit and both episode rules read the true row, so the
 * state after the call is the step loop's with the recorded torques.  The true words go to the block's rec_clean, where one is given. */
template <int MODE>
__global__ void __launch_bounds__(GQ_WAVE) policy_mlp_kernel(const MailboxDev* __restrict__ MBp, const PolicyDev* __restrict__ Pp, const float* __restrict__ obs, const int od) {
  constexpr bool GRU = (MODE & 4) != 0;
  constexpr bool SCAN = (MODE & 8) != 0;
  constexpr bool HIST = (MODE & 16) != 0;
  constexpr bool NOISE = (MODE & 32) != 0;
  static_assert(!(GRU && HIST), "the observation history is the MLP's: a recurrent policy has its hidden state");
  constexpr int LMODE = MODE & 3;
  constexpr bool LEARN = LMODE != 0;
  __shared__ __attribute__((aligned(16))) float xt[GRU ? 3 : 2][GQ_MLP_MAXW * GQ_MLP_ROWS];
  const GQ_MODEL MailboxDev& MB = *mptr(MBp);
  const GQ_MODEL PolicyDev& PD = *mptr(Pp);
  const GQ_MODEL PolicyMlpDev& P = PD.seat;
  const int lane = (int)threadIdx.x, nq = MB.nq, q = MB.xcc_queue[xcc_id()], qmask = MB.qcap - 1, qshift = __builtin_ctz(MB.qcap);
  const int N = MB.n_envs, K = MB.n_steps, D = P.decimation;
  GQ_MB_POLICY_REGISTER() /* rank, mine, t_last (gq_mailbox.h) */
  const MlpNet net = mlp_net_load(P.net);
  [[maybe_unused]] GruNet cell{};
  if constexpr (GRU) cell = gru_net_load(PD.gru.cell);
  const int in_dim = GRU ? cell.in_dim : net.in_dim;
  RowLaw row_law{}; /* the input row (gq_policy_dev.h) */
  row_law.in_obs = P.in_obs; row_law.in_dim = in_dim; row_law.shift = P.shift; row_law.scale = P.scale;
  [[maybe_unused]] int scan_col_z = 0;
  [[maybe_unused]] const float* scan_hits = nullptr;
  if constexpr (SCAN) {
    row_law.scan.offset = PD.scan.law.offset; row_law.scan.clip = PD.scan.law.clip; row_law.scan.scale = PD.scan.law.scale;
    row_law.cells = PD.scan.cells; scan_col_z = PD.scan.col_z; scan_hits = PD.scan.hits;
  }
  const HistLaw& hist = row_law.hist;
  [[maybe_unused]] float* hist_state = nullptr;
  [[maybe_unused]] int32_t* hist_ctl = nullptr;
  if constexpr (HIST) {
    const GQ_MODEL HistLaw& HL = PD.hist.law;
    row_law.hist.frames = HL.frames; row_law.hist.cols = HL.cols; row_law.hist.width = HL.width; row_law.hist.col0 = HL.col0; row_law.hist.inv = HL.inv;
    hist_state = PD.hist.state; hist_ctl = PD.hist.ctl;
  }
  [[maybe_unused]] RowNoise row_noise{}; /* the law's part is the call's, the key each row's */
  [[maybe_unused]] float* noise_clean = nullptr;
  if constexpr (NOISE) {
    const GQ_MODEL NoiseDev& ND = PD.noise;
    row_noise.law.amp = ND.amp; row_noise.law.kind = ND.kind; row_noise.law.scan_amp = ND.scan_amp;
    row_noise.law.seed_lo = P.seed_lo; row_noise.law.seed_hi = P.seed_hi;
    noise_clean = ND.rec_clean;
  }
  const int nmine = mb_queue_envs(N, q, nq);         /* envs of this queue: e = q + nq * i */
  const int G = mine * GQ_WAVE;
  int32_t* const tail = mb_ctr(MB.q_ctr, q, MB_CTR_PUSH);
  int32_t* const items = MB.q_items + (size_t)q * MB.qcap;
  t_last = wall_clock64();
  for (;;) {
    bool all_done = true, progress = false;
    for (int base = rank * GQ_WAVE; base < nmine; base += G) { /* wave-uniform: the tile work below needs every lane */
      const int i = base + lane;
      const int e = i < nmine ? q + nq * i : q;      /* (a lane without env reads env q's words and does nothing) */
      constexpr int KL = LEARN ? 1 : 0;             /* LEARN: the closing visit at k = K */
      const int k = i < nmine ? P.issued[e] : K + KL;
      const bool live = k < K + KL;
      if (live) all_done = false;
      const bool ready = live && ld_pub(MB.steps_done + e) >= k; /* the observation after step k - 1 is out */
      const bool fresh = ready && k % D == 0 && (!LEARN || k < K); /* ... and the env is due for a new action */
      float a[12];
      [[maybe_unused]] bool h_zeroed = false;
      if constexpr (GRU) { /* the episode rule (gq_policy_gru.h), before any cell evaluation of this visit */
        if (ready) h_zeroed = gru_episode_rule<LearnPub>(PD.episode.terminated, PD.episode.pending, PD.gru.hidden_state, cell.hidden, e, k);
      }
      [[maybe_unused]] int hist_c = 0;
      if constexpr (HIST) { /* the episode rule of the history (gq_policy_hist.h), before anything of this visit is staged */
        if (ready) hist_c = hist_episode_rule<LearnPub>(PD.episode.terminated, PD.episode.pending, hist_ctl, e, k);
      }
      if constexpr (LEARN) { /* the visit of the window law (gq_learn.h): step k - 1 is evaluated, the window flushed at k % D == 0 */
        const GQ_MODEL LearnFeetDev& LF = *mptr(P.learn);
        if (LF.learn.has_reward && ready) learn_visit<LMODE == 2, LearnPub>(LF, obs + (size_t)e * od, MB.act + (size_t)e * 12, P.held + (size_t)e * 12, e, k, D, N);
      }
      /* (the observation words are read AFTER the count has been seen: the ballot below waits for every lane's count) */
      for (uint64_t todo = ballot(fresh); todo != 0;) {
        uint64_t tile = 0, t = todo;
        int src = -1;                                /* the lane whose env is row lane & 15 of this tile */
        for (int r = 0; r < GQ_MLP_ROWS && t != 0; r++) {
          const int f = ffs64(t);
          if ((lane & 15) == r) src = f;
          tile |= (uint64_t)1 << f; t &= t - 1;
        }
        todo &= ~tile;
        const int er = shfl_idx(e, src < 0 ? 0 : src);
        RowSrc rs{}; /* the sources of this lane's row */
        rs.obs = obs + (size_t)er * od;
        rs.last = P.last + (size_t)er * 12;
        if constexpr (LEARN) { /* the row as the network is fed it, before shift / scale */
          const int kr = shfl_idx(k, src < 0 ? 0 : src);
          float* const rec = mptr(P.learn)->learn.policy_obs;
          if (rec) rs.rec = rec + ((size_t)(kr / D) * N + er) * in_dim;
        }
        if constexpr (SCAN) {
          if (src >= 0) rs.z_base = ld_pub(rs.obs + scan_col_z);
          rs.hits = scan_hits + (size_t)er * (size_t)row_law.cells * 3;
        }
        if constexpr (HIST) {
          rs.hist_ctl = shfl_idx(hist_c, src < 0 ? 0 : src);
          rs.hist = hist_state + (size_t)er * hist_env_floats(hist);
        }
        [[maybe_unused]] RowNoise rz = row_noise;
        if constexpr (NOISE) { /* the row's key: the counter of the action noise drawn at this policy step, and the env's global id */
          const int kr = shfl_idx(k, src < 0 ? 0 : src);
          rz.step = (uint32_t)(P.step0 + kr); rz.gid = (uint32_t)(er + P.env_id_offset);
          if constexpr (LEARN) { /* the true rows, laid out as policy_obs is: one distance serves every row */
            float* const rec0 = mptr(P.learn)->learn.policy_obs;
            if (noise_clean && rec0) rz.clean_delta = noise_clean - rec0;
          }
        }
        const auto x_value = [&](const int, const int c) {
          if constexpr (NOISE) return src < 0 ? 0.0f : policy_row_value<SCAN, HIST, LearnPub, true>(row_law, rs, c, rz);
          else return src < 0 ? 0.0f : policy_row_value<SCAN, HIST, LearnPub>(row_law, rs, c);
        };
        const float* out;
        if constexpr (GRU) {
          const int H = cell.hidden;
          const bool zr = shfl_idx((int)h_zeroed, src < 0 ? 0 : src) != 0;
          const int kr = shfl_idx(k, src < 0 ? 0 : src);
          const float* const hrow = PD.gru.hidden_state + (size_t)er * H;
          float* const hrec = PD.gru.hidden_seq ? PD.gru.hidden_seq + ((size_t)(kr / D) * N + er) * H : nullptr; /* the state as the cell is fed it */
          wave_barrier(); /* whoever still read the buffers has done so */
          gru_tile_stage(mlp_kp(in_dim), &xt[0][0], x_value);
          gru_tile_stage(mlp_np(H), &xt[1][0], [&](const int, const int c) {
            if (src < 0 || c >= H) return 0.0f;
            const float v = zr ? 0.0f : ld_pub(hrow + c);
            if (hrec) hrec[c] = v;
            return v;
          });
          const bool owns = fresh && ((tile >> lane) & 1);
          const int hslot = popc64(tile & (((uint64_t)1 << lane) - 1));
          out = gru_tile_forward(cell, net, PD.gru.blob, P.blob, &xt[0][0], [&](const float* hn) { /* h': by the env's own lane, like acc / wstate */
            if (owns)
              for (int c = 0; c < H; c++) st_pub(PD.gru.hidden_state + (size_t)e * H + c, hn[c * GQ_MLP_ROWS + hslot]);
          });
        } else {
          mlp_tile_stage(net, xt[0], x_value);
          out = mlp_tile_forward(net, P.blob, xt[0], xt[1]);
        }
        if (fresh && ((tile >> lane) & 1)) {
          if constexpr (HIST) hist_push<LearnPub>(hist_ctl, e, hist_c); /* the frame just staged is the newest: by the env's own lane */
          const int slot = popc64(tile & (((uint64_t)1 << lane) - 1));
          const uint32_t gid = (uint32_t)(e + P.env_id_offset);
#pragma unroll
          for (int j = 0; j < 12; j++) {
#pragma clang fp contract(off)
            float v = out[j * GQ_MLP_ROWS + slot];
            if constexpr (LEARN) {
              const GQ_MODEL LearnDev& L = mptr(P.learn)->learn;
              if (L.policy_means) L.policy_means[((size_t)(k / D) * N + e) * 12 + j] = v;
            }
            const float sg = P.sigma[j];
            if (sg > 0.0f) {
              const uint32_t x0 = philox4x32((uint32_t)j, (uint32_t)(P.step0 + k), gid, GQ_MLP_NOISE_STREAM, P.seed_lo, P.seed_hi, 0);
              const uint32_t x1 = philox4x32((uint32_t)j, (uint32_t)(P.step0 + k), gid, GQ_MLP_NOISE_STREAM, P.seed_lo, P.seed_hi, 1);
              const float nz = sg * mlp_normal(x0, x1);
              v = v + nz;
            }
            if (P.clip > 0.0f) v = fminf(fmaxf(v, -P.clip), P.clip);
            a[j] = v;
            if constexpr (LEARN) { /* the action before the held one; a_prev := a in the first window of a call */
              const GQ_MODEL LearnDev& L = mptr(P.learn)->learn;
              if (L.has_reward) st_pub(L.prev + (size_t)e * 12 + j, k == 0 ? v : ld_pub(P.held + (size_t)e * 12 + j));
            }
            st_pub(P.held + (size_t)e * 12 + j, v);
            if (P.feed_last) st_pub(P.last + (size_t)e * 12 + j, v);
            if (P.policy_actions) P.policy_actions[((size_t)(k / D) * N + e) * 12 + j] = v;
          }
        }
      }
      if (!ready) continue;
      if constexpr (LEARN) {
        if (k == K) { P.issued[e] = K + 1; progress = true; continue; } /* the closing visit: nothing is pushed */
      }
      const float* row = obs + (size_t)e * od;
      float qj[12], qd[12];
#pragma unroll
      for (int j = 0; j < 12; j++) {
        qj[j] = ld_pub(row + P.col_q[j]); qd[j] = ld_pub(row + P.col_qd[j]);
        if (!fresh) a[j] = ld_pub(P.held + (size_t)e * 12 + j);
      }
      /* the action row and the push ticket travel together */
      const int s = mb_push_ticket(tail);
#pragma unroll
      for (int j = 0; j < 12; j++) {
#pragma clang fp contract(off)
        const float sa = P.action_scale[j] * a[j];
        const float q_des = P.q_default[j] + sa;
        const float u = joint_cmd_law(q_des, 0.0f, 0.0f, P.kp[j], P.kd[j], qj[j], qd[j]);
        st_pub(MB.act + (size_t)e * 12 + j, u);
        if (MB.act_seq) MB.act_seq[((size_t)k * N + e) * 12 + j] = u;
      }
      mb_push_item(items, qmask, qshift, s, e); /* after the action is in place */
      P.issued[e] = k + 1;
      progress = true;
    }
    /* (all_done / progress are per lane, as in policy_pd_kernel: the wavefront goes on while any lane has work, and a lane that leaves
     * the loop early would miss the tile work of the others - so the exits below are taken by the whole wavefront) */
    const bool any_live = ballot(!all_done) != 0, any_progress = ballot(progress) != 0;
    if (!any_live) break;
    if (any_progress) { t_last = wall_clock64(); continue; }
    GQ_MB_POLICY_IDLE(lane == 0, rank * GQ_WAVE)
  }
}

/* the network alone over rows [n][in_dim] (gq_policy_mlp_eval): the two forms of the law side by side, so that their bits can be compared.
 * shift / scale act on the first in_obs columns, as in the rollout. */
__global__ void __launch_bounds__(GQ_WAVE) policy_mlp_eval_row_kernel(const PolicyDev* __restrict__ Pp, const float* __restrict__ rows, const int n, float* __restrict__ out) {
  const GQ_MODEL PolicyMlpDev& P = mptr(Pp)->seat;
  const MlpNet net = mlp_net_load(P.net);
  const int r = (int)(blockIdx.x * GQ_WAVE + threadIdx.x);
  if (r >= n) return;
  float x[GQ_MLP_MAXW], y[GQ_MLP_ROWS];
  for (int c = 0; c < net.in_dim; c++) { const float v = rows[(size_t)r * net.in_dim + c]; x[c] = c < P.in_obs ? mlp_obs_in(v, P.shift, P.scale, c) : v; }
  mlp_row_forward(net, P.blob, x, y);
  for (int j = 0; j < 12; j++) out[(size_t)r * 12 + j] = y[j];
}
__global__ void __launch_bounds__(GQ_WAVE) policy_mlp_eval_tile_kernel(const PolicyDev* __restrict__ Pp, const float* __restrict__ rows, const int n, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xt[2][GQ_MLP_MAXW * GQ_MLP_ROWS];
  const GQ_MODEL PolicyMlpDev& P = mptr(Pp)->seat;
  const MlpNet net = mlp_net_load(P.net);
  const int lane = (int)threadIdx.x, r0 = (int)blockIdx.x * GQ_MLP_ROWS, in_dim = net.in_dim, in_obs = P.in_obs;
  const float* const shift = P.shift;
  const float* const scale = P.scale;
  mlp_tile_stage(net, xt[0], [&](const int r, const int c) {
    if (r0 + r >= n || c >= in_dim) return 0.0f;
    const float v = rows[(size_t)(r0 + r) * in_dim + c];
    return c < in_obs ? mlp_obs_in(v, shift, scale, c) : v;
  });
  const float* const y = mlp_tile_forward(net, P.blob, xt[0], xt[1]);
  for (int w = lane; w < GQ_MLP_ROWS * 12; w += GQ_WAVE) {
    const int r = w / 12, j = w % 12;
    if (r0 + r < n) out[(size_t)(r0 + r) * 12 + j] = y[j * GQ_MLP_ROWS + r];
  }
}

/* the recurrent policy alone over rows [n][in_dim] and states [n][H] (gq_policy_gru_eval): the two forms of gq_policy_gru.h side by side.
 * gru.hidden_state: h_in, gru.hidden_seq: h_out (read / written plainly: nothing else runs on them) */
__global__ void __launch_bounds__(GQ_WAVE) policy_gru_eval_row_kernel(const PolicyDev* __restrict__ Pp, const float* __restrict__ rows, const int n, float* __restrict__ out) {
  const GQ_MODEL PolicyMlpDev& P = mptr(Pp)->seat;
  const GQ_MODEL GruDev& GP = mptr(Pp)->gru;
  const MlpNet head = mlp_net_load(P.net);
  const GruNet cell = gru_net_load(GP.cell);
  const int r = (int)(blockIdx.x * GQ_WAVE + threadIdx.x), H = cell.hidden;
  if (r >= n) return;
  float x[GQ_MLP_MAXW], h[GQ_GRU_MAXH], hn[GQ_GRU_MAXH], y[GQ_MLP_ROWS];
  for (int c = 0; c < cell.in_dim; c++) { const float v = rows[(size_t)r * cell.in_dim + c]; x[c] = c < P.in_obs ? mlp_obs_in(v, P.shift, P.scale, c) : v; }
  for (int c = 0; c < H; c++) h[c] = GP.hidden_state[(size_t)r * H + c];
  gru_row_forward(cell, head, GP.blob, x, h, y, hn);
  for (int j = 0; j < 12; j++) out[(size_t)r * 12 + j] = y[j];
  for (int c = 0; c < H; c++) GP.hidden_seq[(size_t)r * H + c] = hn[c];
}
__global__ void __launch_bounds__(GQ_WAVE) policy_gru_eval_tile_kernel(const PolicyDev* __restrict__ Pp, const float* __restrict__ rows, const int n, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xt[GQ_GRU_LDS_FLOATS];
  const GQ_MODEL PolicyMlpDev& P = mptr(Pp)->seat;
  const GQ_MODEL GruDev& GP = mptr(Pp)->gru;
  const MlpNet head = mlp_net_load(P.net);
  const GruNet cell = gru_net_load(GP.cell);
  const int lane = (int)threadIdx.x, r0 = (int)blockIdx.x * GQ_MLP_ROWS, in_dim = cell.in_dim, in_obs = P.in_obs, H = cell.hidden;
  const float* const shift = P.shift;
  const float* const scale = P.scale;
  const float* const h_in = GP.hidden_state;
  float* const h_out = GP.hidden_seq;
  gru_tile_stage(mlp_kp(in_dim), xt, [&](const int r, const int c) {
    if (r0 + r >= n || c >= in_dim) return 0.0f;
    const float v = rows[(size_t)(r0 + r) * in_dim + c];
    return c < in_obs ? mlp_obs_in(v, shift, scale, c) : v;
  });
  gru_tile_stage(mlp_np(H), xt + GQ_GRU_REGION, [&](const int r, const int c) { return (r0 + r >= n || c >= H) ? 0.0f : h_in[(size_t)(r0 + r) * H + c]; });
  const float* const y = gru_tile_forward(cell, head, GP.blob, P.blob, xt, [&](const float* hn) {
    for (int w = lane; w < GQ_MLP_ROWS * H; w += GQ_WAVE) {
      const int r = w / H, c = w % H;
      if (r0 + r < n) h_out[(size_t)(r0 + r) * H + c] = hn[c * GQ_MLP_ROWS + r];
    }
  });
  for (int w = lane; w < GQ_MLP_ROWS * 12; w += GQ_WAVE) {
    const int r = w / 12, j = w % 12;
    if (r0 + r < n) out[(size_t)(r0 + r) * 12 + j] = y[j * GQ_MLP_ROWS + r];
  }
}

/* the step law alone over rows [n][od] (gq_reward_eval, and gq_reward_eval_feet with FEET), lane = row: what policy_mlp_eval_* is for the
 * network - learn_step's bits, to be compared with the host's.  torques / act / act_prev: [n][12], read only by the terms that need them
 * (may be NULL then); terminated: [n] or NULL.  FEET: air_in / air_out [n][4], the state before and after the row's step (read and written
 * only with air_time on; may be NULL then - and may be the same tensor: a lane reads its row before it writes it) */
template <bool FEET>
__global__ void __launch_bounds__(GQ_WAVE) reward_eval_kernel(const LearnFeetDev* __restrict__ Lp, const float* __restrict__ rows, const int od, const float* __restrict__ torques,
                                                              const float* __restrict__ act, const float* __restrict__ act_prev, const uint8_t* __restrict__ terminated,
                                                              const float* air_in, const int n, float* __restrict__ out, float* air_out) {
  const RewardLaw R = reward_law_load(mptr(Lp)->learn.law);
  FootLaw F;
  if constexpr (FEET) F = foot_law_load(mptr(Lp)->feet);
  const int r = (int)(blockIdx.x * GQ_WAVE + threadIdx.x);
  if (r >= n) return;
  const float* const row = rows + (size_t)r * od;
  float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  out[r] = learn_step<FEET>(R, F, true, terminated ? (int)terminated[r] : 0, [&](const int c) { return row[c]; }, [&](const int i) { return air_in[(size_t)r * 4 + i]; },
                            [&](const int j) { return torques[(size_t)r * 12 + j]; }, [&](const int j) { return act[(size_t)r * 12 + j]; },
                            [&](const int j) { return act_prev[(size_t)r * 12 + j]; }, t);
  if constexpr (FEET) {
    if (F.w[FW_AIR_TIME] != 0.0f) {
#pragma unroll
      for (int i = 0; i < 4; i++) air_out[(size_t)r * 4 + i] = t[i];
    }
  }
}

/* the scan law alone (gq_height_scan_eval), a thread per cell: hits [n][cells][3], z [n] -> out [n][cells]; height_scan_cell's bits, to be
 * compared with the rollout's and the host's */
__global__ void __launch_bounds__(GQ_WAVE) height_scan_eval_kernel(const ScanLaw law, const float* __restrict__ hits, const float* __restrict__ z, const long long total,
                                                                   const int cells, float* __restrict__ out) {
  const long long w = (long long)blockIdx.x * GQ_WAVE + threadIdx.x;
  if (w >= total) return;
  out[w] = height_scan_cell(law, z[w / cells], hits[w * 3 + 2]);
}

/* the sensor noise's law alone (gq_obs_noise_eval), a thread per word: rows [n][in_dim] raw input rows, steps / env_ids [n] each row's
 * key -> out [n][in_dim]; obs_noise_add's bits, to be compared with the rollout's and the host's */
__global__ void __launch_bounds__(GQ_WAVE) obs_noise_eval_kernel(const NoiseLaw law, const int in_obs, const int cells, const int in_dim, const float* __restrict__ rows,
                                                                 const int32_t* __restrict__ steps, const int32_t* __restrict__ env_ids, const long long total,
                                                                 float* __restrict__ out) {
  const long long w = (long long)blockIdx.x * GQ_WAVE + threadIdx.x;
  if (w >= total) return;
  const long long r = w / in_dim;
  const int c = (int)(w - r * in_dim);
  out[w] = obs_noise_add(law, obs_noise_amp(law, in_obs, cells, c), c, (uint32_t)steps[r], (uint32_t)env_ids[r], rows[w]);
}

/* which XCDs does this device expose?  bit HW_REG_XCC_ID of *mask is set by every workgroup */
__global__ void xcc_probe_kernel(int32_t* mask) {
  if (threadIdx.x == 0) atomicOr(mask, 1 << xcc_id());
}

#endif /* GQ_IN_MISC */
template <bool BOXES>
__global__ void __launch_bounds__(GQ_WAVE) reset_kernel(ResetArgs a) {
  if (a.mask && !gptr(a.mask)[wave_index()]) return;
  __shared__ WaveMem W;
#if GQ_TICKSET
  if (lane_id() == 0) W.tk_T = nullptr;
#endif
  reset_wave<BOXES>(a, W);
}

#if GQ_IN_MISC
/* HeightMap rays: one wavefront per env, lane = cell (strided when the grid has more than 64).  Scene = the floor plane z = 0
 * plus the static world boxes (mj_ray against static geoms, heightmap.py:90-99): the nearest hit of the vertical ray with any
 * box (slab test in the box frame).  The env's whole grid lies within a circle around `center`: lane = box first picks the
 * boxes whose bounding circle meets it (two ballots), the rays then walk those few instead of every box of the scene (a
 * thread per ray looping over the 100 boxes of random_boxes took 21.7 us per step of config 5). */
__global__ void __launch_bounds__(GQ_WAVE) heightmap_kernel(const GQ_GLOBAL GqDevModel* model, const double* center, int center_stride, const float* yaw, int yaw_stride, int n_envs, int rows, int cols,
                                 float dist_x, float dist_y, float* out) {
  const int env = (int)blockIdx.x;
  center += (size_t)env * center_stride; yaw += (size_t)env * yaw_stride; /* row strides in elements: views of qpos / the observation row work in place */
  heightmap_rays(*model, center[0], center[1], center[2], cosf(yaw[0]), sinf(yaw[0]), rows, cols, dist_x, dist_y, out + (size_t)env * rows * cols * 3);
}

/* mj_jac for one world point per env (include/gq.h gq_jac): kinematics of the env's pose, then lane = dof writes its
 * column: free-joint translations e_k, rotations (base axis a) a x (p - base), hinge on the body's chain axis x (p - anchor). */
__global__ void __launch_bounds__(GQ_WAVE) jac_kernel(const GqDevModel* model, const double* qpos, int body, const double* point, float* jacp, float* jacr) {
  __shared__ WaveMem W;
  const int lane = lane_id(), env = (int)blockIdx.x;
#if GQ_TICKSET
  if (lane == 0) W.tk_T = nullptr;
#endif
  const GQ_MODEL GqDevModel& m = *mptr(model);
  load_qpos_row(W, qpos + (size_t)env * 19, lane);
  wave_barrier();
  stage_kinematics(W, link_fetch(m, lane));
  /* the point relative to the base x/y (f64 first, like everything else) */
  const V3 p = v3((float)(point[(size_t)env * 3] - W.bxy[0]), (float)(point[(size_t)env * 3 + 1] - W.bxy[1]), (float)point[(size_t)env * 3 + 2]);
  if (lane < GQ_NVD) {
    const int kb = body - 1; /* kernel body index: 0 base, 1 + 3 leg + link */
    V3 jp = v3(0.0f, 0.0f, 0.0f), jr = v3(0.0f, 0.0f, 0.0f);
    if (lane < 3) jp = v3(lane == 0, lane == 1, lane == 2);
    else if (lane < 6) {
      const float* R = W.xmat[0];
      const V3 ax = v3(R[lane - 3], R[3 + lane - 3], R[6 + lane - 3]);
      jr = ax; jp = cross(ax, p - v3(0.0f, 0.0f, W.basez));
    } else {
      const int j = lane - 6, leg = j / 3, depth = j % 3;
      if (kb > 0 && (kb - 1) / 3 == leg && (kb - 1) % 3 >= depth) {
        const V3 ax = ld3(W.u.dyn.axis[j]);
        jr = ax; jp = cross(ax, p - ld3(W.u.dyn.anchor[j]));
      }
    }
    if (jacp) { float* o = jacp + (size_t)env * 54; o[lane] = jp.x; o[18 + lane] = jp.y; o[36 + lane] = jp.z; }
    if (jacr) { float* o = jacr + (size_t)env * 54; o[lane] = jr.x; o[18 + lane] = jr.y; o[36 + lane] = jr.z; }
  }
}

/* mj_ray against the static geoms (include/gq.h gq_ray): one thread per ray; floor plane z = 0, world boxes (slab test in the
 * box frame), height field (the cells under the ray's ground track are walked, two triangles each; gq_camera.h) */
__global__ void ray_kernel(const GQ_GLOBAL GqDevModel* model, const double* origin, const float* dir, int total, float* dist_out, int32_t* geom_out) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (idx >= total) return;
  const GQ_GLOBAL GqDevModel& M = *model;
  const double o[3] = {origin[(size_t)idx * 3], origin[(size_t)idx * 3 + 1], origin[(size_t)idx * 3 + 2]};
  const double d[3] = {(double)dir[(size_t)idx * 3], (double)dir[(size_t)idx * 3 + 1], (double)dir[(size_t)idx * 3 + 2]};
  double best = -1.0;
  int geom = -1;
  if (d[2] < 0.0 && o[2] >= 0.0) { best = -o[2] / d[2]; geom = 0; }   /* the floor: a one-sided plane, hit from above */
  for (int b = 0; b < M.nbox; b++) {
    const GQ_GLOBAL GqDevBox& B = M.box[b];
    const double r[3] = {o[0] - (double)B.pos[0], o[1] - (double)B.pos[1], o[2] - (double)B.pos[2]};
    double tin = -1e300, tout = 1e300;
    if (!ray_box(B, r, d, tin, tout) || tout < 0.0) continue;
    const double t = tin >= 0.0 ? tin : tout; /* origin inside the box: the exit point, like mju_rayGeom */
    if (best < 0.0 || t < best) { best = t; geom = 1 + b; }
  }
  if (M.hf_nrow > 0) {
    const double ol[3] = {o[0] - (double)M.hf_pos[0], o[1] - (double)M.hf_pos[1], o[2] - (double)M.hf_pos[2]};
    const double tb = ray_hfield(M, ol, d, 0.0);
    if (tb >= 0.0 && (best < 0.0 || tb < best)) { best = tb; geom = 1 + M.nbox; }
  }
  dist_out[idx] = (float)best;
  if (geom_out) geom_out[idx] = geom;
}

/* gq_camera (gq_camera.h): the pose pass, one wavefront per env, and the pixel pass, grid (tiles, envs) */
__global__ void __launch_bounds__(GQ_WAVE) camera_pose_kernel(const GqDevModel* model, const CamCall c) {
  __shared__ WaveMem W;
  camera_pose_wave(W, *mptr(model), c, (int)blockIdx.x);
}
__global__ void __launch_bounds__(GQ_WAVE) camera_pixel_kernel(const GQ_GLOBAL GqDevModel* model, const CamCall c) {
  camera_tile_wave<false>(*model, c, nullptr, (int)blockIdx.x, (int)blockIdx.y);
}
/* gq_camera_shaded: the same pixel pass, plus the RGBA image */
__global__ void __launch_bounds__(GQ_WAVE) camera_shade_kernel(const GQ_GLOBAL GqDevModel* model, const CamCall c, const CamShade s) {
  camera_tile_wave<true>(*model, c, &s, (int)blockIdx.x, (int)blockIdx.y);
}
/* gq_camera_layered: the ghost pose pass, grid (ghosts, envs), then the shaded pixel pass with the layers composited */
__global__ void __launch_bounds__(GQ_WAVE) camera_ghost_kernel(const GqDevModel* model, const CamCall c, const CamLayers l) {
  __shared__ WaveMem W;
  camera_ghost_wave(W, *mptr(model), c, l, (int)blockIdx.x, (int)blockIdx.y);
}
__global__ void __launch_bounds__(GQ_WAVE) camera_layer_kernel(const GQ_GLOBAL GqDevModel* model, const CamCall c, const CamShade s, const CamLayers l) {
  camera_tile_wave<true, true>(*model, c, &s, (int)blockIdx.x, (int)blockIdx.y, &l);
}

#endif /* GQ_IN_MISC */

/* ---- the kernel variants (Key, gq_step_kernel.h), the part that builds each, and the run-time dispatch to them. */
/* part 0: the non-template kernels and the launch entry points; 1-18: step variants by solver and cone x mode x flat or world scene;
 * 19-22: mailbox variants by cone x flat or world scene; 23-31: step variants of the two split flat self-collision scenes (_HULL, _PRIM)
 * by solver and cone x mode; 32-33: their mailbox variants by cone.  Each part is one translation unit (-DGQ_PART=k); the Makefile's
 * NPARTS is checked. */
constexpr bool scene_split(Scene s) { return s == SCENE_FLAT_SELF_HULL || s == SCENE_FLAT_SELF_PRIM; }
constexpr int part_of(Key k) {
  const int world = scene_boxes(Scene(k.scene));
  if (scene_split(Scene(k.scene))) return k.mailbox ? 32 + k.cone : 23 + (k.solver + k.cone) * 3 + k.mode;
  return k.mailbox ? 19 + 2 * k.cone + world : 1 + ((k.solver + k.cone) * 3 + k.mode) * 2 + world;
}
constexpr int kParts = part_of({1, 0, 1, SCENE_FLAT_SELF_PRIM, 1}) + 1;
#ifdef GQ_NPARTS
static_assert(GQ_NPARTS == kParts, "csrc/Makefile NPARTS does not match part_of()");
#endif
/* Development builds (make dev, tools/dev_build.sh: -DGQ_DEV_ONLY=<cone>, one unit, a 15 s build for A/B timing of kernel experiments
 * through GQ_LIBGQ_PATH) carry the Newton step variants of one cone and one scene - flat + self-collision, -DGQ_DEV_BOXES=1 world hull,
 * =2 world prim - without the stage cut unless -DGQ_DEV_CUTS=1, and the flat self-collision mailbox variant; any other step launch aborts.
 * The flat self-collision scene is the one -DGQ_DEV_SELF names: 0 both pair routines (b2, go1 - and every robot when the build also has
 * -DGQ_SCENE_SPLIT_OFF), 1 SCENE_FLAT_SELF_HULL (mini_cheetah, hyqreal1, spot), 2 SCENE_FLAT_SELF_PRIM (go2, aliengo, hyqreal2, capsule mode). */
#ifdef GQ_DEV_ONLY
#ifndef GQ_DEV_BOXES
#define GQ_DEV_BOXES 0
#endif
#ifndef GQ_DEV_CUTS
#define GQ_DEV_CUTS 0
#endif
#ifndef GQ_DEV_SELF
#define GQ_DEV_SELF 0
#endif
constexpr Scene kDevFlat = GQ_DEV_SELF == 2 ? SCENE_FLAT_SELF_PRIM : GQ_DEV_SELF ? SCENE_FLAT_SELF_HULL : SCENE_FLAT_SELF;
constexpr Scene kDevScene = GQ_DEV_BOXES == 2 ? SCENE_WORLD_PRIM : GQ_DEV_BOXES ? SCENE_WORLD_HULL : kDevFlat;
constexpr bool in_build(Key k) {
  return k.solver == 1 && k.cone == (GQ_DEV_ONLY != 0) && (k.mode != 2 || GQ_DEV_CUTS) && k.scene == (k.mailbox ? kDevFlat : kDevScene);
}
#else
constexpr bool in_build(Key) { return true; }
#endif
/* does the unit of part `part` (-1: the single-unit build) instantiate variant k? */
constexpr bool compiled_in(Key k, int part) { return key_exists(k) && in_build(k) && (part < 0 || part_of(k) == part); }

struct Launch { Key key; const FusedArgs* args; const StepCall* c; const MailboxDev* mb; int grid /* workgroups */; hipStream_t stream; };
template <int S, int M, int CONE, int SC, int MB>
static void launch_variant(const Launch& L) {
  constexpr bool C = CONE, B = scene_boxes(Scene(SC)), SF = scene_self(Scene(SC)), P = scene_prim(Scene(SC));
  constexpr bool NOCVX = !kernel_cvx(Scene(SC)); /* the self stage without the convex block: the _prim kernels */
  static_assert(!NOCVX || (!B && P), "step_kernel_prim is the flat scene with the box routines");
  StepCall call = *L.c;
  if constexpr (MB) {
    if constexpr (NOCVX) hipLaunchKernelGGL((mailbox_step_kernel_prim<S, C>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call, L.mb);
    else hipLaunchKernelGGL((mailbox_step_kernel<S, C, B, SF, P>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call, L.mb);
  } else {
    if constexpr (M == 0) {
      if (call.n_steps > 1 || call.policy) { /* persistent rollout (also a one-step one with the policy inline: only this variant evaluates it): production kernel only */
        if constexpr (S == 1) if (policy_is_foot_cmd(call.policy)) { /* gq_step_foot_cmd: the variants that hold its law */
          if constexpr (NOCVX) hipLaunchKernelGGL((step_kernel_prim_foot<C>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call);
          else hipLaunchKernelGGL((step_kernel_foot<C, B, SF, P>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call);
          return;
        }
        if constexpr (NOCVX) hipLaunchKernelGGL((step_kernel_prim<S, M, C, true>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call);
        else hipLaunchKernelGGL((step_kernel<S, M, C, B, SF, P, true>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call);
        return;
      }
    }
    call.n_steps = 1;
    if constexpr (NOCVX) hipLaunchKernelGGL((step_kernel_prim<S, M, C>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call);
    else hipLaunchKernelGGL((step_kernel<S, M, C, B, SF, P>), dim3(L.grid), dim3(GQ_WAVE), 0, L.stream, L.args, call);
  }
}
/* launches L's variant if the unit of part PART instantiates it; false otherwise */
template <int PART>
static bool dispatch(const Launch& L) {
  return for_variant(L.key, [&](auto S, auto M, auto C, auto SC, auto MB) {
    if constexpr (!compiled_in({S, M, C, SC, MB}, PART)) return false;
    else { launch_variant<S, M, C, SC, MB>(L); return true; }
  });
}
/* the entry point of part PART > 0, instantiated in that part's unit only */
template <int PART> bool launch_part(const Launch& L);
#if GQ_PART > 0
template <int PART> bool launch_part(const Launch& L) { return dispatch<PART>(L); }
template bool launch_part<GQ_PART>(const Launch&);
#endif
#if GQ_IN_MISC
template <int... I>
static bool launch_in_part(const Launch& L, std::integer_sequence<int, I...>) {
  static constexpr bool (*entry[])(const Launch&) = {&launch_part<I + 1>...};
  return entry[part_of(L.key) - 1](L);
}
static bool launch_key(const Launch& L) {
#if GQ_PART < 0
  return dispatch<-1>(L);
#else
  return launch_in_part(L, std::make_integer_sequence<int, kParts - 1>{});
#endif
}
#endif /* GQ_IN_MISC */
}  // namespace gq

#if GQ_IN_MISC
extern "C" void gq_launch_step(const gq::FusedArgs* dev_args, const gq::StepCall* c, int n_envs, int solver, int cone, gq::Scene scene, hipStream_t stream) {
  const gq::Key k = gq::step_key(solver, cone, scene, c->debug != nullptr, c->stop_stage, 0);
  if (!gq::launch_key({k, dev_args, c, nullptr, n_envs, stream})) {
    fprintf(stderr, "libgq: step-kernel variant solver=%d mode=%d cone=%d scene=%d is not compiled into this build\n", k.solver, k.mode, k.cone, k.scene);
    abort();
  }
}
/* returns 0 if the scene / solver combination has no mailbox variant compiled in */
extern "C" int gq_launch_mailbox_step(const gq::FusedArgs* dev_args, const gq::StepCall* c, const gq::MailboxDev* mb, int waves, int solver, int cone, gq::Scene scene, hipStream_t stream) {
  return gq::launch_key({gq::step_key(solver, cone, scene, false, 0, 1), dev_args, c, mb, waves, stream}) ? 1 : 0;
}
extern "C" void gq_launch_reset(const gq::ResetArgs* a, int n_envs, gq::Scene scene, hipStream_t stream) {
  if (gq::scene_boxes(scene)) hipLaunchKernelGGL(gq::reset_kernel<true>, dim3(n_envs), dim3(GQ_WAVE), 0, stream, *a);
  else hipLaunchKernelGGL(gq::reset_kernel<false>, dim3(n_envs), dim3(GQ_WAVE), 0, stream, *a);
}
extern "C" void gq_launch_heightmap(const GQ_GLOBAL GqDevModel* model, const double* center, int center_stride, const float* yaw, int yaw_stride, int n_envs, int rows, int cols,
                                    float dist_x, float dist_y, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(gq::heightmap_kernel, dim3(n_envs), dim3(GQ_WAVE), 0, stream, model, center, center_stride, yaw, yaw_stride, n_envs, rows, cols, dist_x, dist_y, out);
}
extern "C" void gq_launch_xcc_probe(int32_t* mask, hipStream_t stream) {
  hipLaunchKernelGGL(gq::xcc_probe_kernel, dim3(4096), dim3(GQ_WAVE), 0, stream, mask);
}
extern "C" void gq_launch_policy_pd(const gq::MailboxDev* mb, const gq::PolicyPdDev* pd, const float* obs, int od, int waves, hipStream_t stream) {
  hipLaunchKernelGGL(gq::policy_pd_kernel, dim3(waves), dim3(GQ_WAVE), 0, stream, mb, pd, obs, od);
}
/* THE TABLE of policy_mlp_kernel's instantiations, MODE = learn mode (0: gq_rollout_policy, 1: the learning half, 2: with the foot terms)
 * | 4 recurrent | 8 height scan | 16 observation history (the MLP's alone) | 32 sensor noise: listed here and nowhere else - the array below instantiates
 * them, the loop dispatches to them.  Returns whether `mode` is in the table (nothing was launched otherwise). */
using PolicyModes = std::integer_sequence<int, 0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 16, 17, 18, 24, 25, 26,
                                          32, 33, 34, 36, 37, 38, 40, 41, 42, 44, 45, 46, 48, 49, 50, 56, 57, 58>; /* | 32: each with the sensor noise */
template <int... M>
static bool launch_policy_mode(std::integer_sequence<int, M...>, const int mode, const gq::MailboxDev* mb, const gq::PolicyDev* dev, const float* obs, int od, int waves, hipStream_t stream) {
  using Kernel = void (*)(const gq::MailboxDev*, const gq::PolicyDev*, const float*, int);
  static constexpr int modes[] = {M...};
  static constexpr Kernel kernels[] = {&gq::policy_mlp_kernel<M>...};
  for (size_t i = 0; i < sizeof...(M); i++)
    if (modes[i] == mode) { hipLaunchKernelGGL(kernels[i], dim3(waves), dim3(GQ_WAVE), 0, stream, mb, dev, obs, od); return true; }
  return false;
}
extern "C" int gq_launch_policy(const gq::MailboxDev* mb, const gq::PolicyDev* dev, const float* obs, int od, int waves, int mode, hipStream_t stream) {
  return launch_policy_mode(PolicyModes{}, mode, mb, dev, obs, od, waves, stream) ? 1 : 0;
}
extern "C" void gq_launch_height_scan_eval(const gq::ScanLaw* law, const float* hits, const float* z, int n, int cells, float* out, hipStream_t stream) {
  const long long total = (long long)n * cells;
  hipLaunchKernelGGL(gq::height_scan_eval_kernel, dim3((unsigned)((total + GQ_WAVE - 1) / GQ_WAVE)), dim3(GQ_WAVE), 0, stream, *law, hits, z, total, cells, out);
}
extern "C" void gq_launch_obs_noise_eval(const gq::NoiseLaw* law, int in_obs, int cells, int in_dim, const float* rows, const int32_t* steps, const int32_t* env_ids, int n,
                                         float* out, hipStream_t stream) {
  const long long total = (long long)n * in_dim;
  hipLaunchKernelGGL(gq::obs_noise_eval_kernel, dim3((unsigned)((total + GQ_WAVE - 1) / GQ_WAVE)), dim3(GQ_WAVE), 0, stream, *law, in_obs, cells, in_dim, rows, steps, env_ids,
                     total, out);
}
/* impl 0: gru_row_forward, a thread per row; 1: gru_tile_forward, a wavefront per 16 rows */
extern "C" void gq_launch_policy_gru_eval(const gq::PolicyDev* dev, const float* rows, int n_rows, int impl, float* out, hipStream_t stream) {
  if (impl == 0) hipLaunchKernelGGL(gq::policy_gru_eval_row_kernel, dim3((n_rows + GQ_WAVE - 1) / GQ_WAVE), dim3(GQ_WAVE), 0, stream, dev, rows, n_rows, out);
  else hipLaunchKernelGGL(gq::policy_gru_eval_tile_kernel, dim3((n_rows + GQ_MLP_ROWS - 1) / GQ_MLP_ROWS), dim3(GQ_WAVE), 0, stream, dev, rows, n_rows, out);
}
/* feet 0: gq_reward_eval (air_in / air_out are not looked at), 1: gq_reward_eval_feet */
extern "C" void gq_launch_reward_eval(const gq::LearnFeetDev* learn, const float* rows, int od, const float* torques, const float* act, const float* act_prev,
                                      const uint8_t* terminated, const float* air_in, int n, float* out, float* air_out, int feet, hipStream_t stream) {
  const auto kernel = feet ? gq::reward_eval_kernel<true> : gq::reward_eval_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((n + GQ_WAVE - 1) / GQ_WAVE), dim3(GQ_WAVE), 0, stream, learn, rows, od, torques, act, act_prev, terminated, air_in, n, out, air_out);
}
/* impl 0: mlp_row_forward, a thread per row; 1: mlp_tile_forward, a wavefront per 16 rows */
extern "C" void gq_launch_policy_mlp_eval(const gq::PolicyDev* dev, const float* rows, int n_rows, int impl, float* out, hipStream_t stream) {
  if (impl == 0) hipLaunchKernelGGL(gq::policy_mlp_eval_row_kernel, dim3((n_rows + GQ_WAVE - 1) / GQ_WAVE), dim3(GQ_WAVE), 0, stream, dev, rows, n_rows, out);
  else hipLaunchKernelGGL(gq::policy_mlp_eval_tile_kernel, dim3((n_rows + GQ_MLP_ROWS - 1) / GQ_MLP_ROWS), dim3(GQ_WAVE), 0, stream, dev, rows, n_rows, out);
}
extern "C" void gq_launch_jac(const GqDevModel* model, const double* qpos, int body, const double* point, float* jacp, float* jacr, int n_envs, hipStream_t stream) {
  hipLaunchKernelGGL(gq::jac_kernel, dim3(n_envs), dim3(GQ_WAVE), 0, stream, model, qpos, body, point, jacp, jacr);
}
/* s: null for depth / segmentation only (gq_camera); l: null without layers (gq_camera_shaded), needs s */
extern "C" void gq_launch_camera(const GqDevModel* model, const gq::CamCall* c, const gq::CamShade* s, const gq::CamLayers* l, int n_envs, hipStream_t stream) {
  const dim3 grid(((c->width + GQ_CAM_TILE - 1) / GQ_CAM_TILE) * ((c->height + GQ_CAM_TILE - 1) / GQ_CAM_TILE), n_envs);
  const GQ_GLOBAL GqDevModel* gm = (const GQ_GLOBAL GqDevModel*)model;
  hipLaunchKernelGGL(gq::camera_pose_kernel, dim3(n_envs), dim3(GQ_WAVE), 0, stream, model, *c);
  if (l && l->n_ghost > 0) hipLaunchKernelGGL(gq::camera_ghost_kernel, dim3(l->n_ghost, n_envs), dim3(GQ_WAVE), 0, stream, model, *c, *l);
  if (l) hipLaunchKernelGGL(gq::camera_layer_kernel, grid, dim3(GQ_WAVE), 0, stream, gm, *c, *s, *l);
  else if (s) hipLaunchKernelGGL(gq::camera_shade_kernel, grid, dim3(GQ_WAVE), 0, stream, gm, *c, *s);
  else hipLaunchKernelGGL(gq::camera_pixel_kernel, grid, dim3(GQ_WAVE), 0, stream, gm, *c);
}
extern "C" void gq_launch_ray(const GQ_GLOBAL GqDevModel* model, const double* origin, const float* dir, int total, float* dist, int32_t* geom, hipStream_t stream) {
  hipLaunchKernelGGL(gq::ray_kernel, dim3((total + 127) / 128), dim3(128), 0, stream, model, origin, dir, total, dist, geom);
}
#endif /* GQ_IN_MISC */
