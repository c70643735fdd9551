/*
 * TEST INFRASTRUCTURE - the learning rollout's reward on the host: a stand-alone program around the two routines of
 * gym_quadruped_amd/csrc/gq_learn.h, the definition - learn_step (one step's gather and law, with the foot terms of gq_reward_feet.h) and
 * learn_visit (the window law) - compiled with g++ against the header with tests/simt_emu on the include path.  It plays K steps of S
 * independent sequences: for every sequence the visits k = 0..K exactly as policy_mlp_kernel<2> makes them, with plain loads and stores.
 * Which steps are re-spawn steps is not an input: the law derives it from `terminated` and `pending`.
 *
 *   foot_reward_host IN OUT
 *   IN (32-bit words): f32 w[12], sigma_lin, sigma_ang, base_height_target, dt;  f32 foot w[4], air_time_target, min_cmd_speed, impact_limit,
 *                      clearance_target;  int32 S, K, od, D, the 9 + 12 columns of reward_host, then the 24 foot columns {c[4], vx[4], vy[4],
 *                      fz[4], zb[4], cmd_err[2], cmd_vel[2]} (-1: nothing that is on reads it);  f32 air[S][4] before the first step;
 *                      f32 pending[S] (0 / 1: the sequence spends step 0 on its re-spawn);  then for step k = 0..K-1, for sequence s:
 *                      f32 row[od], u[12], a[12], a_prev[12], terminated (0 / 1).
 *                      D >= 1: the decimation, K a multiple of it.  D == 0: no window law - learn_step alone over the steps with the state
 *                      carried, whatever `terminated` says (what reward_eval computes row by row); pending must be 0.
 *   OUT: per step and sequence 7 f32: the step's reward from learn_step (0 at a re-spawn step), the state t[4] after the step (with D >= 1:
 *        as learn_visit left it), and the law's two threshold decisions restated with the law's own expressions - gate (1: the commanded
 *        speed is above min_cmd_speed, or no gate) and a bit mask of the feet with fz above impact_limit - for a float64 reference that must
 *        take the same branches;  then, with D >= 1, rewards [K / D][S] f32, dones [K / D][S] f32 (0 / 1) and the final air times [S][4].
 * inv_sigma and min_cmd_speed^2 are formed as the library forms them: once, in float32.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gq_learn.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: foot_reward_host IN OUT\n"); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> raw((size_t)bytes / 4);
  if (!raw.empty() && std::fread(raw.data(), 4, raw.size(), f) != raw.size()) { std::fprintf(stderr, "short read\n"); return 1; }
  std::fclose(f);
  const size_t head = 16 + 8 + 4 + 21 + 24;
  if (raw.size() < head) { std::fprintf(stderr, "no header\n"); return 1; }
  gq::LearnFeetDev LF{};
  gq::RewardLaw& R = LF.learn.law;
  for (int i = 0; i < GQ_REWARD_TERMS; i++) R.w[i] = raw[i];
  R.inv_sigma_lin = R.w[gq::RW_TRACK_LIN_VEL] != 0.0f ? 1.0f / raw[12] : 0.0f;
  R.inv_sigma_ang = R.w[gq::RW_TRACK_ANG_VEL] != 0.0f ? 1.0f / raw[13] : 0.0f;
  R.base_height_target = raw[14]; R.dt = raw[15];
  gq::FootLaw& F = LF.feet;
  for (int i = 0; i < GQ_FOOT_TERMS; i++) F.w[i] = raw[16 + i];
  F.air_time_target = raw[20];
  F.min_cmd_speed2 = F.w[gq::FW_AIR_TIME] != 0.0f ? raw[21] * raw[21] : 0.0f;
  F.impact_limit = raw[22]; F.clearance_target = raw[23];
  int32_t h[4 + 21 + 24];
  std::memcpy(h, raw.data() + 24, sizeof h);
  const int S = h[0], K = h[1], od = h[2], D = h[3];
  const int32_t* c = h + 4;
  R.col_lin_err[0] = c[0]; R.col_lin_err[1] = c[1]; R.col_ang_err_z = c[2]; R.col_vz = c[3]; R.col_wxy[0] = c[4]; R.col_wxy[1] = c[5];
  R.col_gxy[0] = c[6]; R.col_gxy[1] = c[7]; R.col_z = c[8];
  for (int j = 0; j < 12; j++) R.col_qd[j] = c[9 + j];
  const int32_t* fc = c + 21;
  for (int i = 0; i < 4; i++) { F.col_c[i] = fc[i]; F.col_vx[i] = fc[4 + i]; F.col_vy[i] = fc[8 + i]; F.col_fz[i] = fc[12 + i]; F.col_zb[i] = fc[16 + i]; }
  F.col_cmd_err[0] = fc[20]; F.col_cmd_err[1] = fc[21]; F.col_cmd_vel[0] = fc[22]; F.col_cmd_vel[1] = fc[23];
  if (S < 0 || K < 0 || od < 1 || D < 0 || (D > 0 && K % D != 0)) { std::fprintf(stderr, "bad header\n"); return 1; }
  for (int i = 0; i < 21 + 24; i++)
    if (c[i] < -1 || c[i] >= od) { std::fprintf(stderr, "column %d out of the row\n", c[i]); return 1; }
  const size_t stride = (size_t)od + 37, steps0 = head + (size_t)S * 5;
  const size_t want = steps0 + (size_t)K * (size_t)S * stride;
  if (raw.size() != want) { std::fprintf(stderr, "size: %zu words, expected %zu\n", raw.size(), want); return 1; }
  const size_t W = D > 0 ? (size_t)(K / D) : 0;
  std::vector<float> air(raw.begin() + (long)head, raw.begin() + (long)(head + (size_t)S * 4));
  std::vector<float> out((size_t)K * (size_t)S * 7 + (D > 0 ? 2 * W * (size_t)S + (size_t)S * 4 : 0));
  /* the words a call of the rollout gives the window law, on the host */
  std::vector<uint8_t> pending((size_t)S), terminated((size_t)S), dones(W * (size_t)S);
  std::vector<float> acc((size_t)S, 0.0f), prev((size_t)S * 12);
  std::vector<int32_t> wstate((size_t)S, 0);
  for (int s = 0; s < S; s++) pending[(size_t)s] = raw[head + (size_t)S * 4 + (size_t)s] != 0.0f;
  LF.learn.has_reward = 1;
  LF.learn.terminated = terminated.data(); LF.learn.pending = pending.data();
  LF.learn.acc = acc.data(); LF.learn.wstate = wstate.data(); LF.learn.prev = prev.data();
  LF.learn.rewards = out.data() + (size_t)K * (size_t)S * 7; LF.learn.dones = dones.data();
  LF.air_time = air.data();
  for (int k = 0; k <= K; k++)
    for (int s = 0; s < S && (k > 0 || D > 0); s++) {
      if (k == 0) { gq::learn_visit<true, gq::LearnPlain>(LF, nullptr, nullptr, nullptr, s, 0, D, S); continue; }
      /* step k - 1: its record, then the visit that evaluates it */
      const float* row = raw.data() + steps0 + ((size_t)(k - 1) * (size_t)S + (size_t)s) * stride;
      float* o = out.data() + ((size_t)(k - 1) * (size_t)S + (size_t)s) * 7;
      float* t = air.data() + (size_t)s * 4;
      const bool respawn = D > 0 && (wstate[(size_t)s] & gq::LEARN_RESPAWN);
      float tn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      o[0] = 0.0f;
      if (!respawn) {
        const int term = row[od + 36] != 0.0f;
        o[0] = gq::learn_step<true>(R, F, true, term, [&](const int col) { return row[col]; }, [&](const int i) { return t[i]; }, [&](const int j) { return row[od + j]; },
                                    [&](const int j) { return row[od + 12 + j]; }, [&](const int j) { return row[od + 24 + j]; }, tn);
        gq::FootIn fin{};
        gq::foot_gather_row(F, [&](const int col) { return row[col]; }, fin);
        float gate = 1.0f, mask = 0.0f;
        if (gq::foot_needs_cmd(F)) {
          const float cx = fin.ex + fin.bvx, cy = fin.ey + fin.bvy;
          gate = std::fmaf(cy, cy, cx * cx) > F.min_cmd_speed2 ? 1.0f : 0.0f;
        }
        if (F.w[gq::FW_IMPACT] != 0.0f)
          for (int i = 0; i < 4; i++)
            if (fin.fz[i] - F.impact_limit > 0.0f) mask += (float)(1 << i);
        o[5] = gate; o[6] = mask;
      }
      if (D > 0) {
        terminated[(size_t)s] = row[od + 36] != 0.0f;
        for (int j = 0; j < 12; j++) prev[(size_t)s * 12 + j] = row[od + 24 + j];
        gq::learn_visit<true, gq::LearnPlain>(LF, row, row + od, row + od + 12, s, k, D, S);
      } else if (F.w[gq::FW_AIR_TIME] != 0.0f) {
        for (int i = 0; i < 4; i++) t[i] = tn[i];
      }
      for (int i = 0; i < 4; i++) o[1 + i] = t[i];
    }
  if (D > 0) {
    float* tail = out.data() + (size_t)K * (size_t)S * 7 + W * (size_t)S;
    for (size_t i = 0; i < W * (size_t)S; i++) tail[i] = dones[i] ? 1.0f : 0.0f;
    std::memcpy(tail + W * (size_t)S, air.data(), sizeof(float) * (size_t)S * 4);
  }
  f = std::fopen(argv[2], "wb");
  if (!f || (!out.empty() && std::fwrite(out.data(), 4, out.size(), f) != out.size())) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
  std::fclose(f);
  return 0;
}
