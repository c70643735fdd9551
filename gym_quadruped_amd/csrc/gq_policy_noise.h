/*
 * gq_policy_noise.h - SENSOR NOISE on the in-loop policy's input row (gq_rollout_policy_noise, gq_obs_noise_eval): the law, defined once for
 * host and device.  Plain C++: compiles with the product's gq_device.h and with the host shim (tests/simt_emu); tests/obs_noise_host.cpp
 * plays it inside policy_row_value, tests/obs_noise_ref.py restates it in numpy.  Contraction off, every operation rounded once; the order
 * below is the definition.
 *
 * THE LAW, for column c of the input row (gq_policy_dev.h) at the policy step with absolute step counter `step` = step0 + k of the env with
 * global id gid:
 *
 *   observation column  c < in_obs, amp[c] > 0:                   o~ = o + amp[c] * n         (a product, a sum: two roundings)
 *   scan column         in_obs <= c < in_obs + cells, scan_amp > 0: s~ = s + scan_amp * n       s: what height_scan_cell returns (after clamp
 *                                                                                             and scale) from the TRUE z of the row
 *   last action, history frames: never.  A frame stores the noisy current-block word AS FED, o~, so frame_i at step s carries what the
 *                       current block carried at step s - i; no fresh draw is made on a frame word.  Shift / scale act on o~ as on o.
 *   amplitude 0         no draw, and the word passes untouched bit for bit (not o + 0, which would turn -0.0 into +0.0)
 *
 *   n, OBS_NOISE_UNIFORM  u = float(x0 >> 8) * 2^-24, n = 2 u - 1: exact in fp32, in [-1, 1)
 *   n, OBS_NOISE_NORMAL   n = mlp_normal(x0, x1) (gq_policy_mlp.h, as it stands)
 *   x_w = word w of the Philox4x32-10 block with counter (c, step, gid, GQ_OBS_NOISE_STREAM) and key (seed_lo, seed_hi) - seed, step0 and gid
 *   are the action noise's: the same seed gives the same rollout, two shards draw different noise, and the stream constant keeps the block
 *   apart from every other stream of the project (0x3b1f action noise, 0x9011 PD policy, 0xc0de / 0xd157 resampling, 0x5eed reset, 0x1a70.. IMU).
 *
 * Only what the network is fed is noised: the joint-impedance law, the reward window and both episode rules read the true row.
 */
#pragma once
#include "gq_policy_mlp.h"

#define GQ_OBS_NOISE_STREAM 0x0b5eu /* word 3 of the observation noise's Philox counter */

namespace gq {

enum { OBS_NOISE_UNIFORM = 0, OBS_NOISE_NORMAL = 1 };

/* what every word of a call shares */
struct NoiseLaw {
  const float* amp;        /* [in_obs] amplitudes in raw observation units, >= 0 */
  int32_t kind;            /* OBS_NOISE_* */
  float scan_amp;          /* one amplitude for every scan column, >= 0 */
  uint32_t seed_lo, seed_hi;
};

/* words 0 (low half) and 1 (high half) of the Philox4x32-10 block (Salmon et al. 2011) - the arithmetic of the step side's philox4x32, for
 * host and device.  (The routines below are inlined into their callers: a value that travels through memory would cost the policy kernels
 * scratch.) */
__host__ __device__ __forceinline__ uint64_t noise_philox01(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (uint64_t)c0 | ((uint64_t)c1 << 32);
}
/* n of column c */
__host__ __device__ __forceinline__ float obs_noise_unit(const NoiseLaw& Z, const int c, const uint32_t step, const uint32_t gid) {
#pragma clang fp contract(off)
  const uint64_t x = noise_philox01((uint32_t)c, step, gid, GQ_OBS_NOISE_STREAM, Z.seed_lo, Z.seed_hi);
  const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
  if (Z.kind == OBS_NOISE_NORMAL) return mlp_normal(x0, x1);
  const float u = (float)(x0 >> 8) * (1.0f / 16777216.0f);
  const float t = u + u;
  return t - 1.0f;
}
/* v with the noise of amplitude a on it: v itself, bit for bit, unless a > 0 */
__host__ __device__ __forceinline__ float obs_noise_add(const NoiseLaw& Z, const float a, const int c, const uint32_t step, const uint32_t gid, const float v) {
#pragma clang fp contract(off)
  if (!(a > 0.0f)) return v;
  const float d = a * obs_noise_unit(Z, c, step, gid);
  return v + d;
}
/* the amplitude of column c of an input row with in_obs observation columns and `cells` scan columns: 0 on every other column */
__host__ __device__ inline float obs_noise_amp(const NoiseLaw& Z, const int in_obs, const int cells, const int c) {
  if (c < in_obs) return Z.amp[c];
  return c < in_obs + cells ? Z.scan_amp : 0.0f;
}
}  // namespace gq
