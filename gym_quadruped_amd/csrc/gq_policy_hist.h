/*
 * gq_policy_hist.h - the OBSERVATION HISTORY of the closed-loop rollout's MLP policy (gq_rollout_policy_hist): the frames of the last L
 * policy steps as further columns of the input row, the per-env store that holds them across steps, windows and calls and THE EPISODE RULE of
 * that store (the device block of a call: gq_policy_dev.h).  Plain C++: compiles with the product's gq_device.h and with the host shim
 * (tests/simt_emu).
 *
 * THE LAW.  A FRAME is what the network was fed as its current block at one policy step, raw: the first `cols` observation words as loaded
 * (before shift / scale), then - with feed_last_action - the 12 fed-back action words of that step; F = cols + 12 f words.  The frames are
 * the last columns of the input row, frame_1 .. frame_L from column col0 on (gq_policy_dev.h holds the row's one definition); frame_i is the
 * frame of the policy step i steps back, newest first.  When a frame is staged,
 * shift / scale act on its observation words by their original column c < cols and not on its action words, so frame_i at step s carries
 * exactly the values the current block carried at step s - i.  policy_obs records the history words raw, as every other word.
 *
 * THE STORE, per env: two buffers of L frames, [2][L][F] floats, and one CONTROL WORD: bit 0 the parity p of the buffer that holds what is
 * fed next (slot i - 1 = frame_i), bit 1 VALID - clear: every frame is zero, whatever the buffer holds.  A fresh visit reads buffer p and
 * writes buffer 1 - p: frame_i to slot i (the oldest is not written: it drops out) and the current block to slot 0; the env's own lane then
 * stores the control word (1 - p) | VALID.  Every word of the tile is staged by exactly one lane (mlp_tile_stage), and no lane writes the
 * buffer another lane still reads: the hazard is absent by construction, at the price of one store per staged history word.
 *
 * THE EPISODE RULE (hist_episode_rule; the GRU's, gru_episode_rule, on the same flags).  At the visit of env e for step k - the observation
 * after step k - 1 is out - BEFORE anything of that visit is staged:
 *   k == 0   the env waits for its re-spawn (pending[e]):            VALID := 0
 *   k >= 1   the `terminated` byte after step k - 1 is set:          VALID := 0
 * one control word, not L F stores.  The learning modes' closing visit k = K applies it; the plain mode has none, and a fall in step K - 1
 * is caught by the next call's k == 0.  A frame of a store without VALID is staged as zero from the control word, not from memory.  At every
 * fresh visit, after staging, the current frame is pushed - also in a visit where the rule fired.  Consequence: the history fed at policy
 * step s + 1 is all zero exactly where window s contained a termination (dones[s]); across a call boundary, where the env was pending.  The
 * fed-back last action keeps its own semantics: zeros at the first policy step of a call, kept across a re-spawn.
 */
#pragma once
#include <gq_device.h> /* angle brackets: the include path decides (csrc/ for the product, tests/simt_emu/ for the host programs) */
#include <cstddef>
#include <cstdint>
#include "gq_learn.h" /* LearnPlain / LearnPub: the memory access of the store and its episode rule */

namespace gq {

enum { HIST_PARITY = 1, HIST_VALID = 2 };

struct HistLaw {
  int32_t frames;  /* L >= 1 */
  int32_t cols;    /* leading observation words of a frame, 1 .. in_obs */
  int32_t width;   /* F = cols + 12 feed_last */
  int32_t col0;    /* the first history column of the input row: in_obs + cells + 12 feed_last */
  int32_t inv;     /* ceil(2^16 / F): hc / F == (hc * inv) >> 16 for 0 <= hc < 256, 1 <= F <= 256 (hist_law) */
  int32_t pad_[3];
};

__host__ __device__ inline HistLaw hist_law(const int frames, const int cols, const int feed_last, const int col0) {
  HistLaw H{};
  H.frames = frames; H.cols = cols; H.width = cols + (feed_last ? 12 : 0); H.col0 = col0;
  /* m = ceil(2^16 / F) overshoots 2^16 / F by e / F with e = m F - 2^16 < F <= 256; hc e < 2^16 for hc < 256, so the floor is that of hc / F */
  H.inv = (65536 + H.width - 1) / H.width;
  return H;
}
__host__ __device__ inline size_t hist_env_floats(const HistLaw& H) { return 2 * (size_t)H.frames * (size_t)H.width; }
__host__ __device__ inline int hist_words(const HistLaw& H) { return H.frames * H.width; }
/* word w of slot i in the buffer of parity p, relative to the env's store */
__host__ __device__ inline int hist_at(const HistLaw& H, const int p, const int i, const int w) { return (p * H.frames + i) * H.width + w; }

/* THE EPISODE RULE (head comment): the visit of env e for step k, by the env's own lane.  Returns the control word the visit stages with.
 * Mem: LearnPlain on the host, LearnPub in the rollout (the flags are the step side's stores of this launch). */
template <class Mem>
__host__ __device__ inline int hist_episode_rule(const uint8_t* terminated, const uint8_t* pending, int32_t* ctl, const int e, const int k) {
  int c = Mem::ld(ctl + e);
  const bool reset = k == 0 ? (pending != nullptr && Mem::ld_u8(pending + e) != 0) : Mem::ld_u8(terminated + e) != 0;
  if (reset && (c & HIST_VALID)) {
    c &= ~HIST_VALID;
    Mem::st(ctl + e, c);
  }
  return c;
}
/* STAGE history word hc (0 .. L F - 1: word hc % F of frame_(hc / F + 1)) of the env whose store is `env` and whose control word is c: the
 * raw word, moved one slot on in the other buffer.  Whoever stages the word calls this once. */
template <class Mem>
__host__ __device__ inline float hist_stage_frame(const HistLaw& H, float* env, const int c, const int hc, int* word_of_frame) {
  const int i = (hc * H.inv) >> 16, w = hc - i * H.width, p = c & HIST_PARITY;
  const float v = (c & HIST_VALID) ? Mem::ld(env + hist_at(H, p, i, w)) : 0.0f;
  if (i + 1 < H.frames) Mem::st(env + hist_at(H, p ^ 1, i + 1, w), v);
  *word_of_frame = w;
  return v;
}
/* STAGE word w (0 .. F - 1) of the current block, raw value v: it becomes the newest frame of the other buffer */
template <class Mem>
__host__ __device__ inline void hist_stage_current(const HistLaw& H, float* env, const int c, const int w, const float v) {
  Mem::st(env + hist_at(H, (c & HIST_PARITY) ^ 1, 0, w), v);
}
/* PUSH: after the stage, by the env's own lane - the other buffer is what is fed next, and it is valid */
template <class Mem>
__host__ __device__ inline void hist_push(int32_t* ctl, const int e, const int c) {
  Mem::st(ctl + e, ((c & HIST_PARITY) ^ 1) | HIST_VALID);
}
}  // namespace gq
