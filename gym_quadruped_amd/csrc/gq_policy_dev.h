/*
 * gq_policy_dev.h - what the in-loop policy (policy_mlp_kernel, every MODE) is handed and what it is fed: THE INPUT ROW, defined once for
 * host and device, and the ONE device block of a call.  The features keep their laws in their own headers - gq_policy_mlp.h (the network),
 * gq_policy_gru.h (the cell, the hidden state's episode rule), gq_policy_scan.h (the scan law), gq_policy_hist.h (the store, its episode
 * rule) - which know nothing of each other; this header puts them side by side.  Plain C++: compiles with the product's gq_device.h and with
 * the host shim (tests/simt_emu); tests/policy_row_host.cpp plays policy_row_value with LearnPlain.
 *
 * THE INPUT ROW of env e at a policy step, in_dim = in_obs + cells + 12 f + L F <= 256 columns (policy_row_dim):
 *
 *   x = [ obs_row[0 : in_obs] | scan[0 : cells] | last action (12) | frame_1 | ... | frame_L ]
 *         always                SCAN              f = feed_last      HIST, F = cols + 12 f words each, newest first
 *
 *   obs       column c of the env's observation row, FED as (o - shift[c]) * scale[c] (mlp_obs_in: each operation rounded, absent tables are
 *             the identity), RECORDED raw.  With HIST the raw word of c < cols also becomes word c of the current frame.
 *   scan      cell i of the batch's base-following map through the scan law (height_scan_cell) on word 2 of the cell's hit point and
 *             z_base, the z column of the SAME observation row (it may lie beyond in_obs).  No shift / scale; recorded as fed.
 *   last      the env's previous policy action, raw: no shift / scale, recorded as fed.  With HIST it is the tail of the current frame,
 *             words cols .. cols + 11.
 *   frame_i   the current frame of the policy step i steps back, out of the env's store (gq_policy_hist.h: zero without VALID), each word
 *             moved one slot on in the env's other buffer as it is staged.  RECORDED raw; FED with shift / scale by its ORIGINAL column
 *             w < cols, its action words as they are - frame_i at step s carries what the current block carried at step s - i.
 *   c >= in_dim: 0 (the zero padding of the first layer's inputs).
 *
 * "Recorded" is the learning modes' policy_obs row, where there is one.  Every column is staged exactly once per fresh visit, in any order:
 * a column's value and side effects depend on no other column of the visit (the store is read in one buffer and written in the other).
 *
 * SENSOR NOISE (NOISE, gq_policy_noise.h: the law): the observation and scan columns with a positive amplitude are FED with noise on the raw
 * word, before shift / scale.  The noisy word is what is recorded, what becomes the word of the history's current frame and what goes on to
 * shift / scale; the true word of every column goes to the second record (RowNoise::clean_delta).  z_base stays the true z.  Last-action and frame words
 * are never noised (a frame word was noised when it was the current block's), so both records hold the same word there.
 */
#pragma once
#include "gq_policy_mlp.h"
#include "gq_policy_gru.h"
#include "gq_policy_scan.h"
#include "gq_policy_hist.h"
#include "gq_policy_noise.h"

namespace gq {

/* ---- the input row ---- */
__host__ __device__ inline int policy_row_dim(const int in_obs, const int cells, const int feed_last, const int hist_words) {
  return in_obs + cells + (feed_last ? 12 : 0) + hist_words;
}
/* what every row of a call shares.  The last action needs no field: its columns are the ones between the scan and hist.col0 (HIST) or
 * in_dim - twelve with feed_last, none without (policy_row_dim).  cells / scan are read with SCAN alone, hist with HIST alone. */
struct RowLaw {
  int in_obs, in_dim, cells;
  const float* shift; const float* scale; /* [in_obs] or NULL */
  ScanLaw scan;
  HistLaw hist;
};
/* one row's sources */
struct RowSrc {
  const float* obs;    /* the env's observation row */
  const float* last;   /* [12] its previous policy action */
  const float* hits;   /* SCAN: [cells][3] its hit points */
  float z_base;        /* SCAN: the z column of obs */
  float* hist;         /* HIST: its store, and the control word its visit stages with (hist_episode_rule) */
  int hist_ctl;
  float* rec;          /* [in_dim] where the row is recorded, or NULL */
};
/* NOISE: the call's law and one row's key and second record */
struct RowNoise {
  NoiseLaw law;
  uint32_t step, gid;  /* the row's Philox key: the absolute step counter step0 + k, the global env id */
  ptrdiff_t clean_delta; /* the second record relative to RowSrc::rec, in words: the TRUE word of column c goes to rec[c + clean_delta]; 0: none.
                          * The two records are arrays of one shape, so the distance is the call's, not the row's: no second pointer per lane */
};
/* column c of the row (head comment): the value fed; records the raw word and stages the history's store on the way.  Mem: LearnPlain on
 * the host, LearnPub in the rollout (every word is another wavefront's store of this launch, or one of an earlier visit).  NOISE false: Z is
 * not looked at, and the routine is what it was without the parameter. */
template <bool SCAN, bool HIST, class Mem, bool NOISE = false>
__host__ __device__ __forceinline__ float policy_row_value(const RowLaw& L, const RowSrc& S, const int c, const RowNoise& Z = RowNoise{}) {
  if (c >= L.in_dim) return 0.0f;
  const int in_obs = L.in_obs, cells = SCAN ? L.cells : 0;
  const auto word = [&](const float* const p) { /* a raw word, recorded as loaded */
    const float o = Mem::ld(p);
    if (S.rec) S.rec[c] = o;
    if constexpr (NOISE) {
      if (S.rec && Z.clean_delta) S.rec[c + Z.clean_delta] = o;
    }
    return o;
  };
  [[maybe_unused]] const auto noisy = [&](const float v, const float a) { /* NOISE: the word as fed, both records */
    const float vn = obs_noise_add(Z.law, a, c, Z.step, Z.gid, v);
    if (S.rec) S.rec[c] = vn;
    if (S.rec && Z.clean_delta) S.rec[c + Z.clean_delta] = v;
    return vn;
  };
  if constexpr (HIST) {
    const HistLaw& H = L.hist;
    if (c >= H.col0) { /* a word of frame_1 .. frame_L */
      int w;
      const float o = hist_stage_frame<Mem>(H, S.hist, S.hist_ctl, c - H.col0, &w);
      if (S.rec) S.rec[c] = o;
      if constexpr (NOISE) {
        if (S.rec && Z.clean_delta) S.rec[c + Z.clean_delta] = o;
      }
      return w < H.cols ? mlp_obs_in(o, L.shift, L.scale, w) : o;
    }
    if (c < in_obs) {
      float o;
      if constexpr (NOISE) o = noisy(Mem::ld(S.obs + c), Z.law.amp[c]);
      else o = word(S.obs + c);
      if (c < H.cols) hist_stage_current<Mem>(H, S.hist, S.hist_ctl, c, o);
      return mlp_obs_in(o, L.shift, L.scale, c);
    }
    if (c >= in_obs + cells) { /* the last action: the tail of the current frame */
      const float o = word(S.last + (c - in_obs - cells));
      hist_stage_current<Mem>(H, S.hist, S.hist_ctl, H.cols + (c - in_obs - cells), o);
      return o;
    }
  } else {
    if constexpr (NOISE) {
      if (c < in_obs) return mlp_obs_in(noisy(Mem::ld(S.obs + c), Z.law.amp[c]), L.shift, L.scale, c);
    } else {
      if (c < in_obs) return mlp_obs_in(word(S.obs + c), L.shift, L.scale, c);
    }
  }
  if constexpr (SCAN) { /* (with HIST only the scan's own columns come this far) */
    const int cell = c - in_obs;
    if constexpr (!HIST) {
      if (cell >= cells) return word(S.last + (cell - cells)); /* the last action, behind the scan */
    }
    const float s = height_scan_cell(L.scan, S.z_base, Mem::ld(S.hits + 3 * cell + 2));
    if constexpr (NOISE) return noisy(s, Z.law.scan_amp);
    if (S.rec) S.rec[c] = s;
    return s;
  }
  return word(S.last + (c - in_obs));
}

/* ---- the device block: what a call of gq_rollout_policy* hands to policy_mlp_kernel, and gq_policy_*_eval to its kernels (device
 * pointers), next to the MailboxDev the seat shares with the step side.  A call fills the parts its MODE reads and zeroes the others. ---- */
/* MODE & 4, the recurrent policy: seat.net is then the HEAD (in_dim = hidden) and seat.blob the head's layers, while seat.in_obs / feed_last /
 * shift / scale describe the cell's input row */
struct GruDev {
  GruNet cell;
  const float* blob;            /* the six gate layers */
  float* hidden_state;          /* [N][H] in / out (gq_policy_gru_eval: h_in [n][H]) */
  float* hidden_seq;            /* [n_steps / decimation][N][H] the state FED at each policy step, after the rule, or NULL (eval: h_out [n][H]) */
};
/* the episode flags are the SEAT's: both episode rules read them, the hidden state's (gru_episode_rule) and the history's
 * (hist_episode_rule).  They are carried here and not in the learn block, because the plain mode has none. */
struct EpisodeDev {
  const uint8_t* terminated;    /* [N] the batch's flag, as LearnDev's */
  const uint8_t* pending;       /* [N] or NULL */
};
/* MODE & 8, the height scan */
struct ScanDev {
  ScanLaw law;
  int32_t cells;                /* rows * cols of the batch's base-following map */
  int32_t col_z;                /* column of the base's z in the observation row (may lie beyond in_obs) */
  int32_t pad_[3];
  const float* hits;            /* [N][cells][3], the map's tensor */
};
/* MODE & 16, the observation history */
struct HistDev {
  HistLaw law;
  float* state;                 /* [N][2][L][F] the store */
  int32_t* ctl;                 /* [N] the control words */
};
/* MODE & 32, the sensor noise (gq_policy_noise.h): its seed, step0 and env id offset are the seat's, the action noise's.  The table is
 * immutable during the launch: ordinary loads */
struct NoiseDev {
  const float* amp;             /* [seat.in_obs] */
  int32_t kind;                 /* OBS_NOISE_* */
  float scan_amp;
  float* rec_clean;             /* [n_steps / decimation][N][in_dim] the row with the true words, or NULL (only next to the learn block's policy_obs) */
};
struct PolicyDev {
  PolicyMlpDev seat;
  GruDev gru;
  EpisodeDev episode;
  ScanDev scan;
  HistDev hist;
  NoiseDev noise;               /* appended: the parts before it stay where the existing kernels were built to find them */
};
/* the layout is pinned: these are the size and the offsets the kernels were built and profiled with when the parts were nested structs
 * (the block's address is all a kernel has) - a part that moves changes the addressing of every instantiation */
static_assert(sizeof(PolicyDev) == 632, "PolicyDev");
static_assert(offsetof(PolicyDev, gru.cell) == 472 && offsetof(PolicyDev, episode.terminated) == 504 && offsetof(PolicyDev, scan.law) == 520 && offsetof(PolicyDev, scan.hits) == 552 &&
              offsetof(PolicyDev, hist.law) == 560 && offsetof(PolicyDev, hist.ctl) == 600 && offsetof(PolicyDev, noise.amp) == 608, "PolicyDev");
}  // namespace gq
