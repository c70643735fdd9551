/*
 * TEST INFRASTRUCTURE - the observation history's store and episode rule (gym_quadruped_amd/csrc/gq_policy_hist.h) on the host: a stand-alone
 * program around hist_episode_rule, hist_stage_frame, hist_stage_current and hist_push with plain loads and stores, compiled with g++ against
 * the header with tests/simt_emu on the include path.
 *
 *   policy_hist_host play IN OUT   the policy seat's visits played over consecutive calls.  IN: int32 {n_env, L, F, D, K, n_calls, closing},
 *                                  then per call int32 pending[n_env] (the flag before the call) and terminated[K][n_env] (the byte after
 *                                  each step).  The store starts in buffer 1 with frame i, word w of env e = -(4096 (i + 1) + 64 e + w + 1)
 *                                  and 777 in every word of buffer 0; the current block of global policy step g (over all calls) holds
 *                                  4096 (g + 1) + 64 e + w + 1 - every word names its env, its step and its place.  The words of a visit
 *                                  are staged in the order the tile's lanes take them (column c by lane group c % 4), frames before or
 *                                  after the current block by the column's parity - any order must do.  closing: the learning modes'
 *                                  visit k = K is played too.
 *                                  OUT (f32): per call and policy step the words FED [K / D][n_env][F + L F] (current block, frame_1 ..
 *                                  frame_L), then the store after the call: [n_env][2][L][F], then the control words [n_env] as floats
 *   policy_hist_host div IN OUT    OUT: one float, the number of (F, hc) in 1 .. 256 x 0 .. 255 where (hc * inv) >> 16 != hc / F
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gq_policy_hist.h"

template <class T>
static std::vector<T> read_all(const char* path) {
  std::vector<T> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(1); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fprintf(stderr, "short read of %s\n", path); std::exit(1); }
  std::fclose(f);
  return v;
}
static void write_all(const char* path, const std::vector<float>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f || (!v.empty() && std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size())) { std::fprintf(stderr, "cannot write %s\n", path); std::exit(1); }
  std::fclose(f);
}

static int play(const char* in, const char* out) {
  const std::vector<int32_t> raw = read_all<int32_t>(in);
  if (raw.size() < 7) { std::fprintf(stderr, "no header\n"); return 1; }
  const int n = raw[0], L = raw[1], F = raw[2], D = raw[3], K = raw[4], calls = raw[5], closing = raw[6];
  if (n < 1 || n > 64 || L < 1 || F < 1 || F > 64 || L * F > 255 || D < 1 || K < D || K % D || calls < 1) { std::fprintf(stderr, "bad header\n"); return 1; }
  if (raw.size() != 7 + (size_t)calls * (size_t)(K + 1) * n) { std::fprintf(stderr, "size\n"); return 1; }
  const gq::HistLaw H = gq::hist_law(L, F, 0, F); /* the row played here: the current block's F words, then the frames */
  const size_t per = gq::hist_env_floats(H);
  std::vector<float> state((size_t)n * per, 777.0f), res;
  std::vector<int32_t> ctl(n, gq::HIST_PARITY | gq::HIST_VALID), cw(n);
  for (int e = 0; e < n; e++)
    for (int i = 0; i < L; i++)
      for (int w = 0; w < F; w++) state[e * per + gq::hist_at(H, 1, i, w)] = -(float)(4096 * (i + 1) + 64 * e + w + 1);
  std::vector<uint8_t> pending(n), terminated(n);
  const int32_t* at = raw.data() + 7;
  const int width = F + L * F;
  for (int c = 0; c < calls; c++) {
    for (int e = 0; e < n; e++) pending[e] = (uint8_t)(at[e] != 0);
    const int32_t* term = at + n; /* [K][n] */
    for (int k = 0; k < K + (closing ? 1 : 0); k++) {
      if (k >= 1)
        for (int e = 0; e < n; e++) terminated[e] = (uint8_t)(term[(size_t)(k - 1) * n + e] != 0);
      for (int e = 0; e < n; e++) cw[e] = gq::hist_episode_rule<gq::LearnPlain>(terminated.data(), pending.data(), ctl.data(), e, k);
      if (k % D != 0 || k >= K) continue;
      const int g = c * (K / D) + k / D;
      std::vector<float> fed((size_t)n * width, 0.0f);
      for (int grp = 0; grp < 4; grp++)
        for (int e = n - 1; e >= 0; e--)
          for (int col = grp; col < width; col += 4) {
            float* const env = state.data() + e * per;
            float v;
            if (col < F) {
              v = (float)(4096 * (g + 1) + 64 * e + col + 1);
              gq::hist_stage_current<gq::LearnPlain>(H, env, cw[e], col, v);
            } else {
              int w = -1;
              v = gq::hist_stage_frame<gq::LearnPlain>(H, env, cw[e], col - H.col0, &w);
              if (w != (col - F) % F) { std::fprintf(stderr, "word_of_frame\n"); return 1; }
            }
            fed[(size_t)e * width + col] = v;
          }
      for (int e = 0; e < n; e++) gq::hist_push<gq::LearnPlain>(ctl.data(), e, cw[e]);
      res.insert(res.end(), fed.begin(), fed.end());
    }
    res.insert(res.end(), state.begin(), state.end());
    for (int e = 0; e < n; e++) res.push_back((float)ctl[e]);
    at += (size_t)(K + 1) * n;
  }
  write_all(out, res);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "play")) return play(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "div")) {
    int bad = 0;
    for (int F = 1; F <= 256; F++) {
      const gq::HistLaw H = gq::hist_law(1, F, 0, 0);
      for (int hc = 0; hc < 256; hc++) bad += ((hc * H.inv) >> 16) != hc / F;
    }
    write_all(argv[3], {(float)bad});
    return 0;
  }
  std::fprintf(stderr, "usage: policy_hist_host play IN OUT | div IN OUT\n");
  return 1;
}
