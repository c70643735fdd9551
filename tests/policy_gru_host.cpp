/*
 * TEST INFRASTRUCTURE - the recurrent policy's law and episode rule (gym_quadruped_amd/csrc/gq_policy_gru.h) on the host: a stand-alone
 * program around gru_row_forward, the definition, and gru_episode_rule, compiled with g++ against the header with tests/simt_emu on the
 * include path.
 *
 *   policy_gru_host forward IN OUT   IN: int32 {in_dim, hidden, head layers, act, out_act, width[4], n_rows}, the packed blob, rows
 *                                    [n_rows][in_dim] f32, states [n_rows][hidden] f32
 *                                    OUT: per row the 12 actions, then h' with its padding (Hp floats)
 *   policy_gru_host sig IN OUT       IN: f32 arguments; OUT: gru_sig of each
 *   policy_gru_host rule IN OUT      the episode rule played over consecutive calls.  IN: int32 {n_env, H, D, K, n_calls, closing},
 *                                    then per call int32 pending[n_env] (the flag before the call) and terminated[K][n_env] (the byte
 *                                    after each step).  The hidden rows start at 1; at every policy step the "cell" leaves 2 + the step's
 *                                    index in every column (never zero).  closing: the learning modes' visit k = K is played too.
 *                                    OUT (f32): per call and policy step the rows as FED [K / D][n_env][H], then the rows after the call
 *                                    [n_env][H]
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gq_policy_gru.h"

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

static int forward(const char* in, const char* out) {
  const std::vector<float> raw = read_all<float>(in);
  constexpr int NH = 10;
  if (raw.size() < NH) { std::fprintf(stderr, "no header\n"); return 1; }
  int32_t h[NH];
  std::memcpy(h, raw.data(), sizeof h);
  gq::GruNet G{h[0], h[1]};
  gq::MlpNet head{};
  head.n_layers = h[2]; head.in_dim = G.hidden; head.act = h[3]; head.out_act = h[4];
  for (int l = 0; l < GQ_MLP_MAXL; l++) head.width[l] = h[5 + l];
  const int n_rows = h[9];
  if (G.in_dim < 1 || G.in_dim > GQ_MLP_MAXW || G.hidden < 1 || G.hidden > GQ_GRU_MAXH || head.n_layers < 1 || head.n_layers > GQ_GRU_HEAD_MAXL || n_rows < 0) {
    std::fprintf(stderr, "bad header\n"); return 1;
  }
  for (int l = 0; l < head.n_layers; l++)
    if (head.width[l] < 1 || head.width[l] > GQ_MLP_MAXW) { std::fprintf(stderr, "bad width\n"); return 1; }
  if (head.width[head.n_layers - 1] != 12) { std::fprintf(stderr, "the head must have 12 outputs\n"); return 1; }
  const size_t nb = gq::gru_blob_floats(G, head), want = NH + nb + (size_t)n_rows * (G.in_dim + G.hidden);
  if (raw.size() != want) { std::fprintf(stderr, "size: %zu floats, expected %zu\n", raw.size(), want); return 1; }
  const float* blob = raw.data() + NH;
  const float* rows = blob + nb;
  const float* states = rows + (size_t)n_rows * G.in_dim;
  const int hp = gq::mlp_np(G.hidden);
  std::vector<float> res;
  for (int r = 0; r < n_rows; r++) {
    float a[GQ_MLP_MAXW], hn[GQ_GRU_MAXH];
    gq::gru_row_forward(G, head, blob, rows + (size_t)r * G.in_dim, states + (size_t)r * G.hidden, a, hn);
    res.insert(res.end(), a, a + 12);
    res.insert(res.end(), hn, hn + hp);
  }
  write_all(out, res);
  return 0;
}

static int rule(const char* in, const char* out) {
  const std::vector<int32_t> raw = read_all<int32_t>(in);
  if (raw.size() < 6) { std::fprintf(stderr, "no header\n"); return 1; }
  const int n = raw[0], H = raw[1], D = raw[2], K = raw[3], calls = raw[4], closing = raw[5];
  if (n < 1 || H < 1 || H > GQ_GRU_MAXH || D < 1 || K < D || K % D || calls < 1) { std::fprintf(stderr, "bad header\n"); return 1; }
  if (raw.size() != 6 + (size_t)calls * (size_t)(K + 1) * n) { std::fprintf(stderr, "size\n"); return 1; }
  std::vector<float> hs((size_t)n * H, 1.0f), res;
  std::vector<uint8_t> pending(n), terminated(n);
  const int32_t* at = raw.data() + 6;
  for (int c = 0; c < calls; c++) {
    for (int e = 0; e < n; e++) pending[e] = (uint8_t)(at[e] != 0);
    const int32_t* term = at + n; /* [K][n] */
    for (int k = 0; k < K + (closing ? 1 : 0); k++) {
      if (k >= 1)
        for (int e = 0; e < n; e++) terminated[e] = (uint8_t)(term[(size_t)(k - 1) * n + e] != 0);
      for (int e = 0; e < n; e++) gq::gru_episode_rule<gq::LearnPlain>(terminated.data(), pending.data(), hs.data(), H, e, k);
      if (k % D == 0 && k < K) { /* a policy step: the rows as fed, then the cell */
        res.insert(res.end(), hs.begin(), hs.end());
        for (float& v : hs) v = 2.0f + (float)(c * (K / D) + k / D);
      }
    }
    res.insert(res.end(), hs.begin(), hs.end());
    at += (size_t)(K + 1) * n;
  }
  write_all(out, res);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "forward")) return forward(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "rule")) return rule(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "sig")) {
    std::vector<float> x = read_all<float>(argv[2]);
    for (float& v : x) v = gq::gru_sig(v);
    write_all(argv[3], x);
    return 0;
  }
  std::fprintf(stderr, "usage: policy_gru_host forward IN OUT | sig IN OUT | rule IN OUT\n");
  return 1;
}
