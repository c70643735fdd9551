/*
 * TEST INFRASTRUCTURE - the MLP policy's law (gym_quadruped_amd/csrc/gq_policy_mlp.h) on the host: a stand-alone program around
 * mlp_row_forward, the definition of the network, compiled with g++ against the header with tests/simt_emu on the include path.
 *
 *   policy_mlp_host forward IN OUT   IN: int32 {n_layers, in_dim, act, out_act, width[4], n_rows}, the packed blob, rows [n_rows][in_dim] f32
 *                                    OUT: per row, the outputs of every layer in turn (Np floats each, activation applied)
 *                                    (the last layer's first 12 are also compared with mlp_row_forward's result: exit 2 on a difference)
 *   policy_mlp_host act WHICH IN OUT IN: f32 arguments; OUT: mlp_activate(WHICH, x) of each
 *   policy_mlp_host normal IN OUT    IN: uint32 pairs (words 0, 1 of a Philox block); OUT: mlp_normal of each as f32
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gq_policy_mlp.h"

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
  if (raw.size() < 9) { std::fprintf(stderr, "no header\n"); return 1; }
  int32_t h[9];
  std::memcpy(h, raw.data(), sizeof h);
  gq::MlpNet net{};
  net.n_layers = h[0]; net.in_dim = h[1]; net.act = h[2]; net.out_act = h[3];
  for (int l = 0; l < GQ_MLP_MAXL; l++) net.width[l] = h[4 + l];
  const int n_rows = h[8];
  if (net.n_layers < 1 || net.n_layers > GQ_MLP_MAXL || net.in_dim < 1 || net.in_dim > GQ_MLP_MAXW || n_rows < 0) { std::fprintf(stderr, "bad header\n"); return 1; }
  for (int l = 0; l < net.n_layers; l++)
    if (net.width[l] < 1 || net.width[l] > GQ_MLP_MAXW) { std::fprintf(stderr, "bad width\n"); return 1; }
  const size_t nb = gq::mlp_blob_floats(net);
  if (raw.size() != 9 + nb + (size_t)n_rows * net.in_dim) { std::fprintf(stderr, "size: %zu floats, expected %zu\n", raw.size(), 9 + nb + (size_t)n_rows * net.in_dim); return 1; }
  const float* blob = raw.data() + 9;
  const float* rows = blob + nb;
  std::vector<float> res;
  const int n_out = net.width[net.n_layers - 1];
  for (int r = 0; r < n_rows; r++) {
    float buf[2][GQ_MLP_MAXW];
    const int kp0 = gq::mlp_kp(net.in_dim);
    for (int c = 0; c < kp0; c++) buf[0][c] = c < net.in_dim ? rows[(size_t)r * net.in_dim + c] : 0.0f;
    const float* w = blob;
    int cur = 0;
    for (int l = 0; l < net.n_layers; l++) {
      gq::mlp_row_layer(net, l, w, buf[cur], buf[cur ^ 1]);
      w += gq::mlp_layer_floats(net, l);
      cur ^= 1;
      res.insert(res.end(), buf[cur], buf[cur] + gq::mlp_np(net.width[l]));
    }
    float y[GQ_MLP_MAXW];
    gq::mlp_row_forward(net, blob, rows + (size_t)r * net.in_dim, y);
    if (std::memcmp(y, buf[cur], sizeof(float) * n_out) != 0) { std::fprintf(stderr, "row %d: mlp_row_forward differs from its layers\n", r); return 2; }
  }
  write_all(out, res);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "forward")) return forward(argv[2], argv[3]);
  if (argc == 5 && !std::strcmp(argv[1], "act")) {
    const int which = std::atoi(argv[2]);
    std::vector<float> x = read_all<float>(argv[3]);
    for (float& v : x) v = gq::mlp_activate(which, v);
    write_all(argv[4], x);
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "normal")) {
    const std::vector<uint32_t> w = read_all<uint32_t>(argv[2]);
    std::vector<float> z(w.size() / 2);
    for (size_t i = 0; i < z.size(); i++) z[i] = gq::mlp_normal(w[2 * i], w[2 * i + 1]);
    write_all(argv[3], z);
    return 0;
  }
  std::fprintf(stderr, "usage: policy_mlp_host forward IN OUT | act WHICH IN OUT | normal IN OUT\n");
  return 1;
}
