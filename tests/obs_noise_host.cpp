/*
 * TEST INFRASTRUCTURE - the sensor noise on the in-loop policy's input row (gym_quadruped_amd/csrc/gq_policy_noise.h, gq_policy_dev.h) on the
 * host: a stand-alone program around policy_row_value<SCAN, HIST, LearnPlain, NOISE = true> with plain loads and stores, compiled with g++
 * against the headers with tests/simt_emu on the include path.
 *
 *   obs_noise_host IN OUT   consecutive policy steps of n envs, every column of the row staged exactly once per step; policy step s of env e
 *                           is keyed by (step0 + s D, gid[e]).
 *     IN   uint32 {n, in_obs, od, col_z, cells, feed_last, L, cols, steps, reverse, kind, seed_lo, seed_hi, step0, D}, uint32 gid[n], then f32:
 *          amp[in_obs], scan_amp, shift[in_obs], scale[in_obs], the scan law {offset, clip, scale}, the store before the first step
 *          [n][2][L][F] and its control words [n] (as floats; nothing with L = 0), then per step obs [n][od], last action [n][12], hit points
 *          [n][cells][3].  cells = 0: no scan; L = 0: no history.  The staging order is policy_row_host's (reverse: the opposite one).
 *     OUT  f32, per step: the words FED [n][Kp], the RECORDED row [n][in_dim], the CLEAN record [n][in_dim], the store [n][2][L][F], the control
 *          words [n] as floats
 *   obs_noise_host philox IN OUT   words 0, 1 of noise_philox01: IN uint32 {seed_lo, seed_hi, m}, then m counters of 4 words; OUT uint32 [m][2]
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gq_policy_dev.h"

static std::vector<char> read_all(const char* path) {
  std::vector<char> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(1); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes);
  if (!v.empty() && std::fread(v.data(), 1, v.size(), f) != v.size()) { std::fprintf(stderr, "short read of %s\n", path); std::exit(1); }
  std::fclose(f);
  return v;
}
static int write_all(const char* path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path, "wb");
  if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) { std::fprintf(stderr, "cannot write %s\n", path); return 1; }
  std::fclose(f);
  return 0;
}

struct Play {
  int n, od, col_z, kp, D;
  uint32_t step0;
  gq::RowLaw law;
  gq::NoiseLaw noise;
  std::vector<uint32_t> gid;
  std::vector<int> order;          /* the columns in staging order */
  std::vector<float> state;        /* [n][2][L][F] */
  std::vector<int32_t> ctl;        /* [n] */
};

template <bool SCAN, bool HIST>
static void step(Play& P, const int s, const float* obs, const float* last, const float* hits, std::vector<float>& res) {
  const gq::RowLaw& L = P.law;
  const size_t per = HIST ? gq::hist_env_floats(L.hist) : 0;
  std::vector<float> fed((size_t)P.n * P.kp, -1.0f), rec((size_t)P.n * L.in_dim, -1.0f), clean((size_t)P.n * L.in_dim, -1.0f);
  for (int e = P.n - 1; e >= 0; e--) {
    gq::RowSrc S{};
    S.obs = obs + (size_t)e * P.od;
    S.last = last + (size_t)e * 12;
    S.rec = rec.data() + (size_t)e * L.in_dim;
    if constexpr (SCAN) { S.z_base = S.obs[P.col_z]; S.hits = hits + (size_t)e * L.cells * 3; }
    if constexpr (HIST) { S.hist = P.state.data() + (size_t)e * per; S.hist_ctl = P.ctl[e]; }
    gq::RowNoise Z{};
    Z.law = P.noise; Z.step = P.step0 + (uint32_t)(s * P.D); Z.gid = P.gid[e];
    Z.clean_delta = clean.data() - rec.data();
    for (const int c : P.order) fed[(size_t)e * P.kp + c] = gq::policy_row_value<SCAN, HIST, gq::LearnPlain, true>(L, S, c, Z);
  }
  if constexpr (HIST)
    for (int e = 0; e < P.n; e++) gq::hist_push<gq::LearnPlain>(P.ctl.data(), e, P.ctl[e]);
  res.insert(res.end(), fed.begin(), fed.end());
  res.insert(res.end(), rec.begin(), rec.end());
  res.insert(res.end(), clean.begin(), clean.end());
  res.insert(res.end(), P.state.begin(), P.state.end());
  for (int e = 0; e < P.n && HIST; e++) res.push_back((float)P.ctl[e]);
}

static int philox_mode(const char* in_path, const char* out_path) {
  const std::vector<char> raw = read_all(in_path);
  uint32_t h[3];
  if (raw.size() < sizeof h) { std::fprintf(stderr, "no header\n"); return 1; }
  std::memcpy(h, raw.data(), sizeof h);
  if (raw.size() != sizeof h + (size_t)h[2] * 16) { std::fprintf(stderr, "size\n"); return 1; }
  std::vector<uint32_t> c((size_t)h[2] * 4), out((size_t)h[2] * 2);
  std::memcpy(c.data(), raw.data() + sizeof h, c.size() * 4);
  for (size_t i = 0; i < h[2]; i++) {
    const uint64_t x = gq::noise_philox01(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3], h[0], h[1]);
    out[2 * i] = (uint32_t)x; out[2 * i + 1] = (uint32_t)(x >> 32);
  }
  return write_all(out_path, out.data(), out.size() * 4);
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "philox")) return philox_mode(argv[2], argv[3]);
  if (argc != 3) { std::fprintf(stderr, "usage: obs_noise_host [philox] IN OUT\n"); return 1; }
  const std::vector<char> raw = read_all(argv[1]);
  uint32_t h[15];
  if (raw.size() < sizeof h) { std::fprintf(stderr, "no header\n"); return 1; }
  std::memcpy(h, raw.data(), sizeof h);
  const int n = (int)h[0], in_obs = (int)h[1], od = (int)h[2], col_z = (int)h[3], cells = (int)h[4], feed_last = (int)h[5], Lf = (int)h[6], cols = (int)h[7], steps = (int)h[8],
            reverse = (int)h[9], kind = (int)h[10], D = (int)h[14];
  if (n < 1 || n > 64 || in_obs < 1 || od < in_obs || od > 256 || col_z < 0 || col_z >= od || cells < 0 || cells > 64 || Lf < 0 || Lf > 8 || steps < 1 || D < 1 ||
      (kind != gq::OBS_NOISE_UNIFORM && kind != gq::OBS_NOISE_NORMAL) || (Lf > 0 && (cols < 1 || cols > in_obs))) { std::fprintf(stderr, "bad header\n"); return 1; }
  const int F = Lf > 0 ? cols + (feed_last ? 12 : 0) : 0, col0 = in_obs + cells + (feed_last ? 12 : 0);
  const int in_dim = gq::policy_row_dim(in_obs, cells, feed_last, Lf * F);
  if (in_dim > GQ_MLP_MAXW) { std::fprintf(stderr, "in_dim\n"); return 1; }
  const size_t store = (size_t)n * 2 * Lf * F;
  const size_t per_step = (size_t)n * (od + 12 + (size_t)cells * 3);
  const size_t want = (size_t)n + 3 * (size_t)in_obs + 1 + 3 + store + (Lf > 0 ? n : 0) + steps * per_step;
  if (raw.size() != sizeof h + want * sizeof(float)) { std::fprintf(stderr, "size\n"); return 1; }
  std::vector<float> in(want);
  std::memcpy(in.data(), raw.data() + sizeof h, want * sizeof(float));
  const float* at = in.data();
  Play P{};
  P.n = n; P.od = od; P.col_z = col_z; P.kp = gq::mlp_kp(in_dim); P.D = D; P.step0 = h[13];
  P.gid.resize(n);
  std::memcpy(P.gid.data(), at, (size_t)n * 4); at += n;
  P.noise.amp = at; at += in_obs;
  P.noise.scan_amp = at[0]; at += 1;
  P.noise.kind = kind; P.noise.seed_lo = h[11]; P.noise.seed_hi = h[12];
  P.law.in_obs = in_obs; P.law.in_dim = in_dim; P.law.cells = cells;
  P.law.shift = at; P.law.scale = at + in_obs; at += 2 * in_obs;
  P.law.scan = gq::ScanLaw{at[0], at[1], at[2]}; at += 3;
  if (Lf > 0) {
    P.law.hist = gq::hist_law(Lf, cols, feed_last, col0);
    P.state.assign(at, at + store); at += store;
    for (int e = 0; e < n; e++) P.ctl.push_back((int32_t)at[e]);
    at += n;
  }
  for (int g = 0; g < 4; g++)
    for (int c = g; c < P.kp; c += 4) P.order.push_back(c);
  if (reverse) std::reverse(P.order.begin(), P.order.end());
  std::vector<float> res;
  for (int s = 0; s < steps; s++, at += per_step) {
    const float* obs = at;
    const float* last = obs + (size_t)n * od;
    const float* hits = last + (size_t)n * 12;
    if (cells > 0 && Lf > 0) step<true, true>(P, s, obs, last, hits, res);
    else if (cells > 0) step<true, false>(P, s, obs, last, hits, res);
    else if (Lf > 0) step<false, true>(P, s, obs, last, hits, res);
    else step<false, false>(P, s, obs, last, hits, res);
  }
  return write_all(argv[2], res.data(), res.size() * sizeof(float));
}
