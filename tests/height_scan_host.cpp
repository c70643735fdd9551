/*
 * TEST INFRASTRUCTURE - the height scan's law (gym_quadruped_amd/csrc/gq_policy_scan.h) on the host: a stand-alone program around
 * height_scan_cell, compiled with g++ against the header with tests/simt_emu on the include path.
 *
 *   height_scan_host IN OUT   IN: f32 records {z_base, z_hit, offset, clip, scale}; OUT: the scan word of each as f32
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gq_policy_scan.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: height_scan_host IN OUT\n"); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes < 0 || bytes % (5 * sizeof(float)) != 0) { std::fprintf(stderr, "%s: %ld bytes are no whole number of records\n", argv[1], bytes); return 1; }
  std::vector<float> in((size_t)bytes / sizeof(float));
  if (!in.empty() && std::fread(in.data(), sizeof(float), in.size(), f) != in.size()) { std::fprintf(stderr, "short read of %s\n", argv[1]); return 1; }
  std::fclose(f);
  std::vector<float> out(in.size() / 5);
  for (size_t i = 0; i < out.size(); i++) {
    const float* r = in.data() + 5 * i;
    const gq::ScanLaw law{r[2], r[3], r[4]};
    out[i] = gq::height_scan_cell(law, r[0], r[1]);
  }
  f = std::fopen(argv[2], "wb");
  if (!f || (!out.empty() && std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size())) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
  std::fclose(f);
  return 0;
}
