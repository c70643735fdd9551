/* TEST INFRASTRUCTURE - a GqModelDesc as the kernels read it, in host memory: the model block, the SoA cloud vertices, the height field. */
#pragma once
#include <vector>
#include "gq_host_model.h"

struct EmuModel { GqDevModel M; std::vector<float> vx, vy, vz, hf; };
inline int emu_build_model(const GqModelDesc* desc, EmuModel& m, char* err, int errlen) { /* 0, or -1 with the text in err */
  if (gq_build_dev_model(desc, &m.M, &m.vx, &m.vy, &m.vz, err, (size_t)errlen)) return -1;
  gq_hfield_heights(desc, &m.hf);
  m.M.hf_data = m.hf.empty() ? nullptr : m.hf.data();
  return 0;
}
