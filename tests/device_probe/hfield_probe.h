/* TEST INFRASTRUCTURE - the bodies of the height-field entry points, shared by tests/device_probe/probe.hip (hipcc, the product's flags and
 * headers) and tests/simt_emu/emu_step.cpp (g++, the emulator's shim), so that both backends of tests/hfield_cases.py run the same thing around
 * csrc/gq_boxes.h's closest_on_triangle, hf_triangle_under and sphere_hfield.  Lane = case.
 *
 * The model: a zeroed GqDevModel whose hf_* fields are filled from the grid's description exactly as csrc/gq_host_model.cpp fills them
 * (hfp_fill), the elevations as gq_hfield_heights makes them.  grid[8] (float64): nrow, ncol, size x / y / elevation, pos x / y / z. */
#pragma once
#include <cmath>
#include <vector>
#include "gq_boxes.h"

namespace hfprobe {

/* raw [nrow][ncol]: the normalised elevations of GqModelDesc::hfield_data (host memory); heights: metres relative to pos z */
inline void hfp_fill(GqDevModel& M, const double* grid, const float* raw, std::vector<float>& heights) {
  const int nr = (int)grid[0], nc = (int)grid[1];
  const double sx = grid[2], sy = grid[3], sz = grid[4];
  M.hf_nrow = nr; M.hf_ncol = nc; M.hf_cls = 0;
  for (int i = 0; i < 3; i++) M.hf_pos[i] = (float)grid[5 + i];
  M.hf_sx = (float)sx; M.hf_sy = (float)sy;
  const double dx = 2 * sx / (nc - 1), dy = 2 * sy / (nr - 1);
  M.hf_dx = (float)dx; M.hf_dy = (float)dy; M.hf_inv_dx = (float)(1 / dx); M.hf_inv_dy = (float)(1 / dy);
  double slope = 0, zmax = 0;
  const double dd = std::sqrt(dx * dx + dy * dy);
  for (int r = 0; r < nr; r++)
    for (int c = 0; c < nc; c++) {
      const double h = sz * raw[r * nc + c];
      if (h > zmax) zmax = h;
      if (c + 1 < nc) slope = std::fmax(slope, std::fabs(sz * raw[r * nc + c + 1] - h) / dx);
      if (r + 1 < nr) slope = std::fmax(slope, std::fabs(sz * raw[(r + 1) * nc + c] - h) / dy);
      if (r + 1 < nr && c > 0) slope = std::fmax(slope, std::fabs(sz * raw[(r + 1) * nc + c - 1] - h) / dd);
    }
  M.hf_maxslope = (float)(std::sqrt(2.0) * slope); M.hf_zmax = (float)zmax;
  heights.resize((size_t)nr * nc);
  for (size_t i = 0; i < heights.size(); i++) heights[i] = (float)(sz * (double)raw[i]);
}

/* closest_on_triangle.  in[n][12]: p, a, b, c; out[n][3]: the point; interior[n] */
__device__ inline void hfp_triangle_case(int i, const float* in, float* out, int32_t* interior) {
  const float* a = in + (size_t)i * 12;
  bool inside;
  const gq::V3 q = gq::closest_on_triangle(gq::v3(a[0], a[1], a[2]), gq::v3(a[3], a[4], a[5]), gq::v3(a[6], a[7], a[8]), gq::v3(a[9], a[10], a[11]), inside);
  out[3 * (size_t)i] = q.x; out[3 * (size_t)i + 1] = q.y; out[3 * (size_t)i + 2] = q.z;
  interior[i] = inside ? 1 : 0;
}

/* sphere_hfield and hf_triangle_under in the coordinates hfield_item_scan gives them: base[n][2] (float64) the x / y of the robot's base,
 * q[n][5] (float32): the sphere's centre (x, y relative to the base, z in the world), radius, reach.  The reference corner and its offset are
 * computed as hfield_item_scan computes them.  hit[n]; out[n][4]: dist, normal of sphere_hfield (whatever it left there);
 * under[n][5]: 1 / 0, then the height of the triangle under the centre at the centre's (x, y) relative to pos z and its normal */
__device__ inline void hfp_sphere_case(int i, const GQ_MODEL GqDevModel& m, const double* base, const float* q, int32_t* hit, float* out, float* under) {
  const GQ_MODEL float* H = gq::mptr(m.hf_data);
  const double bx = base[2 * (size_t)i], by = base[2 * (size_t)i + 1];
  const float* a = q + (size_t)i * 5;
  const double gx = (bx - (double)m.hf_pos[0] + (double)m.hf_sx) * (double)m.hf_inv_dx, gy = (by - (double)m.hf_pos[1] + (double)m.hf_sy) * (double)m.hf_inv_dy;
  const gq::HfRef ref = {(int)floor(gx), (int)floor(gy)};
  const gq::V3 hp = gq::v3((float)((double)m.hf_pos[0] - (double)m.hf_sx + (double)ref.cb * (double)m.hf_dx - bx),
                           (float)((double)m.hf_pos[1] - (double)m.hf_sy + (double)ref.rb * (double)m.hf_dy - by), m.hf_pos[2]);
  const gq::V3 p = gq::v3(a[0], a[1], a[2]) - hp;
  float d; gq::V3 n;
  hit[i] = gq::sphere_hfield(m, H, ref, p, a[3], a[4], d, n) ? 1 : 0;
  float* o = out + 4 * (size_t)i;
  o[0] = d; o[1] = n.x; o[2] = n.y; o[3] = n.z;
  gq::HfTri t;
  float* u = under + 5 * (size_t)i;
  u[0] = u[1] = u[2] = u[3] = u[4] = 0.0f;
  if (gq::hf_triangle_under(m, H, ref, p.x, p.y, t)) {
    u[0] = 1.0f; u[1] = t.a.z - (t.n.x * (p.x - t.a.x) + t.n.y * (p.y - t.a.y)) / t.n.z; u[2] = t.n.x; u[3] = t.n.y; u[4] = t.n.z;
  }
}

} /* namespace hfprobe */
