/*
 * gq_policy_scan.h - the HEIGHT SCAN of the closed-loop rollout's policy (gq_rollout_policy_scan, gq_height_scan_eval): the law that turns
 * the hit points of the batch's base-following HeightMap (gq_batch_set_heightmap: [N][rows * cols][3], cast by the stepping wavefront at
 * every step) into columns of the policy's input row.  Where those columns stand in the row, and the device block of a call:
 * gq_policy_dev.h.  Plain C++: compiles with the product's gq_device.h and with the host shim (tests/simt_emu).
 *
 * THE LAW, for cell c in the HeightMap's own cell order i * cols + j:
 *   s_c = clamp((z_base - offset) - z_hit_c, -clip, +clip) * scale
 * fp32, contraction off, one rounding per operation: two subtractions in the order written, fmaxf, fminf, one multiply.  z_hit_c is word 2
 * of the cell's hit point as the step kernel wrote it (a ray that hits nothing lands at pz + 1 above the ray's origin and saturates at
 * -clip); z_base is the z column of the env's observation row (base_pos, or failing that qpos).  No shift / scale table acts on a scan
 * column.
 */
#pragma once
#include <gq_device.h> /* angle brackets: the include path decides (csrc/ for the product, tests/simt_emu/ for the host programs) */
#include <cmath>
#include <cstdint>

namespace gq {

struct ScanLaw {
  float offset, clip, scale; /* finite; clip > 0 */
};

__host__ __device__ inline float height_scan_cell(const ScanLaw& S, const float z_base, const float z_hit) {
#pragma clang fp contract(off)
  const float zr = z_base - S.offset;
  const float d = zr - z_hit;
  const float lo = fmaxf(d, -S.clip);
  const float c = fminf(lo, S.clip);
  return c * S.scale;
}
}  // namespace gq
