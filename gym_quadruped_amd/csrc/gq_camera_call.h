/*
 * gq_camera_call.h - the host side of a gq_camera call: the caller's arguments into the CamCall both launches take by value (gq_camera.h).
 * gq_api.hip's camera_run fills its call with this; so does the host emulator of the tests (tests/simt_emu), which then runs the same
 * pose and pixel passes over the same record.  Host code only.
 */
#pragma once
#include <cmath>
#include <cstdio>

#include "gq.h"
#include "gq_camera.h"

namespace gq {

/* lg_cloud[i] (GQ_MAXLG entries): the GqModelDesc cloud of host.lg[i], -1: none - gq_camera's face-plane table is indexed by cloud */
inline void cam_lg_cloud(int32_t* lg_cloud, const GqDevModel& host, const GqModelDesc* desc) {
  for (int i = 0; i < host.nlg; i++) lg_cloud[i] = desc->geom_cloudid[host.item_geomid[4 + i]];
}
/* c: zero-initialised by the caller; rec and cpos (the batch's scratch) stay the caller's to set.  host: the model as gq_build_dev_model
 * made it; lg_cloud: as cam_lg_cloud fills it, ncloud / ngeom: the desc's counts.  The arguments are taken as the
 * entry point's own checks left them.  Returns 0, or 1 with the error text (fn: the entry point's name) in err. */
inline int cam_fill_call(CamCall& c, const char* fn, const GqDevModel& host, const int32_t* lg_cloud, int ncloud, int ngeom, const double* qpos,
                         int qpos_stride, int body, const double pos[3], const double quat[4], float fovy_deg, int width, int height, float znear,
                         float zfar, int flags, const float* hull_planes, const int32_t* hull_plane_adr, float* depth, int32_t* seg, double* cam_xpos,
                         float* cam_xmat, char* err, size_t errlen) {
  const double qn = std::sqrt(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
  if (!(qn > 0.0)) { std::snprintf(err, errlen, "%s: zero quaternion", fn); return 1; }
  for (int i = 0; i < host.nlg; i++) {
    if (host.lg[i].ptype != 0) continue;
    if (!hull_planes || !hull_plane_adr) { std::snprintf(err, errlen, "%s: the model has hull geoms and no face planes were passed", fn); return 1; }
    const int cl = lg_cloud[i];
    if (cl < 0 || cl >= ncloud) { std::snprintf(err, errlen, "%s: link geom %d has no cloud", fn, i); return 1; }
    c.plane_adr[i] = hull_plane_adr[cl]; c.plane_num[i] = hull_plane_adr[cl + 1] - hull_plane_adr[cl];
    if (c.plane_adr[i] < 0 || c.plane_num[i] < 4) { std::snprintf(err, errlen, "%s: cloud %d has %d face planes (a hull has at least 4)", fn, cl, c.plane_num[i]); return 1; }
  }
  const double th = std::tan(0.5 * (double)fovy_deg * 3.14159265358979323846 / 180.0);
  c.qpos = qpos; c.qpos_stride = qpos_stride; c.body = body;
  for (int k = 0; k < 3; k++) c.pos[k] = pos[k];
  for (int k = 0; k < 4; k++) c.quat[k] = (float)(quat[k] / qn);
  c.width = width; c.height = height; c.flags = flags; c.ngeom = ngeom;
  c.tan_x = (float)(th * width / height); c.tan_y = (float)th; c.znear = znear; c.zfar = zfar;
  c.planes = hull_planes; c.xpos_out = cam_xpos; c.xmat_out = cam_xmat; c.depth = depth; c.seg = seg;
  return 0;
}

}  // namespace gq
