/* TEST INFRASTRUCTURE - runs the unmodified camera passes (csrc/gq_camera.h: camera_pose_wave, camera_tile_wave<false>) under the host
 * SIMT emulator, one emulated wavefront per env and per tile, and exposes the ray primitives of that file one by one. */
#include <functional>
#include <vector>

#include "gq_device.h"          /* the emulator shim (this directory comes first on the include path) */
#include "gq_camera_call.h"
#include "emu_model.h"

void emu_run_wave(unsigned block, unsigned nblocks, const std::function<void()>& body);

/* gq_camera on host memory: the call record is filled by the library's own cam_fill_call, the launches are gq_launch_camera's */
extern "C" int emu_camera(const GqModelDesc* desc, int n_envs, const double* qpos, int qpos_stride, int body, const double* pos, const double* quat,
                          float fovy_deg, int width, int height, float znear, float zfar, int flags, const float* hull_planes,
                          const int32_t* hull_plane_adr, float* depth, int32_t* seg, double* cam_xpos, float* cam_xmat, char* err, int errlen) {
  static EmuModel m;
  if (emu_build_model(desc, m, err, errlen)) return -1;
  const GqDevModel& M = m.M;
  int32_t lg_cloud[GQ_MAXLG];
  gq::cam_lg_cloud(lg_cloud, M, desc);
  gq::CamCall c{};
  if (gq::cam_fill_call(c, "emu_camera", M, lg_cloud, desc->ncloud, desc->ngeom, qpos, qpos_stride, body, pos, quat, fovy_deg, width, height, znear, zfar,
                        flags, hull_planes, hull_plane_adr, depth, seg, cam_xpos, cam_xmat, err, (size_t)errlen)) return -1;
  std::vector<float> rec((size_t)n_envs * GQ_CAM_REC, 0.0f);
  std::vector<double> cpos((size_t)n_envs * 3, 0.0);
  c.rec = rec.data(); c.cpos = cpos.data();
  for (int e = 0; e < n_envs; e++)
    emu_run_wave((unsigned)e, (unsigned)n_envs, [&]() {
      __shared__ gq::WaveMem W;
      gq::camera_pose_wave(W, *gq::mptr(&M), c, e);
    });
  const int tiles = ((width + GQ_CAM_TILE - 1) / GQ_CAM_TILE) * ((height + GQ_CAM_TILE - 1) / GQ_CAM_TILE);
  /* the envs last to first (the device runs them in no order): a store past env e's image then lands on pixels env e + 1 has already
   * written and shows in the result, instead of being painted over */
  for (int e = n_envs - 1; e >= 0; e--)
    for (int t = 0; t < tiles; t++)
      emu_run_wave((unsigned)t, (unsigned)tiles, [&]() { gq::camera_tile_wave<false>(M, c, nullptr, t, e); });
  return 0;
}

/* the robot-geom primitives on n rays (o, d: [n][3], geom frame).  kind 0 cam_sphere (par: r), 1 cam_cylinder (r, h), 2 cam_capsule (r, h),
 * 3 cam_cone (rb, zb, zt), 4 cam_hull (P: [np][4]).  t: the entry parameter as returned; part: the part output (0 for the sphere) */
extern "C" void emu_cam_prim(int kind, int n, const float* o, const float* d, const float* par, const float* P, int np, float* t, int32_t* part) {
  for (int i = 0; i < n; i++) {
    const gq::V3 oo = gq::v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), dd = gq::v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    int pt = 0;
    switch (kind) {
      case 0: t[i] = gq::cam_sphere(oo, dd, par[0]); break;
      case 1: t[i] = gq::cam_cylinder(oo, dd, par[0], par[1], pt); break;
      case 2: t[i] = gq::cam_capsule(oo, dd, par[0], par[1], pt); break;
      case 3: t[i] = gq::cam_cone(oo, dd, par[0], par[1], par[2], pt); break;
      default: t[i] = gq::cam_hull(oo, dd, P, np, pt); break;
    }
    part[i] = pt;
  }
}
/* ray_slab<float> from the caller's bounds tin / tout ([n], updated in place); hit: its return value, axis: -1 where no slab set tin */
extern "C" void emu_ray_slab(int n, const float* ol, const float* dl, const float* s, float* tin, float* tout, int32_t* axis, int32_t* hit) {
  for (int i = 0; i < n; i++) {
    int ax = -1;
    hit[i] = gq::ray_slab<float>(ol + 3 * i, dl + 3 * i, s, tin[i], tout[i], &ax) ? 1 : 0;
    axis[i] = ax;
  }
}
/* ray_triangle<float> / <double> of n rays against the triangle (a, b, c); t is written where hit */
extern "C" void emu_ray_triangle_f(int n, const float* o, const float* d, const float* a, const float* b, const float* c, float* t, int32_t* hit) {
  for (int i = 0; i < n; i++) hit[i] = gq::ray_triangle<float>(o + 3 * i, d + 3 * i, a, b, c, t[i]) ? 1 : 0;
}
extern "C" void emu_ray_triangle_d(int n, const double* o, const double* d, const double* a, const double* b, const double* c, double* t, int32_t* hit) {
  for (int i = 0; i < n; i++) hit[i] = gq::ray_triangle<double>(o + 3 * i, d + 3 * i, a, b, c, t[i]) ? 1 : 0;
}
/* ray_hfield<double> over a caller-given grid H [nrow][ncol] of cells dx x dy centred on the origin (half sizes sx, sy, highest elevation
 * zmax): ol, d [n][3], tmin [n]; t: the return value, tri: the triangle (-1 where none) */
extern "C" void emu_ray_hfield(const float* H, int nrow, int ncol, float sx, float sy, float dx, float dy, float zmax, int n, const double* ol,
                               const double* d, const double* tmin, double* t, int32_t* tri) {
  static GqDevModel M;
  M.hf_nrow = nrow; M.hf_ncol = ncol; M.hf_sx = sx; M.hf_sy = sy; M.hf_dx = dx; M.hf_dy = dy; M.hf_zmax = zmax; M.hf_data = H;
  for (int i = 0; i < n; i++) {
    int tr = -1;
    t[i] = gq::ray_hfield<double>(M, ol + 3 * i, d + 3 * i, tmin[i], &tr);
    tri[i] = tr;
  }
}
