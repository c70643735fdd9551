/*
 * gq_camera.h - the depth / segmentation camera (include/gq.h gq_camera; the reference renders it with mujoco.Renderer,
 * sensors/rgbd_camera.py) as a ray caster, in two launches (gq_kernels.hip camera_pose_kernel, camera_pixel_kernel):
 *  - pose pass, one wavefront per env: the kinematics of the caller's qpos, the camera frame (body pose o camera offset), and, lane = robot
 *    geom, every geom's frame relative to the camera (fp32) into the batch's scratch record.  The camera origin in the world is fp64.
 *  - pixel pass, one wavefront per 8 x 8 tile of one env: lane = candidate culls the robot geoms and the world boxes against the tile's
 *    view cone (two ballots, as heightmap_rays does for boxes), then lane = pixel walks the survivors wave-uniformly.
 * gq_camera_layered adds a ghost pose pass (one wavefront per env and ghost: the robot geoms posed from each ghost qpos, relative to the
 * env's camera) and composites ghosts and markers over the shaded image in its pixel pass (cam_layers).  The robot and the ghosts go through
 * one cull, cast, normal and light routine (cam_rob_cull, cam_rob_cast, cam_rob_normal, cam_light); the file runs from the primitives up to
 * the pixel pass, camera_tile_wave, at its end.
 * Also the static-geom ray tests that gq_ray's ray_kernel and the pixel pass share (slab, height-field cell walk).
 * Semantics: pixel (r, c) looks along ((2 (c + .5) / W - 1) tan(fovy / 2) W / H, (1 - 2 (r + .5) / H) tan(fovy / 2), -1) in
 * the camera frame, so a hit's ray parameter is its planar depth; the nearest hit in [znear, zfar] wins, none gives zfar.  Convex geoms are
 * seen only from outside (front faces): a ray that starts inside one, or enters it before znear, does not see it.
 */
#pragma once
#include "gq_step_body.h"

namespace gq {

#define GQ_CAM_TILE 8                          /* a wavefront renders one GQ_CAM_TILE x GQ_CAM_TILE tile */
#define GQ_CAM_NROB (4 + GQ_MAXLG)             /* robot geoms: the four foot spheres, then lg[] */
#define GQ_CAM_REC (12 + 12 * GQ_CAM_NROB)     /* scratch floats per env: camera rotation (9, world), pad (3), per robot geom R (9) t (3) */

/* one gq_camera call, by value in both launches */
struct CamCall {
  const double* qpos; int qpos_stride;
  int body;                                    /* ModelDesc body of the camera, 0 = world */
  double pos[3]; float quat[4];                /* camera frame in the body frame (quat normalised) */
  int width, height, flags, ngeom;             /* flags: bit 0 robot, bit 1 static scene, bit 2 track; ngeom: segmentation id of the floor */
  float tan_x, tan_y, znear, zfar;             /* tan(fovy / 2) W / H, tan(fovy / 2) */
  const float* planes;                         /* [P][4] face planes n.x <= d of the hull geoms, geom frame */
  int32_t plane_adr[GQ_MAXLG], plane_num[GQ_MAXLG]; /* per lg[]: first plane and count (0: not a hull) */
  float* rec;                                  /* [N][GQ_CAM_REC] batch scratch: pose pass -> pixel pass */
  double* cpos;                                /* [N][3] batch scratch: camera origin, world, fp64 */
  double* xpos_out; float* xmat_out;           /* optional copies for the caller */
  float* depth; int32_t* seg;                  /* [N][H][W] */
};

/* the shaded pixel pass (gq_camera_shaded): GqCamShade as the library resolved it, by value */
#define GQ_CAM_NLIGHT 8                        /* lights, headlight included */
struct CamLight {
  float pos[3], dir[3];                        /* world; dir unit (kind 0: unused) */
  float amb[3], dif[3], spe[3], att[3];
  float cos_cut, expo;                         /* spot cone: cos(cutoff), exponent */
  int kind;                                    /* 0 headlight (L = camera +z), 1 directional, 2 spot */
};
struct CamShade {
  const float* geom_mat;                       /* [ngeom][7] rgba, specular, shininess, emission (device) */
  uint32_t* rgba;                              /* [N][H][W] RGBA8 */
  float box_mat[7];                            /* world boxes, same layout */
  float rgb1[3], rgb2[3], mark_rgb[3], square, mark_w, floor_mat[3];   /* floor / height field checker; floor_mat: spec, shin, emis */
  float top[3], bottom[3];                     /* background */
  int nlight;
  CamLight light[GQ_CAM_NLIGHT];
};

/* the layered pixel pass (gq_camera_layered): translucent ghost robots and markers over the shaded image, by value */
#define GQ_CAM_NLAYER 8                        /* layers composited per pixel (include/gq.h GQ_CAM_MAXLAYER) */
#define GQ_CAM_GREC (12 * GQ_CAM_NROB)         /* ghost record floats per (env, ghost): per robot geom R (9) t (3), camera frame */
struct CamLayers {
  const double* ghost_qpos; int ghost_stride, n_ghost;   /* [N][n_ghost][ghost_stride] */
  const float* ghost_alpha;                    /* [N][n_ghost] */
  const float* ghost_rgb;                      /* [N][n_ghost][3], or null: geom_mat's colours */
  int n_marker; const float* markers;          /* [N][n_marker][16]: type, pos, axis, size, rgba, pad (world) */
  float* grec;                                 /* [N][n_ghost][GQ_CAM_GREC] batch scratch: ghost pose pass -> pixel pass */
};

/* ---- static-geom ray tests (T = double: gq_ray; the pixel pass uses float for boxes, origin relative to the camera) */
template <class T> __device__ __forceinline__ T ray_far();   /* "no bound yet" */
template <> __device__ __forceinline__ double ray_far<double>() { return 1e300; }
template <> __device__ __forceinline__ float ray_far<float>() { return 1e30f; }
template <class T>
__device__ inline bool ray_triangle(const T* o, const T* d, const T* a, const T* b, const T* c, T& t) {
  const T e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const T pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
  const T det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
  if (fabs(det) < T(1e-14)) return false;
  const T inv = T(1) / det, tv[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
  const T u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
  if (u < T(-1e-9) || u > T(1) + T(1e-9)) return false;
  const T qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  const T v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv;
  if (v < T(-1e-9) || u + v > T(1) + T(1e-9)) return false;
  t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
  return t >= T(0);
}
/* slab test of the ray o + t d against the box |x_k| <= s_k (box frame); tin / tout come in as the caller's bounds */
template <class T>
__device__ inline bool ray_slab(const T* ol, const T* dl, const T* s, T& tin, T& tout, int* axis = nullptr) {   /* axis: the slab that sets tin */
  bool hit = true;
  for (int k = 0; k < 3 && hit; k++) {
    if (fabs(dl[k]) < T(1e-14)) { hit = fabs(ol[k]) <= s[k]; continue; }
    T t0 = (-s[k] - ol[k]) / dl[k], t1 = (s[k] - ol[k]) / dl[k];
    if (t0 > t1) { const T tt = t0; t0 = t1; t1 = tt; }
    if (t0 > tin) { tin = t0; if (axis) *axis = k; }
    if (t1 < tout) tout = t1;
    hit = tin <= tout;
  }
  return hit;
}
/* a world box: r = origin - box centre, d: direction, both in world axes */
template <class T, class Box>
__device__ inline bool ray_box(const Box& B, const T* r, const T* d, T& tin, T& tout, int* axis = nullptr) {
  T ol[3], dl[3], s[3];
  for (int k = 0; k < 3; k++) {
    ol[k] = (T)B.mat[k] * r[0] + (T)B.mat[3 + k] * r[1] + (T)B.mat[6 + k] * r[2];
    dl[k] = (T)B.mat[k] * d[0] + (T)B.mat[3 + k] * d[1] + (T)B.mat[6 + k] * d[2];
    s[k] = (T)B.size[k];
  }
  return ray_slab(ol, dl, s, tin, tout, axis);
}
/* the height field: ol = origin - hf_pos.  The cells under the ray's ground track are walked from the parameter max(tmin, entry into the
 * field's bounding box), two triangles each; returns the first hit >= tmin, -1 if none.  tri: the triangle hit, 2 (row ncol + col) + k
 * (k = 0: corners (c, r), (c + 1, r), (c, r + 1); k = 1: (c + 1, r + 1), (c, r + 1), (c + 1, r)). */
template <class T, class Mref>
__device__ inline T ray_hfield(const Mref& M, const T* ol, const T* d, const T tmin, int* tri = nullptr) {
  const T sx = M.hf_sx, sy = M.hf_sy, dx = M.hf_dx, dy = M.hf_dy, zmax = (T)M.hf_zmax;
  /* parameter interval of the ray inside the field's bounding box [-sx, sx] x [-sy, sy] x [0, zmax] */
  T t0 = tmin, t1 = ray_far<T>();
  bool in = true;
  const T lo[3] = {-sx, -sy, T(0)}, hi[3] = {sx, sy, zmax};
  for (int k = 0; k < 3 && in; k++) {
    if (fabs(d[k]) < T(1e-14)) { in = ol[k] >= lo[k] && ol[k] <= hi[k]; continue; }
    T a = (lo[k] - ol[k]) / d[k], b2 = (hi[k] - ol[k]) / d[k];
    if (a > b2) { const T tt = a; a = b2; b2 = tt; }
    if (a > t0) t0 = a;
    if (b2 < t1) t1 = b2;
    in = t0 <= t1;
  }
  if (!in) return T(-1);
  const int nc = M.hf_ncol, nr = M.hf_nrow;
  const float* H = M.hf_data;
  /* walk the cells along the ground track from t0 to t1 (2-D DDA) */
  T t = t0;
  const T px = ol[0] + t * d[0], py = ol[1] + t * d[1];
  int c = (int)floor((px + sx) / dx), r = (int)floor((py + sy) / dy);
  c = c < 0 ? 0 : (c > nc - 2 ? nc - 2 : c); r = r < 0 ? 0 : (r > nr - 2 ? nr - 2 : r);
  const int stc = d[0] > 0 ? 1 : -1, str = d[1] > 0 ? 1 : -1;
  for (int it = 0; it < nc + nr + 2; it++) {
    const T x0 = -sx + dx * c, y0 = -sy + dy * r, x1 = x0 + dx, y1 = y0 + dy;
    const T h00 = H[r * nc + c], h10 = H[r * nc + c + 1], h01 = H[(r + 1) * nc + c], h11 = H[(r + 1) * nc + c + 1];
    const T A[3] = {x0, y0, h00}, B[3] = {x1, y0, h10}, Cc[3] = {x0, y1, h01}, D[3] = {x1, y1, h11};
    T th, tb = T(-1);
    int k = 0;
    if (ray_triangle(ol, d, A, B, Cc, th) && th >= tmin) tb = th;
    if (ray_triangle(ol, d, D, Cc, B, th) && th >= tmin && (tb < T(0) || th < tb)) { tb = th; k = 1; }
    if (tb >= T(0)) {
      if (tri) *tri = 2 * (r * nc + c) + k;
      return tb;
    }
    /* next cell: the nearer of the two cell borders the track crosses */
    const T tx = fabs(d[0]) < T(1e-14) ? ray_far<T>() : ((stc > 0 ? x1 : x0) - ol[0]) / d[0];
    const T ty = fabs(d[1]) < T(1e-14) ? ray_far<T>() : ((str > 0 ? y1 : y0) - ol[1]) / d[1];
    if (tx < ty) { c += stc; t = tx; } else { r += str; t = ty; }
    if (t > t1 || c < 0 || r < 0 || c > nc - 2 || r > nr - 2) break;
  }
  return T(-1);
}

/* ---- robot geoms, in the geom frame (o, d: the ray there).  Each returns the entry parameter (front face), or -1 when the ray misses.
 * A ray that starts inside gets -1 from the sphere and the capsule, and from the cylinder, the hull and the cone the entry behind the
 * origin (negative); so does a ray that points away from the shape.  The caller keeps entries in [znear, best], which drops both.
 * part: which surface the entry is on (cam_shade); callers that do not shade pass a local they never read. */
__device__ inline float cam_sphere(V3 o, V3 d, float r) {
  const float a = dot(d, d), b = dot(o, d), c = dot(o, o) - r * r;
  if (c <= 0.0f) return -1.0f;
  const float disc = b * b - a * c;
  return disc < 0.0f ? -1.0f : (-b - sqrtf(disc)) / a;
}
__device__ inline float cam_cylinder(V3 o, V3 d, float r, float h, int& part) {   /* axis z, radius r, half length h; part 0 side, 1 cap */
  float tin = -1e30f, tout = 1e30f;
  part = 1;
  if (fabsf(d.z) < 1e-20f) { if (fabsf(o.z) > h) return -1.0f; }
  else {
    float t0 = (-h - o.z) / d.z, t1 = (h - o.z) / d.z;
    if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
    tin = t0; tout = t1;
  }
  const float a = d.x * d.x + d.y * d.y, b = o.x * d.x + o.y * d.y, c = o.x * o.x + o.y * o.y - r * r;
  if (a < 1e-20f) { if (c > 0.0f) return -1.0f; }
  else {
    const float disc = b * b - a * c;
    if (disc < 0.0f) return -1.0f;
    const float s = sqrtf(disc), ts = (-b - s) / a;
    if (ts > tin) part = 0;
    tin = fmaxf(tin, ts); tout = fminf(tout, (-b + s) / a);
  }
  return tin <= tout ? tin : -1.0f;
}
__device__ inline float cam_capsule(V3 o, V3 d, float r, float h, int& part) {   /* part 0 cylinder, 1 cap at +h, 2 cap at -h */
  const float zc = fminf(fmaxf(o.z, -h), h);
  if (o.x * o.x + o.y * o.y + (o.z - zc) * (o.z - zc) <= r * r) return -1.0f;   /* inside */
  float best = 1e30f;
  int pc;
  const float tc = cam_cylinder(o, d, r, h, pc), t0 = cam_sphere(o - v3(0.0f, 0.0f, h), d, r), t1 = cam_sphere(o + v3(0.0f, 0.0f, h), d, r);
  part = 0;
  if (tc > 0.0f) best = tc;
  if (t0 > 0.0f && t0 < best) { best = t0; part = 1; }
  if (t1 > 0.0f && t1 < best) { best = t1; part = 2; }
  return best < 1e30f ? best : -1.0f;
}
/* Cyrus-Beck against the hull's face planes; the plane loop is wave-uniform (the addresses too: scalar loads) */
__device__ inline float cam_hull(V3 o, V3 d, const float* P, int n, int& part) {   /* part: the entry plane */
  float tin = -1e30f, tout = 1e30f;
  part = 0;
  bool miss = false;
  for (int k = 0; k < n; k++) {
    const V3 nk = v3(P[4 * k], P[4 * k + 1], P[4 * k + 2]);
    const float den = dot(nk, d), num = P[4 * k + 3] - dot(nk, o);
    if (fabsf(den) < 1e-20f) { miss |= num < 0.0f; continue; }
    const float t = num / den;
    if (den < 0.0f) {
      if (t > tin) part = k;
      tin = fmaxf(tin, t);
    } else tout = fminf(tout, t);
  }
  return !miss && tin <= tout ? tin : -1.0f;
}

/* the ghost pose pass's geom frames.  lane = robot geom: its frame relative to the camera (rotation Rc, origin pc relative to the base x/y
 * of W's kinematics), R = Rc' Rg, t = Rc' (pg - pc), 12 floats per geom from out.  camera_pose_wave holds the same text for the robot: the
 * one pair left apart, because the compiler contracts the sum for R differently in the two places (see there) */
template <class Mref>
__device__ __forceinline__ void cam_geom_frames(WaveMem& W, const Mref& m, const float* Rc, const V3 pc, float* out, const int lane) {
  const int nrob = 4 + m.nlg;
  if (lane < nrob) {
    V3 pg;
    float Rg[9];
    if (lane < 4) {
      const FootRec FR = foot_fetch(m, lane);
      const int b = 3 + 3 * FR.leg;
      pg = ld3(W.xpos[b]) + matvec(W.xmat[b], ld3(FR.pos));
      for (int k = 0; k < 9; k++) Rg[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    } else {
      const auto& G = m.lg[lane - 4];
      const int b = G.body;
      pg = ld3(W.xpos[b]) + matvec(W.xmat[b], ld3(G.pos));
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rg[3 * i + j] = W.xmat[b][3 * i] * G.mat[j] + W.xmat[b][3 * i + 1] * G.mat[3 + j] + W.xmat[b][3 * i + 2] * G.mat[6 + j];
    }
    float* o = out + 12 * lane;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) o[3 * i + j] = Rc[i] * Rg[j] + Rc[3 + i] * Rg[3 + j] + Rc[6 + i] * Rg[6 + j];
    st3(o + 9, matTvec(Rc, pg - pc));
  }
}

/* pose pass: one wavefront per env; W: the wave's LDS */
template <class Mref>
__device__ inline void camera_pose_wave(WaveMem& W, const Mref& m, const CamCall& c, const int env) {
  const int lane = lane_id();
#if GQ_TICKSET
  if (lane == 0) W.tk_T = nullptr;
#endif
  load_qpos_row(W, c.qpos + (size_t)env * c.qpos_stride, lane);
  wave_barrier();
  stage_kinematics(W, link_fetch(m, lane));
  /* the camera frame relative to the base x/y, like every kinematic quantity */
  float Rq[9], Rc[9];
  q2mat(Rq, Q4{c.quat[0], c.quat[1], c.quat[2], c.quat[3]});
  V3 pc;
  if (c.body == 0) {
    pc = v3((float)(c.pos[0] - W.bxy[0]), (float)(c.pos[1] - W.bxy[1]), (float)c.pos[2]);
    for (int k = 0; k < 9; k++) Rc[k] = Rq[k];
  } else if (c.flags & 4) { /* GQ_CAM_TRACK: the body's position, the offset and the orientation in world axes */
    pc = ld3(W.xpos[c.body - 1]) + v3((float)c.pos[0], (float)c.pos[1], (float)c.pos[2]);
    for (int k = 0; k < 9; k++) Rc[k] = Rq[k];
  } else {
    const int kb = c.body - 1;
    pc = ld3(W.xpos[kb]) + matvec(W.xmat[kb], v3((float)c.pos[0], (float)c.pos[1], (float)c.pos[2]));
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) Rc[3 * i + j] = W.xmat[kb][3 * i] * Rq[j] + W.xmat[kb][3 * i + 1] * Rq[3 + j] + W.xmat[kb][3 * i + 2] * Rq[6 + j];
  }
  float* rec = c.rec + (size_t)env * GQ_CAM_REC;
  if (lane < 9) {
    rec[lane] = Rc[lane];
    if (c.xmat_out) c.xmat_out[(size_t)env * 9 + lane] = Rc[lane];
  } else if (lane < 12) {
    const int k = lane - 9;
    const double p = c.body == 0 ? c.pos[k] : (k == 0 ? W.bxy[0] + (double)pc.x : k == 1 ? W.bxy[1] + (double)pc.y : (double)pc.z);
    c.cpos[(size_t)env * 3 + k] = p;
    if (c.xpos_out) c.xpos_out[(size_t)env * 3 + k] = p;
  }
  /* lane = robot geom: its frame in the camera frame, the text of cam_geom_frames and not a call to it.  Here the compiler rounds R's sum
   * a b + c d + e f as fma(e, f, fma(c, d, a b)), inside the helper (called from here or from the ghost pass) as fma(e, f, fma(a, b, c d));
   * a call moves the robot's depths by an ulp or two (measured).  One explicit order for both changes what is drawn. */
  const int nrob = 4 + m.nlg;
  if (lane < nrob) {
    V3 pg;
    float Rg[9];
    if (lane < 4) {
      const FootRec FR = foot_fetch(m, lane);
      const int b = 3 + 3 * FR.leg;
      pg = ld3(W.xpos[b]) + matvec(W.xmat[b], ld3(FR.pos));
      for (int k = 0; k < 9; k++) Rg[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    } else {
      const auto& G = m.lg[lane - 4];
      const int b = G.body;
      pg = ld3(W.xpos[b]) + matvec(W.xmat[b], ld3(G.pos));
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rg[3 * i + j] = W.xmat[b][3 * i] * G.mat[j] + W.xmat[b][3 * i + 1] * G.mat[3 + j] + W.xmat[b][3 * i + 2] * G.mat[6 + j];
    }
    float* o = rec + 12 + 12 * lane;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) o[3 * i + j] = Rc[i] * Rg[j] + Rc[3 + i] * Rg[3 + j] + Rc[6 + i] * Rg[6 + j];
    st3(o + 9, matTvec(Rc, pg - pc));
  }
}

/* ghost pose pass (gq_camera_layered): one wavefront per (env, ghost).  The kinematics of the ghost's qpos; the camera stays the one the
 * pose pass placed from the env's own qpos (rec, cpos), so each ghost geom's frame is taken relative to that camera into L.grec. */
template <class Mref>
__device__ inline void camera_ghost_wave(WaveMem& W, const Mref& m, const CamCall& c, const CamLayers& L, const int ghost, const int env) {
  const int lane = lane_id();
#if GQ_TICKSET
  if (lane == 0) W.tk_T = nullptr;
#endif
  const size_t row = (size_t)env * L.n_ghost + ghost;
  load_qpos_row(W, L.ghost_qpos + row * L.ghost_stride, lane);
  wave_barrier();
  stage_kinematics(W, link_fetch(m, lane));
  const float* rec = c.rec + (size_t)env * GQ_CAM_REC;
  float Rc[9];
  for (int k = 0; k < 9; k++) Rc[k] = rec[k];
  const double* co = c.cpos + (size_t)env * 3;
  const V3 pc = v3((float)(co[0] - W.bxy[0]), (float)(co[1] - W.bxy[1]), (float)co[2]);   /* relative to the ghost's base x/y */
  cam_geom_frames(W, m, Rc, pc, L.grec + row * GQ_CAM_GREC, lane);
}

/* does the sphere (centre ctr, camera frame) meet the cone (unit axis ax, half angle (ca, sa)) within the depth range?  Conservative:
 * behind the apex the distance to the cone is underestimated. */
__device__ __forceinline__ bool cam_cone_sphere(V3 ctr, float rad, V3 ax, float ca, float sa, float znear, float zfar) {
  rad += 1e-3f;   /* slack for fp32 rounding of the frames: culling must never drop a visible geom */
  if (-ctr.z + rad < znear || -ctr.z - rad > zfar) return false;
  const float a = dot(ctr, ax);
  const V3 p = ctr - a * ax;
  return sqrtf(dot(p, p)) * ca - a * sa <= rad;
}

/* may robot geom `lane` (its camera-frame record g) show in the tile's view cone?  The robot and every ghost go through this and the three
 * helpers below (cast, normal, lights): a ghost posed like the robot then meets the compositor's strict t < t0 with equal bits */
template <class Mref>
__device__ __forceinline__ bool cam_rob_cull(const Mref& M, const CamCall& c, const float* g, const int lane, V3 ax, float ca, float sa) {
  V3 ctr = ld3(g + 9);
  float rad;
  if (lane < 4) rad = M.foot_radius[lane];
  else {
    const auto& G = M.lg[lane - 4];
    ctr = ctr + matvec(g, ld3(G.aabb_c));
    rad = sqrtf(G.aabb_h[0] * G.aabb_h[0] + G.aabb_h[1] * G.aabb_h[1] + G.aabb_h[2] * G.aabb_h[2]) + G.radius;
  }
  return cam_cone_sphere(ctr, rad, ax, ca, sa, c.znear, c.zfar);
}
/* the pixel ray d (camera frame) against robot geom g whose camera-frame record is gr: the entry parameter or -1; pg: the part (SHADE) */
template <bool SHADE, class Mref>
__device__ __forceinline__ float cam_rob_cast(const Mref& M, const CamCall& c, const float* gr, const int g, V3 d, int& pg) {
  const V3 t = ld3(gr + 9), o = (-1.0f) * matTvec(gr, t), dl = matTvec(gr, d);
  float th;
  if (g < 4) th = cam_sphere(o, dl, M.foot_radius[g]);
  else {
    const auto& G = M.lg[g - 4];
    const int pt = G.ptype;
    if (pt == 2) th = cam_sphere(o, dl, G.psize[0]);
    else if (pt == 3) th = cam_capsule(o, dl, G.psize[0], G.psize[1], pg);
    else if (pt == 5) th = cam_cylinder(o, dl, G.psize[0], G.psize[1], pg);
    else if (pt == 6) {
      const float ov[3] = {o.x, o.y, o.z}, dv[3] = {dl.x, dl.y, dl.z}, s[3] = {G.psize[0], G.psize[1], G.psize[2]};
      float tin = -1e30f, tout = 1e30f;
      th = ray_slab(ov, dv, s, tin, tout, SHADE ? &pg : nullptr) ? tin : -1.0f;
    } else {
      th = cam_hull(o, dl, c.planes + 4 * c.plane_adr[g - 4], c.plane_num[g - 4], pg);
      pg += c.plane_adr[g - 4];   /* the entry plane, as an index into c.planes */
    }
  }
  return th;
}

/* ---- shading (gq_camera_shaded): the winner's normal, its material and the lights, fp32 in the camera frame */
__device__ __forceinline__ uint32_t cam_byte(float x) { return (uint32_t)floorf(255.0f * fminf(fmaxf(x, 0.0f), 1.0f) + 0.5f); }
__device__ __forceinline__ V3 cam_unit(V3 a) { return (1.0f / sqrtf(dot(a, a))) * a; }
/* x^e for x in [0, 1], e >= 0 on the transcendental unit (v_log_f32 / v_exp_f32, as fast_pow_ratio; the library powf is hundreds of
 * instructions of special cases); 0^0 = 1 */
__device__ __forceinline__ float cam_pow(float x, float e) { return e > 0.0f ? __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)) : 1.0f; }

/* outward normal (camera frame, not unit) of robot geom `slot` (camera-frame record gr) at the ray parameter best, entered on `part` */
template <class Mref>
__device__ __forceinline__ V3 cam_rob_normal(const Mref& M, const CamCall& c, const float* gr, int slot, int part, V3 d, float best) {
  const V3 t = ld3(gr + 9), p = (-1.0f) * matTvec(gr, t) + best * matTvec(gr, d);
  V3 nl = p;   /* spheres */
  if (slot >= 4) {
    const auto& G = M.lg[slot - 4];
    const int pt = G.ptype;
    const float h = G.psize[1];
    if (pt == 3) nl = part == 0 ? v3(p.x, p.y, 0.0f) : p - v3(0.0f, 0.0f, part == 1 ? h : -h);
    else if (pt == 5) nl = part == 0 ? v3(p.x, p.y, 0.0f) : v3(0.0f, 0.0f, p.z > 0.0f ? 1.0f : -1.0f);
    else if (pt == 6) {
      const V3 dl = matTvec(gr, d);
      const float dk = part == 0 ? dl.x : part == 1 ? dl.y : dl.z, s = dk > 0.0f ? -1.0f : 1.0f;
      nl = v3(part == 0 ? s : 0.0f, part == 1 ? s : 0.0f, part == 2 ? s : 0.0f);
    } else if (pt != 2) nl = ld3(c.planes + 4 * part);
  }
  return matvec(gr, nl);
}

/* the lights at the hit best d with normal n (camera frame, not unit), base colour col, material (specular, shininess, emission):
 * out, unclamped */
__device__ __forceinline__ void cam_light(const CamShade& S, const float* Rc, const double* co, V3 n, const float* col, const float* mat, V3 d,
                                          float best, float* out) {
  n = cam_unit(n);
  const V3 v = (-1.0f) * cam_unit(d), ph = best * d;   /* towards the camera; the hit, camera frame */
  for (int k = 0; k < 3; k++) out[k] = mat[2] * col[k];
  const float shin = 128.0f * mat[1];
  for (int l = 0; l < S.nlight; l++) { /* wave-uniform: each light is taken into the camera frame once per wave */
    const CamLight& Lt = S.light[l];
    V3 L = v3(0.0f, 0.0f, 1.0f);
    float w = 1.0f;   /* attenuation x spot */
    if (Lt.kind == 1) L = (-1.0f) * matTvec(Rc, ld3(Lt.dir));
    else if (Lt.kind == 2) {
      const V3 lp = matTvec(Rc, v3((float)((double)Lt.pos[0] - co[0]), (float)((double)Lt.pos[1] - co[1]), (float)((double)Lt.pos[2] - co[2])));
      const V3 q = lp - ph;
      const float r = sqrtf(dot(q, q));
      L = (1.0f / r) * q;
      const float cs = -dot(L, matTvec(Rc, ld3(Lt.dir)));
      w = (cs >= Lt.cos_cut ? cam_pow(cs, Lt.expo) : 0.0f) / (Lt.att[0] + Lt.att[1] * r + Lt.att[2] * r * r);
    }
    const float nL = dot(n, L), nH = fmaxf(dot(n, cam_unit(L + v)), 0.0f);
    const float sp = nL > 0.0f ? mat[0] * cam_pow(nH, shin) : 0.0f, df = fmaxf(nL, 0.0f);
    for (int k = 0; k < 3; k++) out[k] += w * (Lt.amb[k] * col[k] + Lt.dif[k] * col[k] * df + Lt.spe[k] * sp);
  }
}

/* the opaque colour of a pixel, unclamped into out: the background, or the winner (id, slot, part) lit */
template <class Mref>
__device__ inline void cam_shade(const Mref& M, const CamCall& c, const CamShade& S, const float* rec, const float* Rc, const double* co, V3 d, V3 dw,
                                 float best, int id, int slot, int part, int nbox, float* out) {
  float col[3], mat[3];   /* base colour; specular, shininess, emission */
  V3 n;                   /* outward normal, camera frame (not unit) */
  if (id < 0) { /* background: the gradient over the world z of the unit ray */
    const float s = 0.5f * (1.0f + dw.z / sqrtf(dot(dw, dw)));
    for (int k = 0; k < 3; k++) out[k] = S.bottom[k] + (S.top[k] - S.bottom[k]) * s;
    return;
  }
  if (id < c.ngeom) { /* robot geom `slot` */
    n = cam_rob_normal(M, c, rec + 12 + 12 * slot, slot, part, d, best);
    const float* gm = S.geom_mat + 7 * id;
    col[0] = gm[0]; col[1] = gm[1]; col[2] = gm[2]; mat[0] = gm[4]; mat[1] = gm[5]; mat[2] = gm[6];
  } else {
    V3 nw = v3(0.0f, 0.0f, 1.0f);   /* the floor */
    const int b = id - c.ngeom - 1;
    if (b >= 0 && b < nbox) { /* world box: the entry face of slab `part` */
      const auto& B = M.box[slot];
      const V3 ax = v3(B.mat[part], B.mat[3 + part], B.mat[6 + part]);
      nw = dot(ax, dw) > 0.0f ? (-1.0f) * ax : ax;
      for (int k = 0; k < 3; k++) col[k] = S.box_mat[k];
      for (int k = 0; k < 3; k++) mat[k] = S.box_mat[4 + k];
    } else {
      if (b == nbox) { /* height-field triangle `slot` */
        const int nc = M.hf_ncol, cell = slot >> 1, r = cell / nc, cc = cell % nc;
        const float* Hf = M.hf_data;
        const float dx = M.hf_dx, dy = M.hf_dy;
        if (slot & 1) {
          const float h11 = Hf[(r + 1) * nc + cc + 1];
          nw = v3((Hf[(r + 1) * nc + cc] - h11) * dy, (Hf[r * nc + cc + 1] - h11) * dx, dx * dy);
        } else {
          const float h00 = Hf[r * nc + cc];
          nw = v3(-(Hf[r * nc + cc + 1] - h00) * dy, -(Hf[(r + 1) * nc + cc] - h00) * dx, dx * dy);
        }
      }
      /* the checker in world x / y: the fp64 origin reduced modulo two squares, then the fp32 ray */
      const double p2 = 2.0 * (double)S.square;
      const float ox = (float)(co[0] - p2 * floor(co[0] / p2)), oy = (float)(co[1] - p2 * floor(co[1] / p2));
      const float fx = (ox + best * dw.x) / S.square, fy = (oy + best * dw.y) / S.square, ix = floorf(fx), iy = floorf(fy);
      const float ux = fx - ix, uy = fy - iy;
      const float edge = fminf(fminf(ux, 1.0f - ux), fminf(uy, 1.0f - uy)) * S.square;
      const float* rgb = edge < S.mark_w ? S.mark_rgb : (((int)ix + (int)iy) & 1) ? S.rgb2 : S.rgb1;
      for (int k = 0; k < 3; k++) col[k] = rgb[k];
      for (int k = 0; k < 3; k++) mat[k] = S.floor_mat[k];
    }
    n = matTvec(Rc, nw);
  }
  cam_light(S, Rc, co, n, col, mat, d, best, out);
}

/* ---- layers (gq_camera_layered): ghost robots and markers, each at most one translucent layer per pixel */
/* the solid cone with base disc radius rb at z = zb and apex at z = zt > zb (axis z): entry parameter or -1; part 0 side, 1 base.  Within
 * the slab zb <= z <= zt the solid is {x^2 + y^2 <= k^2 (zt - z)^2}, k = rb / (zt - zb), a convex set, so its ray interval is the slab's
 * interval cut by the one piece of {f(t) <= 0} that meets it, f(t) = a t^2 + 2 b t + c. */
__device__ inline float cam_cone(V3 o, V3 d, float rb, float zb, float zt, int& part) {
  float lo = -1e30f, hi = 1e30f;
  part = 1;
  if (fabsf(d.z) < 1e-20f) { if (o.z < zb || o.z > zt) return -1.0f; }
  else {
    float t0 = (zb - o.z) / d.z, t1 = (zt - o.z) / d.z;
    if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
    lo = t0; hi = t1;
  }
  const float k = rb / (zt - zb), k2 = k * k, hz = zt - o.z;
  const float a = d.x * d.x + d.y * d.y - k2 * d.z * d.z, b = o.x * d.x + o.y * d.y + k2 * hz * d.z, cc = o.x * o.x + o.y * o.y - k2 * hz * hz;
  if (fabsf(a) <= 1e-7f * (d.x * d.x + d.y * d.y + k2 * d.z * d.z)) { /* parallel to a generator: 2 b t + c <= 0 */
    if (fabsf(b) < 1e-30f) { if (cc > 0.0f) return -1.0f; }
    else {
      const float r = -0.5f * cc / b;
      if (b > 0.0f) hi = fminf(hi, r);
      else if (r > lo) { lo = r; part = 0; }
    }
  } else {
    const float disc = b * b - a * cc;
    if (disc < 0.0f) { if (a > 0.0f) return -1.0f; }   /* a < 0: f <= 0 everywhere */
    else {
      const float s = sqrtf(disc), r0 = (-b - s) / a, r1 = (-b + s) / a, q0 = fminf(r0, r1), q1 = fmaxf(r0, r1);
      if (a > 0.0f) { /* inside between the roots */
        if (q0 > lo) { lo = q0; part = 0; }
        hi = fminf(hi, q1);
      } else if (lo <= q0) hi = fminf(hi, q0);   /* inside outside the roots: the piece that meets the slab */
      else if (q1 > lo) { lo = q1; part = 0; }
    }
  }
  return lo <= hi ? lo : -1.0f;
}

/* marker k of the env (wave-uniform row mk, world axes) in the camera frame: type, centre p (the base for capsules and arrows), unit axis u
 * with an orthonormal pair e1, e2, length len */
struct CamMarker {
  int type;
  V3 p, u, e1, e2;
  float len, r0, r1, head;
};
__device__ __forceinline__ CamMarker cam_marker(const float* mk, const float* Rc, const double* co) {
  CamMarker m;
  m.type = (int)mk[0];
  m.p = matTvec(Rc, v3((float)((double)mk[1] - co[0]), (float)((double)mk[2] - co[1]), (float)((double)mk[3] - co[2])));
  const V3 a = matTvec(Rc, v3(mk[4], mk[5], mk[6]));
  m.len = sqrtf(dot(a, a));
  m.u = m.len > 0.0f ? (1.0f / m.len) * a : v3(0.0f, 0.0f, 1.0f);
  const V3 t = fabsf(m.u.x) < 0.6f ? v3(1.0f, 0.0f, 0.0f) : v3(0.0f, 1.0f, 0.0f);
  m.e1 = cam_unit(t - dot(t, m.u) * m.u);
  m.e2 = v3(m.u.y * m.e1.z - m.u.z * m.e1.y, m.u.z * m.e1.x - m.u.x * m.e1.z, m.u.x * m.e1.y - m.u.y * m.e1.x);
  m.r0 = mk[7]; m.r1 = mk[8]; m.head = mk[9];
  if (m.type != 1 && !(m.len > 0.0f)) m.type = 0;   /* capsules and arrows of zero length are skipped */
  return m;
}
/* a bounding sphere of the marker (camera frame) */
__device__ __forceinline__ float cam_marker_bound(const CamMarker& m, V3& ctr) {
  if (m.type == 1) { ctr = m.p; return m.r0; }
  ctr = m.p + (0.5f * m.len) * m.u;
  return 0.5f * m.len + (m.type == 3 ? fmaxf(m.r0, m.r1) : m.r0);
}
/* the ray d (camera frame, from the camera) against the marker: entry parameter or -1, and the outward normal there (camera frame) */
__device__ inline float cam_marker_cast(const CamMarker& m, V3 d, V3& n) {
  if (m.type == 1) {
    const V3 o = (-1.0f) * m.p;
    const float t = cam_sphere(o, d, m.r0);
    n = o + t * d;
    return t;
  }
  const V3 ow = (-1.0f) * m.p;   /* the camera relative to the base, then in the marker frame (e1, e2, u) */
  const V3 o = v3(dot(ow, m.e1), dot(ow, m.e2), dot(ow, m.u)), dl = v3(dot(d, m.e1), dot(d, m.e2), dot(d, m.u));
  float t = -1.0f;
  V3 nl = v3(0.0f, 0.0f, 1.0f);
  int part = 0;
  if (m.type == 2) {
    const float h = 0.5f * m.len;
    const V3 oc = o - v3(0.0f, 0.0f, h);
    t = cam_capsule(oc, dl, m.r0, h, part);
    const V3 p = oc + t * dl;
    nl = part == 0 ? v3(p.x, p.y, 0.0f) : p - v3(0.0f, 0.0f, part == 1 ? h : -h);
  } else if (m.type == 3) { /* shaft: cylinder radius r0 over z in [0, zb]; head: cone of base radius r1 from zb to the tip */
    const float zb = (1.0f - m.head) * m.len, h = 0.5f * zb;
    const V3 oc = o - v3(0.0f, 0.0f, h);
    int ps = 0, pc = 0;
    const float ts = cam_cylinder(oc, dl, m.r0, h, ps), tc = cam_cone(o, dl, m.r1, zb, m.len, pc);
    if (ts >= 0.0f && (tc < 0.0f || ts <= tc)) {
      t = ts;
      const V3 p = oc + t * dl;
      nl = ps == 0 ? v3(p.x, p.y, 0.0f) : v3(0.0f, 0.0f, p.z > 0.0f ? 1.0f : -1.0f);
    } else if (tc >= 0.0f) {
      t = tc;
      const V3 p = o + t * dl;
      const float k = m.r1 / (m.len - zb);
      nl = pc == 0 ? v3(p.x, p.y, k * k * (m.len - p.z)) : v3(0.0f, 0.0f, -1.0f);
    }
  }
  n = nl.x * m.e1 + nl.y * m.e2 + nl.z * m.u;
  return t;
}

/* composite the ghosts and markers of env `env` over the opaque colour C (depth t0) of this lane's pixel.  Each layer is shaded when it
 * enters a depth-sorted list of GQ_CAM_NLAYER (t, rgb, a) entries held in registers (static indices only: the insertion is an unrolled
 * compare-and-swap chain); layers arrive in index order (ghosts, then markers) and a tie goes behind, so ties sort by index.  Empty
 * entries have a = 0, which leaves C exactly as it is. */
template <class Mref>
__device__ inline void cam_layers(const Mref& M, const CamCall& c, const CamShade& S, const CamLayers& L, const float* Rc, const double* co, V3 d,
                                  V3 ax, float ca, float sa, float t0, int env, float* C) {
  const int lane = lane_id(), nrob = 4 + M.nlg;
  float lt[GQ_CAM_NLAYER], lr[GQ_CAM_NLAYER], lg[GQ_CAM_NLAYER], lb[GQ_CAM_NLAYER], la[GQ_CAM_NLAYER];
#pragma unroll
  for (int k = 0; k < GQ_CAM_NLAYER; k++) { lt[k] = 3e38f; lr[k] = lg[k] = lb[k] = la[k] = 0.0f; }
  auto insert = [&](float t, float r, float g, float b, float a) {
#pragma unroll
    for (int k = 0; k < GQ_CAM_NLAYER; k++) {
      const bool s = t < lt[k];
      const float t1 = s ? lt[k] : t, r1 = s ? lr[k] : r, g1 = s ? lg[k] : g, b1 = s ? lb[k] : b, a1 = s ? la[k] : a;
      if (s) { lt[k] = t; lr[k] = r; lg[k] = g; lb[k] = b; la[k] = a; }
      t = t1; r = r1; g = g1; b = b1; a = a1;
    }
  };
  for (int gh = 0; gh < L.n_ghost; gh++) { /* wave-uniform */
    const size_t row = (size_t)env * L.n_ghost + gh;
    const float* grec = L.grec + row * GQ_CAM_GREC;
    bool near = false;
    if (lane < nrob) near = cam_rob_cull(M, c, grec + 12 * lane, lane, ax, ca, sa);
    float tg = t0;   /* the ghost's nearest hit in [znear, t0) */
    int sg = -1, pb = 0;
    for (uint64_t todo = ballot(near); todo; todo &= todo - 1) { /* wave-uniform */
      const int g = ffs64(todo);
      int pg = 0;
      const float th = cam_rob_cast<true>(M, c, grec + 12 * g, g, d, pg);
      if (th >= c.znear && th < tg) { tg = th; sg = g; pb = pg; }
    }
    if (sg >= 0) {
      const float* gm = S.geom_mat + 7 * M.item_geomid[sg];
      const float* rgb = L.ghost_rgb ? L.ghost_rgb + 3 * row : gm;
      const float col[3] = {rgb[0], rgb[1], rgb[2]}, mat[3] = {gm[4], gm[5], gm[6]};
      float o[3];
      cam_light(S, Rc, co, cam_rob_normal(M, c, grec + 12 * sg, sg, pb, d, tg), col, mat, d, tg, o);
      insert(tg, o[0], o[1], o[2], L.ghost_alpha[row]);
    }
  }
  if (L.n_marker > 0) {
    const float* mrow = L.markers + (size_t)env * L.n_marker * 16;
    bool near = false;
    if (lane < L.n_marker) {
      const CamMarker m = cam_marker(mrow + 16 * lane, Rc, co);
      V3 ctr;
      const float rad = cam_marker_bound(m, ctr);
      near = m.type >= 1 && m.type <= 3 && cam_cone_sphere(ctr, rad, ax, ca, sa, c.znear, c.zfar);
    }
    for (uint64_t todo = ballot(near); todo; todo &= todo - 1) { /* wave-uniform */
      const float* mk = mrow + 16 * ffs64(todo);
      const CamMarker m = cam_marker(mk, Rc, co);
      V3 n;
      const float th = cam_marker_cast(m, d, n);
      if (th >= c.znear && th < t0) {
        const float col[3] = {mk[10], mk[11], mk[12]}, mat[3] = {0.5f, 0.5f, 0.0f};
        float o[3];
        cam_light(S, Rc, co, n, col, mat, d, th, o);
        insert(th, o[0], o[1], o[2], mk[13]);
      }
    }
  }
#pragma unroll
  for (int k = GQ_CAM_NLAYER - 1; k >= 0; k--) { /* far to near */
    C[0] = la[k] * lr[k] + (1.0f - la[k]) * C[0];
    C[1] = la[k] * lg[k] + (1.0f - la[k]) * C[1];
    C[2] = la[k] * lb[k] + (1.0f - la[k]) * C[2];
  }
}

/* pixel pass: one wavefront renders tile `tile` of env `env`; SHADE: also its RGBA image (sh); LAYERS: ghosts and markers composited over
 * that image (ly, gq_camera_layered) */
template <bool SHADE, bool LAYERS = false, class Mref>
__device__ inline void camera_tile_wave(const Mref& M, const CamCall& c, const CamShade* sh, const int tile, const int env,
                                        const CamLayers* ly = nullptr) {
  const int lane = lane_id(), W = c.width, H = c.height;
  const int tiles_x = (W + GQ_CAM_TILE - 1) / GQ_CAM_TILE, tx = tile % tiles_x, ty = tile / tiles_x;
  const int row = ty * GQ_CAM_TILE + lane / GQ_CAM_TILE, col = tx * GQ_CAM_TILE + lane % GQ_CAM_TILE;
  const bool valid = row < H && col < W;
  const int r = row < H ? row : H - 1, cl = col < W ? col : W - 1;   /* lanes past the image edge mirror a pixel and do not store */
  const V3 d = v3((2.0f * ((float)cl + 0.5f) / (float)W - 1.0f) * c.tan_x, (1.0f - 2.0f * ((float)r + 0.5f) / (float)H) * c.tan_y, -1.0f);
  const float* rec = c.rec + (size_t)env * GQ_CAM_REC;
  float Rc[9];
  for (int k = 0; k < 9; k++) Rc[k] = rec[k];
  const double co[3] = {c.cpos[(size_t)env * 3], c.cpos[(size_t)env * 3 + 1], c.cpos[(size_t)env * 3 + 2]};
  /* the tile's view cone: axis through the tile centre, half angle to the farthest corner ray */
  const int c0 = tx * GQ_CAM_TILE, c1 = imin(c0 + GQ_CAM_TILE, W), r0 = ty * GQ_CAM_TILE, r1 = imin(r0 + GQ_CAM_TILE, H);
  const float xl = (2.0f * c0 / W - 1.0f) * c.tan_x, xh = (2.0f * c1 / W - 1.0f) * c.tan_x;
  const float yh = (1.0f - 2.0f * r0 / H) * c.tan_y, yl = (1.0f - 2.0f * r1 / H) * c.tan_y;
  V3 ax = v3(0.5f * (xl + xh), 0.5f * (yl + yh), -1.0f);
  ax = (1.0f / sqrtf(dot(ax, ax))) * ax;
  float ca = 1.0f;
  for (int k = 0; k < 4; k++) {
    const V3 q = v3(k & 1 ? xh : xl, k & 2 ? yh : yl, -1.0f);
    ca = fminf(ca, dot(q, ax) / sqrtf(dot(q, q)));
  }
  const float sa = sqrtf(fmaxf(0.0f, 1.0f - ca * ca));
  /* cull, lane = candidate */
  const int nrob = 4 + M.nlg, nbox = M.nbox;
  uint64_t rob = 0, box[2] = {0, 0};
  if (c.flags & 1) {
    bool near = false;
    if (lane < nrob) near = cam_rob_cull(M, c, rec + 12 + 12 * lane, lane, ax, ca, sa);
    rob = ballot(near);
  }
  if (c.flags & 2)
    for (int half = 0; half < 2 && half * GQ_WAVE < nbox; half++) { /* wave-uniform */
      const int b = half * GQ_WAVE + lane;
      bool near = false;
      if (b < nbox) {
        const V3 v = v3((float)((double)M.box[b].pos[0] - co[0]), (float)((double)M.box[b].pos[1] - co[1]), (float)((double)M.box[b].pos[2] - co[2]));
        near = cam_cone_sphere(matTvec(Rc, v), M.box[b].rad, ax, ca, sa, c.znear, c.zfar);
      }
      box[half] = ballot(near);
    }
  /* cast, lane = pixel.  The shaded pass also keeps what the winner is: slot (robot geom g / world box b / height-field triangle) and part
   * (the surface of the primitive the entry is on); its normal is formed once, after the walk.  The depth-only pass never reads them. */
  float best = c.zfar;
  int id = -1, slot = 0, part = 0;
  const V3 dw = matvec(Rc, d);   /* the ray in world axes */
  if (c.flags & 2) {
    if (dw.z < 0.0f && co[2] >= 0.0) { /* the floor: a one-sided plane, hit from above */
      const float t = (float)(-co[2] / (double)dw.z);
      if (t >= c.znear && t <= best) { best = t; id = c.ngeom; }
    }
    const float dv[3] = {dw.x, dw.y, dw.z};
    for (int half = 0; half < 2; half++)
      for (uint64_t todo = box[half]; todo; todo &= todo - 1) { /* wave-uniform */
        const int b = half * GQ_WAVE + ffs64(todo);
        const float rv[3] = {(float)(co[0] - (double)M.box[b].pos[0]), (float)(co[1] - (double)M.box[b].pos[1]), (float)(co[2] - (double)M.box[b].pos[2])};
        float tin = -1e30f, tout = 1e30f;
        int ax_in = 0;
        if (ray_box(M.box[b], rv, dv, tin, tout, SHADE ? &ax_in : nullptr) && tin >= c.znear && tin <= best) {
          best = tin; id = c.ngeom + 1 + b;
          if (SHADE) { slot = b; part = ax_in; }
        }
      }
    if (M.hf_nrow > 0) { /* fp64: the walk runs in the field's own coordinates */
      const double ol[3] = {co[0] - (double)M.hf_pos[0], co[1] - (double)M.hf_pos[1], co[2] - (double)M.hf_pos[2]}, dd[3] = {dw.x, dw.y, dw.z};
      int tri = 0;
      const double t = ray_hfield(M, ol, dd, (double)c.znear, SHADE ? &tri : nullptr);
      if (t >= 0.0 && t <= (double)best) {
        best = (float)t; id = c.ngeom + 1 + nbox;
        if (SHADE) slot = tri;
      }
    }
  }
  for (uint64_t todo = rob; todo; todo &= todo - 1) { /* wave-uniform */
    const int g = ffs64(todo);
    int pg = 0;
    const float th = cam_rob_cast<SHADE>(M, c, rec + 12 + 12 * g, g, d, pg);
    if (th >= c.znear && th <= best) {
      best = th; id = M.item_geomid[g];
      if (SHADE) { slot = g; part = pg; }
    }
  }
  const size_t px = ((size_t)env * H + row) * W + col;
  if (valid) {
    c.depth[px] = best;
    if (c.seg) c.seg[px] = id;
  }
  if constexpr (SHADE) {
    float rgb[3];
    cam_shade(M, c, *sh, rec, Rc, co, d, dw, best, id, slot, part, nbox, rgb);
    if constexpr (LAYERS) cam_layers(M, c, *sh, *ly, Rc, co, d, ax, ca, sa, best, env, rgb);
    const uint32_t rgba = cam_byte(rgb[0]) | cam_byte(rgb[1]) << 8 | cam_byte(rgb[2]) << 16 | 0xff000000u;
    if (valid) sh->rgba[px] = rgba;
  }
}

}  // namespace gq
