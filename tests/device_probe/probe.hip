/* TEST INFRASTRUCTURE - calls the product's device routines one by one on the GPU (tests/test_gpu_device_probe.py).
 *
 * Built with the product's own device flags (csrc/Makefile print-flags) against the product's headers, so what runs here is what the step
 * kernels inline: the DPP ladders and permutes of csrc/gq_device.h, its transcendental-unit shortcuts, the hand-written small math and the
 * tree factor / solve of csrc/gq_step_kernel.h, the contact routines of csrc/gq_pairs.h and csrc/gq_convex.h, and the Newton solver's solves,
 * row laws and elliptic routines of csrc/gq_newton.h (bodies in newton_probe.h, shared with the emulator).  The host emulator
 * (tests/simt_emu) shadows gq_device.h and compiles with g++, so none of this is reached by the CPU suite.
 *
 * Every entry point takes device pointers and a case count, launches once with 64-thread blocks on the null stream, synchronises and returns
 * the HIP error code.  Wave kernels: block = one 64-value pattern.  Lane kernels: lane = case, guarded by the count.  The product never builds
 * or loads this. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gq_step_kernel.h"
#include "gq_pairs.h"
#include "gq_convex.h"
#include "newton_probe.h"
#include "hfield_probe.h"
#include <cstring>
#include <vector>

#define PROBE_K __global__ void __launch_bounds__(64)

static int probe_done() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}
static int probe_blocks(int n) { return (n + 63) / 64; }

/* ------------------------------------------------------------------ wave primitives: block = pattern */
PROBE_K k_wave_reduce(const float* in, float* sum, float* mn, float* mx, float* qsum) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const float v = in[i];
  sum[i] = gq::wave_sum(v); mn[i] = gq::wave_min(v); mx[i] = gq::wave_max(v); qsum[i] = gq::quad_sum(v);
}
PROBE_K k_wave_scan(const int32_t* in, int32_t* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  out[i] = gq::wave_incl_scan(in[i]);
}
/* src[block]: the wave-uniform source lane; outf / outi: the float and the int overload */
PROBE_K k_bcast(const float* in, const int32_t* src, float* outf, int32_t* outi) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int s = gq::uniform(src[blockIdx.x]);
  const float v = in[i];
  outf[i] = gq::bcast(v, s);
  outi[i] = gq::bcast(__float_as_int(v), s);
}
/* out[block][5][64]: readlane<0, 15, 31, 47, 63> */
PROBE_K k_readlane(const float* in, float* out) {
  const int l = threadIdx.x;
  const float v = in[blockIdx.x * 64 + l];
  float* o = out + (size_t)blockIdx.x * 5 * 64 + l;
  o[0] = gq::readlane<0>(v); o[64] = gq::readlane<15>(v); o[128] = gq::readlane<31>(v); o[192] = gq::readlane<47>(v); o[256] = gq::readlane<63>(v);
}
/* out[block][8][64]: m = 1, 2, 4, 8, 16, 32, 17, 63 (float overload); outi: the same through the int overload */
PROBE_K k_shfl_xor(const float* in, float* out, int32_t* outi) {
  const int l = threadIdx.x;
  const float v = in[blockIdx.x * 64 + l];
  const int iv = __float_as_int(v);
  float* o = out + (size_t)blockIdx.x * 8 * 64 + l;
  int32_t* oi = outi + (size_t)blockIdx.x * 8 * 64 + l;
  o[0] = gq::shfl_xor(v, 1); o[64] = gq::shfl_xor(v, 2); o[128] = gq::shfl_xor(v, 4); o[192] = gq::shfl_xor(v, 8);
  o[256] = gq::shfl_xor(v, 16); o[320] = gq::shfl_xor(v, 32); o[384] = gq::shfl_xor(v, 17); o[448] = gq::shfl_xor(v, 63);
  oi[0] = gq::shfl_xor(iv, 1); oi[64] = gq::shfl_xor(iv, 2); oi[128] = gq::shfl_xor(iv, 4); oi[192] = gq::shfl_xor(iv, 8);
  oi[256] = gq::shfl_xor(iv, 16); oi[320] = gq::shfl_xor(iv, 32); oi[384] = gq::shfl_xor(iv, 17); oi[448] = gq::shfl_xor(iv, 63);
}
/* idx[block][64]: per-lane source lanes in 0..63 */
PROBE_K k_shfl_idx(const float* in, const int32_t* idx, float* outf, int32_t* outi) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const float v = in[i];
  const int s = idx[i] & 63;
  outf[i] = gq::shfl_idx(v, s);
  outi[i] = gq::shfl_idx(__float_as_int(v), s);
}
/* the mask as every lane sees it, its population count and its lowest set bit */
PROBE_K k_ballot(const int32_t* pred, uint64_t* mask, int32_t* popc, int32_t* ffs) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const uint64_t m = gq::ballot(pred[i] != 0);
  mask[i] = m; popc[i] = gq::popc64(m); ffs[i] = gq::ffs64(m);
}

extern "C" int probe_wave_reduce(const float* in, int npat, float* sum, float* mn, float* mx, float* qsum) {
  hipLaunchKernelGGL(k_wave_reduce, dim3(npat), dim3(64), 0, 0, in, sum, mn, mx, qsum); return probe_done();
}
extern "C" int probe_wave_scan(const int32_t* in, int npat, int32_t* out) {
  hipLaunchKernelGGL(k_wave_scan, dim3(npat), dim3(64), 0, 0, in, out); return probe_done();
}
extern "C" int probe_bcast(const float* in, const int32_t* src, int npat, float* outf, int32_t* outi) {
  hipLaunchKernelGGL(k_bcast, dim3(npat), dim3(64), 0, 0, in, src, outf, outi); return probe_done();
}
extern "C" int probe_readlane(const float* in, int npat, float* out) {
  hipLaunchKernelGGL(k_readlane, dim3(npat), dim3(64), 0, 0, in, out); return probe_done();
}
extern "C" int probe_shfl_xor(const float* in, int npat, float* out, int32_t* outi) {
  hipLaunchKernelGGL(k_shfl_xor, dim3(npat), dim3(64), 0, 0, in, out, outi); return probe_done();
}
extern "C" int probe_shfl_idx(const float* in, const int32_t* idx, int npat, float* outf, int32_t* outi) {
  hipLaunchKernelGGL(k_shfl_idx, dim3(npat), dim3(64), 0, 0, in, idx, outf, outi); return probe_done();
}
extern "C" int probe_ballot(const int32_t* pred, int npat, uint64_t* mask, int32_t* popc, int32_t* ffs) {
  hipLaunchKernelGGL(k_ballot, dim3(npat), dim3(64), 0, 0, pred, mask, popc, ffs); return probe_done();
}

/* ------------------------------------------------------------------ scalar math: lane = argument */
PROBE_K k_bits(const uint64_t* m, int n, int32_t* popc, int32_t* ffs) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) { popc[i] = gq::popc64(m[i]); ffs[i] = gq::ffs64(m[i]); }
}
/* out[4][n]: fast_rcp, fast_sqrt, fast_rsqrt, fast_cos_turns of x */
PROBE_K k_unary(const float* x, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    out[i] = gq::fast_rcp(v); out[n + i] = gq::fast_sqrt(v); out[2 * (size_t)n + i] = gq::fast_rsqrt(v); out[3 * (size_t)n + i] = gq::fast_cos_turns(v);
  }
}
PROBE_K k_fdiv(const float* a, const float* b, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = gq::fdiv(a[i], b[i]);
}
PROBE_K k_med3(const float* x, const float* lo, const float* hi, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = gq::med3(x[i], lo[i], hi[i]);
}
PROBE_K k_atan2(const float* y, const float* x, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = gq::atan2_fast(y[i], x[i]);
}
PROBE_K k_sincos(const float* x, int n, float* s, float* c) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) { float ss, cc; gq::sincos_small(x[i], ss, cc); s[i] = ss; c[i] = cc; }
}
PROBE_K k_pow_ratio(const float* a, const float* p, const float* b, const float* q, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = gq::fast_pow_ratio(a[i], p[i], b[i], q[i]);
}
/* solimp[n][5] */
PROBE_K k_impedance(const float* solimp, const float* pos, const float* margin, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    float s[5];
#pragma unroll
    for (int k = 0; k < 5; k++) s[k] = solimp[5 * (size_t)i + k];
    out[i] = gq::impedance(s, pos[i], margin[i]);
  }
}
/* q, out: [n][4] (w, x, y, z) */
PROBE_K k_qnormalize(const float* q, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    gq::Q4 a = {q[4 * (size_t)i], q[4 * (size_t)i + 1], q[4 * (size_t)i + 2], q[4 * (size_t)i + 3]};
    a = gq::qnormalize(a);
    out[4 * (size_t)i] = a.w; out[4 * (size_t)i + 1] = a.x; out[4 * (size_t)i + 2] = a.y; out[4 * (size_t)i + 3] = a.z;
  }
}
/* ck[n][6]: counter words 0-3, key words 0-1; words[n][4]: the block; normal[n]: philox_normal of it */
PROBE_K k_philox(const uint32_t* ck, int n, uint32_t* words, float* normal) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    const uint32_t* c = ck + 6 * (size_t)i;
#pragma unroll
    for (int w = 0; w < 4; w++) words[4 * (size_t)i + w] = gq::philox4x32(c[0], c[1], c[2], c[3], c[4], c[5], w);
    normal[i] = gq::philox_normal(c[0], c[1], c[2], c[3], c[4], c[5]);
  }
}

#define PROBE_LANES(kernel, n, ...) do { if ((n) > 0) hipLaunchKernelGGL(kernel, dim3(probe_blocks(n)), dim3(64), 0, 0, __VA_ARGS__); return probe_done(); } while (0)
extern "C" int probe_bits(const uint64_t* m, int n, int32_t* popc, int32_t* ffs) { PROBE_LANES(k_bits, n, m, n, popc, ffs); }
extern "C" int probe_unary(const float* x, int n, float* out) { PROBE_LANES(k_unary, n, x, n, out); }
extern "C" int probe_fdiv(const float* a, const float* b, int n, float* out) { PROBE_LANES(k_fdiv, n, a, b, n, out); }
extern "C" int probe_med3(const float* x, const float* lo, const float* hi, int n, float* out) { PROBE_LANES(k_med3, n, x, lo, hi, n, out); }
extern "C" int probe_atan2(const float* y, const float* x, int n, float* out) { PROBE_LANES(k_atan2, n, y, x, n, out); }
extern "C" int probe_sincos(const float* x, int n, float* s, float* c) { PROBE_LANES(k_sincos, n, x, n, s, c); }
extern "C" int probe_pow_ratio(const float* a, const float* p, const float* b, const float* q, int n, float* out) { PROBE_LANES(k_pow_ratio, n, a, p, b, q, n, out); }
extern "C" int probe_impedance(const float* solimp, const float* pos, const float* margin, int n, float* out) { PROBE_LANES(k_impedance, n, solimp, pos, margin, n, out); }
extern "C" int probe_qnormalize(const float* q, int n, float* out) { PROBE_LANES(k_qnormalize, n, q, n, out); }
extern "C" int probe_philox(const uint32_t* ck, int n, uint32_t* words, float* normal) { PROBE_LANES(k_philox, n, ck, n, words, normal); }

/* ------------------------------------------------------------------ factor_tree_both + solve_tree: block = system, lane = right-hand side
 * Mc[nsys][12][9], Mb[nsys][6][6] (the kernel's tree-sparse storage of M), damping[nsys][18], rhs[nsys][64][18];
 * x0 / x1 [nsys][64][18]: M^-1 rhs and (M + h diag(damping))^-1 rhs */
PROBE_K k_tree(const float* Mc, const float* Mb, const float* damping, float h, const float* rhs, float* x0, float* x1) {
  __shared__ gq::WaveMem W;
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int k = lane; k < GQ_NJ * 9; k += 64) (&W.Mc[0][0])[k] = Mc[(size_t)b * GQ_NJ * 9 + k];
  if (lane < 36) (&W.Mb[0][0])[lane] = Mb[(size_t)b * 36 + lane];
  gq::wave_barrier();
  gq::factor_tree_both(W, (const GQ_MODEL float*)(damping + (size_t)b * GQ_NVD), h);
  const float* r = rhs + ((size_t)b * 64 + lane) * GQ_NVD;
  float x[GQ_NVD], y[GQ_NVD];
#pragma unroll
  for (int k = 0; k < GQ_NVD; k++) x[k] = y[k] = r[k];
  gq::solve_tree(W, 0, x);
  gq::solve_tree(W, 1, y);
  float* o0 = x0 + ((size_t)b * 64 + lane) * GQ_NVD;
  float* o1 = x1 + ((size_t)b * 64 + lane) * GQ_NVD;
#pragma unroll
  for (int k = 0; k < GQ_NVD; k++) { o0[k] = x[k]; o1[k] = y[k]; }
}
extern "C" int probe_tree(const float* Mc, const float* Mb, const float* damping, float h, const float* rhs, int nsys, float* x0, float* x1) {
  if (nsys > 0) hipLaunchKernelGGL(k_tree, dim3(nsys), dim3(64), 0, 0, Mc, Mb, damping, h, rhs, x0, x1);
  return probe_done();
}

/* ------------------------------------------------------------------ contact routines
 * pair routines: lane = case.  capsule_box in[n][22]: p0 3, p1 3, r, bc 3, bR 9, bh 3; box_box in[n][30]: ca 3, Ra 9, ha 3, cb 3, Rb 9, hb 3.  cnt[n]: contacts, out[n][4][7]: dist, pos, normal per contact (the layout of the
 * emulator's emu_capsule_box / emu_box_box); slots past the count are left untouched */
#define PROBE_CAP_IN 22
#define PROBE_BOX_IN 30
__device__ static void probe_store_hit(const gq::PairHit& H, int32_t* cnt, float* out) {
  *cnt = H.n;
  for (int q = 0; q < 4; q++)
    if (q < H.n) {
      const gq::V3 nn = gq::hit_nrm(H, q);
      out[7 * q] = H.dist[q]; out[7 * q + 1] = H.pos[q].x; out[7 * q + 2] = H.pos[q].y; out[7 * q + 3] = H.pos[q].z;
      out[7 * q + 4] = nn.x; out[7 * q + 5] = nn.y; out[7 * q + 6] = nn.z;
    }
}
PROBE_K k_capsule_box(const float* in, float margin, int n, int32_t* cnt, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* a = in + (size_t)i * PROBE_CAP_IN;
  float R[9];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = a[10 + k];
  gq::PairHit H;
  gq::capsule_box(gq::v3(a[0], a[1], a[2]), gq::v3(a[3], a[4], a[5]), a[6], gq::v3(a[7], a[8], a[9]), R, gq::v3(a[19], a[20], a[21]), margin, H);
  probe_store_hit(H, cnt + i, out + (size_t)i * 28);
}
PROBE_K k_box_box(const float* in, float margin, int n, int32_t* cnt, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* a = in + (size_t)i * PROBE_BOX_IN;
  float Ra[9], Rb[9];
#pragma unroll
  for (int k = 0; k < 9; k++) { Ra[k] = a[3 + k]; Rb[k] = a[18 + k]; }
  gq::PairHit H;
  gq::box_box(gq::v3(a[0], a[1], a[2]), Ra, gq::v3(a[12], a[13], a[14]), gq::v3(a[15], a[16], a[17]), Rb, gq::v3(a[27], a[28], a[29]), margin, H);
  probe_store_hit(H, cnt + i, out + (size_t)i * 28);
}
extern "C" int probe_capsule_box(const float* in, float margin, int n, int32_t* cnt, float* out) { PROBE_LANES(k_capsule_box, n, in, margin, n, cnt, out); }
extern "C" int probe_box_box(const float* in, float margin, int n, int32_t* cnt, float* out) { PROBE_LANES(k_box_box, n, in, margin, n, cnt, out); }

/* cvx_pair_wave: block = pair.  desc[npair][2][20]: the words of the two CvxShape in field order (kind, adr, num, pm as int32; R 9, t 3, h 3, r
 * as floats); adr + num of a cloud lies inside the vertex arrays (the caller's business; the routine clamps its chunk loads to adr + num - 1).
 * hit[npair], out[npair][7]: dist, pos, normal (the layout of the emulator's emu_convex), written where the pair was hit */
PROBE_K k_convex(const float* vx, const float* vy, const float* vz, const float* desc, float margin, int32_t* hit, float* out) {
  __shared__ float shp[GQ_CVX_SHP_WORDS], poly[GQ_CVX_POLY_WORDS];
  const int b = blockIdx.x;
  gq::CvxShape S[2];
  for (int s = 0; s < 2; s++) {
    const float* d = desc + ((size_t)b * 2 + s) * GQ_CVX_SHAPE_WORDS;
    const int32_t* di = reinterpret_cast<const int32_t*>(d);
    S[s].kind = di[0]; S[s].adr = di[1]; S[s].num = di[2]; S[s].pm = di[3];
    for (int k = 0; k < 9; k++) S[s].R[k] = d[4 + k];
    S[s].t = gq::v3(d[13], d[14], d[15]); S[s].h = gq::v3(d[16], d[17], d[18]); S[s].r = d[19];
  }
  gq::cvx_shape_store((gq::LdsF)shp, S[0]); gq::cvx_shape_store((gq::LdsF)(shp + GQ_CVX_SHAPE_WORDS), S[1]);
  gq::wave_barrier();
  const bool h = gq::cvx_pair_wave((gq::LdsF)shp, (gq::LdsF)poly, (const GQ_MODEL float*)vx, (const GQ_MODEL float*)vy, (const GQ_MODEL float*)vz, margin);
  gq::wave_barrier();
  if (threadIdx.x == 0) {
    hit[b] = h ? 1 : 0;
    if (h) {
      const float* o = shp + 2 * GQ_CVX_SHAPE_WORDS;
      float* w = out + (size_t)b * 7;
      w[0] = o[0]; w[1] = o[4]; w[2] = o[5]; w[3] = o[6]; w[4] = o[1]; w[5] = o[2]; w[6] = o[3];
    }
  }
}
extern "C" int probe_convex(const float* vx, const float* vy, const float* vz, const float* desc, float margin, int npair, int32_t* hit, float* out) {
  if (npair > 0) hipLaunchKernelGGL(k_convex, dim3(npair), dim3(64), 0, 0, vx, vy, vz, desc, margin, hit, out);
  return probe_done();
}

/* ------------------------------------------------------------------ csrc/gq_boxes.h, the height field: lane = case; the bodies and the argument
 * layouts are in hfield_probe.h.  probe_sphere_hfield builds the model on the host from the grid's description (grid [8], raw [nrow][ncol]:
 * device memory like every argument, copied back), uploads it with the elevations, launches once and frees both. */
PROBE_K k_closest_on_triangle(const float* in, int n, float* out, int32_t* interior) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) hfprobe::hfp_triangle_case(i, in, out, interior);
}
PROBE_K k_sphere_hfield(const GqDevModel* M, const double* base, const float* q, int n, int32_t* hit, float* out, float* under) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) hfprobe::hfp_sphere_case(i, *gq::mptr(M), base, q, hit, out, under);
}
extern "C" int probe_closest_on_triangle(const float* in, int n, float* out, int32_t* interior) { PROBE_LANES(k_closest_on_triangle, n, in, n, out, interior); }
extern "C" int probe_sphere_hfield(const double* grid, const float* raw, const double* base, const float* q, int n, int32_t* hit, float* out, float* under) {
  double g[8];
  hipError_t e = hipMemcpy(g, grid, sizeof g, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  const int nr = (int)g[0], nc = (int)g[1];
  if (nr < 2 || nc < 2 || nr > 4096 || nc > 4096) return -1;
  std::vector<float> rawh((size_t)nr * nc), heights;
  e = hipMemcpy(rawh.data(), raw, rawh.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  static GqDevModel M; /* large: not on the stack */
  memset(&M, 0, sizeof M);
  hfprobe::hfp_fill(M, g, rawh.data(), heights);
  float* dH = nullptr;
  GqDevModel* dM = nullptr;
  e = hipMalloc(&dH, heights.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&dM, sizeof M);
  if (e == hipSuccess) e = hipMemcpy(dH, heights.data(), heights.size() * sizeof(float), hipMemcpyHostToDevice);
  M.hf_data = dH;
  if (e == hipSuccess) e = hipMemcpy(dM, &M, sizeof M, hipMemcpyHostToDevice);
  int rc = (int)e;
  if (e == hipSuccess) {
    if (n > 0) hipLaunchKernelGGL(k_sphere_hfield, dim3(probe_blocks(n)), dim3(64), 0, 0, dM, base, q, n, hit, out, under);
    rc = probe_done();
  }
  if (dM) hipFree(dM);
  if (dH) hipFree(dH);
  return rc;
}

/* ------------------------------------------------------------------ csrc/gq_newton.h: the bodies and the argument layouts are in newton_probe.h */
template <int MODE> PROBE_K k_newton_solve(const float* Sc, const float* Sb, const float* damping, float hd, const float* rhs, const float* rhs2, int nrhs, int alias,
                                           float* out, float* out2, int32_t* touched) {
  nprobe::np_solve<MODE>(blockIdx.x, threadIdx.x, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
}
PROBE_K k_newton_dense(const float* Hc, const float* Hb, const float* J, const float* w, const int32_t* r01, const float* rhs, int nrhs, int alias, float* out, int32_t* touched) {
  nprobe::np_dense(blockIdx.x, threadIdx.x, Hc, Hb, J, w, r01, rhs, nrhs, alias, out, touched);
}
PROBE_K k_newton_rows(const int32_t* rtype, const float* in, int n, float* out, int32_t* piece) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) nprobe::np_rows(i, n, rtype, in, out, piece);
}
PROBE_K k_newton_ell(const int32_t* code, const int32_t* r0, const float* par, const float* alpha, int na, float* st, float* dd) {
  nprobe::np_ell(blockIdx.x, threadIdx.x, code, r0, par, alpha, na, st, dd);
}
extern "C" int probe_newton_solve(int mode, const float* Sc, const float* Sb, const float* damping, float hd, const float* rhs, const float* rhs2, int nsys, int nrhs, int alias,
                                  float* out, float* out2, int32_t* touched) {
  if (mode < 0 || mode > 3) return -1;
  if (nsys > 0 && nrhs > 0) {
    if (mode == 0) hipLaunchKernelGGL(k_newton_solve<0>, dim3(nsys), dim3(64), 0, 0, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
    if (mode == 1) hipLaunchKernelGGL(k_newton_solve<1>, dim3(nsys), dim3(64), 0, 0, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
    if (mode == 2) hipLaunchKernelGGL(k_newton_solve<2>, dim3(nsys), dim3(64), 0, 0, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
    if (mode == 3) hipLaunchKernelGGL(k_newton_solve<3>, dim3(nsys), dim3(64), 0, 0, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
  }
  return probe_done();
}
extern "C" int probe_newton_dense(const float* Hc, const float* Hb, const float* J, const float* w, const int32_t* r01, const float* rhs, int nsys, int nrhs, int alias,
                                  float* out, int32_t* touched) {
  if (nsys > 0 && nrhs > 0) hipLaunchKernelGGL(k_newton_dense, dim3(nsys), dim3(64), 0, 0, Hc, Hb, J, w, r01, rhs, nrhs, alias, out, touched);
  return probe_done();
}
extern "C" int probe_newton_rows(const int32_t* rtype, const float* in, int n, float* out, int32_t* piece) { PROBE_LANES(k_newton_rows, n, rtype, in, n, out, piece); }
extern "C" int probe_newton_ell(const int32_t* code, const int32_t* r0, const float* par, const float* alpha, int npat, int na, float* st, float* dd) {
  if (npat > 0) hipLaunchKernelGGL(k_newton_ell, dim3(npat), dim3(64), 0, 0, code, r0, par, alpha, na, st, dd);
  return probe_done();
}
