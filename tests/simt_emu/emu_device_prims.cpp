/* TEST INFRASTRUCTURE - the emulator shim's wave primitives and fast-math stand-ins (gq_device.h in this directory) and the kernel's small math
 * (csrc/gq_step_kernel.h, compiled against the shim) behind the entry points of tests/device_probe/probe.hip, on host memory: the same case
 * tables (tests/device_cases.py) pin the shim and the hardware to the same float64 references.  The Newton solver's routines (csrc/gq_newton.h,
 * tests/newton_cases.py) run through the bodies of tests/device_probe/newton_probe.h, the ones the probe launches. */
#include <functional>
#include "gq_device.h"
#include "gq_step_kernel.h"
#include "newton_probe.h"

void emu_run_wave(unsigned block, unsigned nblocks, const std::function<void()>& body);

template <class F> static int waves(int npat, F&& f) {
  for (int b = 0; b < npat; b++) emu_run_wave((unsigned)b, (unsigned)npat, [&]() { f(b * 64 + gq::lane_id(), b, gq::lane_id()); });
  return 0;
}
static int as_int(float v) { int i; memcpy(&i, &v, 4); return i; }

extern "C" int emu_wave_reduce(const float* in, int npat, float* sum, float* mn, float* mx, float* qsum) {
  return waves(npat, [&](int i, int, int) { const float v = in[i]; sum[i] = gq::wave_sum(v); mn[i] = gq::wave_min(v); mx[i] = gq::wave_max(v); qsum[i] = gq::quad_sum(v); });
}
extern "C" int emu_wave_scan(const int32_t* in, int npat, int32_t* out) {
  return waves(npat, [&](int i, int, int) { out[i] = gq::wave_incl_scan(in[i]); });
}
extern "C" int emu_bcast(const float* in, const int32_t* src, int npat, float* outf, int32_t* outi) {
  return waves(npat, [&](int i, int b, int) { const float v = in[i]; outf[i] = gq::bcast(v, src[b]); outi[i] = gq::bcast(as_int(v), src[b]); });
}
extern "C" int emu_readlane(const float* in, int npat, float* out) {
  return waves(npat, [&](int i, int b, int l) {
    const float v = in[i];
    float* o = out + (size_t)b * 5 * 64 + l;
    o[0] = gq::readlane<0>(v); o[64] = gq::readlane<15>(v); o[128] = gq::readlane<31>(v); o[192] = gq::readlane<47>(v); o[256] = gq::readlane<63>(v);
  });
}
extern "C" int emu_shfl_xor(const float* in, int npat, float* out, int32_t* outi) {
  static const int M[8] = {1, 2, 4, 8, 16, 32, 17, 63};
  return waves(npat, [&](int i, int b, int l) {
    const float v = in[i];
    for (int k = 0; k < 8; k++) { out[((size_t)b * 8 + k) * 64 + l] = gq::shfl_xor(v, M[k]); outi[((size_t)b * 8 + k) * 64 + l] = gq::shfl_xor(as_int(v), M[k]); }
  });
}
extern "C" int emu_shfl_idx(const float* in, const int32_t* idx, int npat, float* outf, int32_t* outi) {
  return waves(npat, [&](int i, int, int) { const float v = in[i]; outf[i] = gq::shfl_idx(v, idx[i] & 63); outi[i] = gq::shfl_idx(as_int(v), idx[i] & 63); });
}
extern "C" int emu_ballot(const int32_t* pred, int npat, uint64_t* mask, int32_t* popc, int32_t* ffs) {
  return waves(npat, [&](int i, int, int) { const uint64_t m = gq::ballot(pred[i] != 0); mask[i] = m; popc[i] = gq::popc64(m); ffs[i] = gq::ffs64(m); });
}

extern "C" int emu_bits(const uint64_t* m, int n, int32_t* popc, int32_t* ffs) {
  for (int i = 0; i < n; i++) { popc[i] = gq::popc64(m[i]); ffs[i] = gq::ffs64(m[i]); }
  return 0;
}
extern "C" int emu_unary(const float* x, int n, float* out) {
  for (int i = 0; i < n; i++) { out[i] = gq::fast_rcp(x[i]); out[n + i] = gq::fast_sqrt(x[i]); out[2 * (size_t)n + i] = gq::fast_rsqrt(x[i]); out[3 * (size_t)n + i] = gq::fast_cos_turns(x[i]); }
  return 0;
}
extern "C" int emu_fdiv(const float* a, const float* b, int n, float* out) { for (int i = 0; i < n; i++) out[i] = gq::fdiv(a[i], b[i]); return 0; }
extern "C" int emu_med3(const float* x, const float* lo, const float* hi, int n, float* out) { for (int i = 0; i < n; i++) out[i] = gq::med3(x[i], lo[i], hi[i]); return 0; }
extern "C" int emu_atan2(const float* y, const float* x, int n, float* out) { for (int i = 0; i < n; i++) out[i] = gq::atan2_fast(y[i], x[i]); return 0; }
extern "C" int emu_sincos(const float* x, int n, float* s, float* c) { for (int i = 0; i < n; i++) gq::sincos_small(x[i], s[i], c[i]); return 0; }
extern "C" int emu_pow_ratio(const float* a, const float* p, const float* b, const float* q, int n, float* out) {
  for (int i = 0; i < n; i++) out[i] = gq::fast_pow_ratio(a[i], p[i], b[i], q[i]);
  return 0;
}
extern "C" int emu_impedance(const float* solimp, const float* pos, const float* margin, int n, float* out) {
  for (int i = 0; i < n; i++) out[i] = gq::impedance(solimp + 5 * (size_t)i, pos[i], margin[i]);
  return 0;
}
extern "C" int emu_qnormalize(const float* q, int n, float* out) {
  for (int i = 0; i < n; i++) {
    gq::Q4 a = {q[4 * (size_t)i], q[4 * (size_t)i + 1], q[4 * (size_t)i + 2], q[4 * (size_t)i + 3]};
    a = gq::qnormalize(a);
    out[4 * (size_t)i] = a.w; out[4 * (size_t)i + 1] = a.x; out[4 * (size_t)i + 2] = a.y; out[4 * (size_t)i + 3] = a.z;
  }
  return 0;
}
extern "C" int emu_philox(const uint32_t* ck, int n, uint32_t* words, float* normal) {
  for (int i = 0; i < n; i++) {
    const uint32_t* c = ck + 6 * (size_t)i;
    for (int w = 0; w < 4; w++) words[4 * (size_t)i + w] = gq::philox4x32(c[0], c[1], c[2], c[3], c[4], c[5], w);
    normal[i] = gq::philox_normal(c[0], c[1], c[2], c[3], c[4], c[5]);
  }
  return 0;
}

/* ------------------------------------------------------------------ csrc/gq_newton.h (argument layouts: tests/device_probe/newton_probe.h) */
extern "C" int emu_newton_solve(int mode, const float* Sc, const float* Sb, const float* damping, float hd, const float* rhs, const float* rhs2, int nsys, int nrhs, int alias,
                                float* out, float* out2, int32_t* touched) {
  if (mode < 0 || mode > 3) return -1;
  if (nrhs <= 0) return 0;
  return waves(nsys, [&](int, int b, int l) {
    if (mode == 0) nprobe::np_solve<0>(b, l, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
    else if (mode == 1) nprobe::np_solve<1>(b, l, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
    else if (mode == 2) nprobe::np_solve<2>(b, l, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
    else nprobe::np_solve<3>(b, l, Sc, Sb, damping, hd, rhs, rhs2, nrhs, alias, out, out2, touched);
  });
}
extern "C" int emu_newton_dense(const float* Hc, const float* Hb, const float* J, const float* w, const int32_t* r01, const float* rhs, int nsys, int nrhs, int alias,
                                float* out, int32_t* touched) {
  if (nrhs <= 0) return 0;
  return waves(nsys, [&](int, int b, int l) { nprobe::np_dense(b, l, Hc, Hb, J, w, r01, rhs, nrhs, alias, out, touched); });
}
extern "C" int emu_newton_rows(const int32_t* rtype, const float* in, int n, float* out, int32_t* piece) {
  for (int i = 0; i < n; i++) nprobe::np_rows(i, n, rtype, in, out, piece);
  return 0;
}
extern "C" int emu_newton_ell(const int32_t* code, const int32_t* r0, const float* par, const float* alpha, int npat, int na, float* st, float* dd) {
  return waves(npat, [&](int, int b, int l) { nprobe::np_ell(b, l, code, r0, par, alpha, na, st, dd); });
}
