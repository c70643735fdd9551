/* TEST INFRASTRUCTURE - the bodies of the Newton-solver entry points, shared by tests/device_probe/probe.hip (hipcc, the product's flags and
 * headers) and tests/simt_emu/emu_device_prims.cpp (g++, the emulator's shim): one copy of the staging, the canaries and the call sequences, so
 * that both backends of tests/newton_cases.py run the same thing around csrc/gq_newton.h's routines.  Every body is called by all 64 lanes of
 * one wave (block = system / pattern) except np_rows (lane = case). */
#pragma once
#include "gq_newton.h"

namespace nprobe {

#define NP_CANARY 0x7fc0beef  /* a quiet NaN: an output left unwritten fails every comparison, a guard word is compared as bits */
#define NP_GUARD 2            /* guard words on either side of every 18-float vector in LDS */
#define NP_VEC (GQ_NVD + 2 * NP_GUARD)

__device__ inline float np_canary() { return __builtin_bit_cast(float, (int)NP_CANARY); }
__device__ inline int np_dead(float v) { return __builtin_bit_cast(int, v) != (int)NP_CANARY ? 1 : 0; }
/* lanes 0 .. 4 nvec - 1: one guard word each of nvec guarded vectors */
__device__ inline int np_guards_touched(const float (*buf)[NP_VEC], int nvec, int lane) {
  if (lane >= 4 * nvec) return 0;
  const int k = lane & 3;
  return np_dead(buf[lane >> 2][k < NP_GUARD ? k : GQ_NVD + k]);
}

/* The linear solves.  MODE 0: solve_tree_fused<false>; 1: solve_tree_fused<true> with damping[] and hd; 2: solve_tree_fused<false, true>
 * (out: S^-1 g; the second quad leaves the factor of S + diag(damping)) followed by solve_tree_stored (out2: (S + diag(damping))^-1 g);
 * 3: solve_tree_fused2 (out: S^-1 g, out2: S^-1 g2).
 * Sc[nsys][12][9], Sb[nsys][6][6], damping[nsys][18], rhs / rhs2 / out / out2 [nsys][nrhs][18]; alias: out takes g's place in LDS.
 * touched[nsys][64]: guard words found changed, per lane over all right-hand sides. */
template <int MODE>
__device__ inline void np_solve(int b, int lane, const float* Sc, const float* Sb, const float* damping, float hd, const float* rhs, const float* rhs2,
                                int nrhs, int alias, float* out, float* out2, int32_t* touched) {
  __shared__ float sSc[GQ_NJ][9], sSb[6][6], sD[GQ_NVD];
  __shared__ float buf[4][NP_VEC];                 /* g, out, g2, out2 */
  __shared__ float fac[2][NP_GUARD + 96 + NP_GUARD]; /* the stored factor: fleg [4][24], fbase [21] */
  for (int k = lane; k < GQ_NJ * 9; k += 64) (&sSc[0][0])[k] = Sc[(size_t)b * GQ_NJ * 9 + k];
  if (lane < 36) (&sSb[0][0])[lane] = Sb[(size_t)b * 36 + lane];
  if (lane < GQ_NVD) sD[lane] = damping[(size_t)b * GQ_NVD + lane];
  for (int k = lane; k < 2 * (96 + 2 * NP_GUARD); k += 64) (&fac[0][0])[k] = np_canary();
  int bad = 0;
  float* fleg = &fac[0][NP_GUARD];
  float* fbase = &fac[1][NP_GUARD];
  for (int r = 0; r < nrhs; r++) {
    const size_t at = ((size_t)b * nrhs + r) * GQ_NVD;
    gq::wave_barrier();
    for (int k = lane; k < 4 * NP_VEC; k += 64) (&buf[0][0])[k] = np_canary();
    gq::wave_barrier();
    if (lane < GQ_NVD) { buf[0][NP_GUARD + lane] = rhs[at + lane]; buf[2][NP_GUARD + lane] = (MODE == 3 ? rhs2 : rhs)[at + lane]; }
    gq::wave_barrier();
    float* g = &buf[0][NP_GUARD];
    float* g2 = &buf[2][NP_GUARD];
    float* o = alias ? g : &buf[1][NP_GUARD];
    float* o2 = alias ? g2 : &buf[3][NP_GUARD];
    if constexpr (MODE == 0) gq::solve_tree_fused<false>(sSc, sSb, nullptr, 0.0f, g, o);
    if constexpr (MODE == 1) gq::solve_tree_fused<true>(sSc, sSb, sD, hd, g, o);
    if constexpr (MODE == 2) {
      gq::solve_tree_fused<false, true>(sSc, sSb, sD, 0.0f, g, o, fleg, fbase);
      gq::solve_tree_stored(fleg, fbase, g2, o2);
    }
    if constexpr (MODE == 3) gq::solve_tree_fused2(sSc, sSb, g, o, g2, o2);
    gq::wave_barrier();
    if (lane < GQ_NVD) { out[at + lane] = o[lane]; if (MODE >= 2) out2[at + lane] = o2[lane]; }
    bad += np_guards_touched(buf, 4, lane);
    /* every guard word of the stored factor: NP_GUARD words on either side of fleg [96], NP_GUARD before fbase and the words that follow
     * fbase[21] in its row (next to the data first) */
    if (lane < 2 * NP_GUARD) bad += np_dead(fac[0][lane < NP_GUARD ? lane : 96 + lane]) + np_dead(fac[1][lane < NP_GUARD ? lane : 21 + lane]);
    if (lane >= 2 * NP_GUARD && lane < 2 * NP_GUARD + 4) bad += np_dead(fac[1][21 + lane]) + np_dead(fac[1][96 + lane - 4]);   /* further past fbase; the row's end */
  }
  touched[(size_t)b * 64 + lane] = bad;
}

/* newton_dense_step.  Hc[n][12][9], Hb[n][6][6]: the tree-sparse Hessian as the assembly leaves it; J[n][64][18]: the rows (W.u.B);
 * w[n][64]: the row weights (W.force); r01[n][2]: the range [r0, r1) of rows that may couple two legs */
__device__ inline void np_dense(int b, int lane, const float* Hc, const float* Hb, const float* J, const float* w, const int32_t* r01, const float* rhs,
                                int nrhs, int alias, float* out, int32_t* touched) {
  __shared__ gq::WaveMem W;
  __shared__ float buf[2][NP_VEC];
  for (int k = lane; k < GQ_NJ * 9; k += 64) (&W.u2.n.Hc[0][0])[k] = Hc[(size_t)b * GQ_NJ * 9 + k];
  if (lane < 36) (&W.u2.n.Hb[0][0])[lane] = Hb[(size_t)b * 36 + lane];
  for (int k = lane; k < 64 * GQ_NVD; k += 64) (&W.u.B[0][0])[k] = J[(size_t)b * 64 * GQ_NVD + k];
  W.force[lane] = w[(size_t)b * 64 + lane];
  const int r0 = gq::uniform(r01[2 * b]), r1 = gq::uniform(r01[2 * b + 1]);
  int bad = 0;
  for (int r = 0; r < nrhs; r++) {
    const size_t at = ((size_t)b * nrhs + r) * GQ_NVD;
    gq::wave_barrier();
    if (lane < 2 * NP_VEC) (&buf[0][0])[lane] = np_canary();
    gq::wave_barrier();
    if (lane < GQ_NVD) buf[0][NP_GUARD + lane] = rhs[at + lane];
    gq::wave_barrier();
    float* g = &buf[0][NP_GUARD];
    float* o = alias ? g : &buf[1][NP_GUARD];
    gq::newton_dense_step(W, r0, r1, g, o);
    gq::wave_barrier();
    if (lane < GQ_NVD) out[at + lane] = o[lane];
    bad += np_guards_touched(buf, 2, lane);
  }
  touched[(size_t)b * 64 + lane] = bad;
}

/* row_law, row_piece, row_cost, row_dd of case i.  in[n][6]: y, v, R, D, floss, (unused); out[6][n]: force, cost, wact, row_cost, d1, d2;
 * piece[n] */
__device__ inline void np_rows(int i, int n, const int32_t* rtype, const float* in, float* out, int32_t* piece) {
  const float* a = in + 6 * (size_t)i;
  const float y = a[0], v = a[1], R = a[2], D = a[3], floss = a[4];
  float cost, wact, d1, d2;
  const float f = gq::row_law(rtype[i], y, R, D, floss, cost, wact);
  gq::row_dd(rtype[i], y, v, R, D, floss, d1, d2);
  out[i] = f; out[(size_t)n + i] = cost; out[2 * (size_t)n + i] = wact; out[3 * (size_t)n + i] = gq::row_cost(rtype[i], y, R, D, floss);
  out[4 * (size_t)n + i] = d1; out[5 * (size_t)n + i] = d2;
  piece[i] = gq::row_piece(rtype[i], y, R, floss);
}

/* ell_state, then ell_dd at na step lengths with the three contact sums taken the way newton_solve takes them.
 * code / r0 [n][64]; par[n][64][6]: fri, mu, D0, y, v, rD; alpha[n][na];
 * st[n][7][64]: force, cost share, wact, zone, uhat, TT, y0;  dd[n][na][2][64]: d1, d2 */
__device__ inline void np_ell(int b, int lane, const int32_t* code, const int32_t* r0, const float* par, const float* alpha, int na, float* st, float* dd) {
  const size_t i = (size_t)b * 64 + lane;
  gq::EllRow E;
  E.code = code[i]; E.r0 = r0[i]; E.fri = par[6 * i]; E.mu = par[6 * i + 1]; E.D0 = par[6 * i + 2];
  const float y = par[6 * i + 3], v = par[6 * i + 4], rD = par[6 * i + 5];
  float ci, wact, uhat, TT, y0;
  int zone;
  const float f = gq::ell_state(E, y, rD, ci, wact, zone, uhat, TT, y0);
  float* s = st + (size_t)b * 7 * 64 + lane;
  s[0] = f; s[64] = ci; s[128] = wact; s[192] = (float)zone; s[256] = uhat; s[320] = TT; s[384] = y0;
  const bool fr = (E.code & 15) >= 1;
  const float u = fr ? E.fri * y : 0.0f, V = fr ? E.fri * v : 0.0f;
  const float UV = gq::ell_seg_sum(E, u * V), VV = gq::ell_seg_sum(E, V * V), N1 = E.mu * gq::shfl_idx(v, E.r0);
  for (int k = 0; k < na; k++) {
    float d1, d2;
    gq::ell_dd(E, alpha[(size_t)b * na + k], y, v, rD, TT, y0, UV, VV, N1, d1, d2);
    float* o = dd + (((size_t)b * na + k) * 2) * 64 + lane;
    o[0] = d1; o[64] = d2;
  }
}

}  // namespace nprobe
