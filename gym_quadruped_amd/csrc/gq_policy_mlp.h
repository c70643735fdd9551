/*
 * gq_policy_mlp.h - the MLP policy of the closed-loop rollout (gq_rollout_policy, gq_policy_mlp_eval): the law of the network in two
 * forms that give the same bits, the weight blob both read, and the seat's part of the device block of a call (gq_policy_dev.h).
 * Compiles with the product's gq_device.h and with the host emulator's shim (tests/simt_emu): mlp_row_forward and everything it
 * uses is plain C++, only mlp_tile_forward needs the matrix cores.
 *
 * THE CONTRACT of a layer with K inputs and N outputs:   y_o = fmaf(x_{Kp-1}, w_{Kp-1,o}, ... fmaf(x_1, w_{1,o}, fmaf(x_0, w_{0,o}, b_o)))
 * k ascending, one rounding per fmaf, no wider accumulation; Kp = K rounded up to a multiple of 4 with x_k = w_k = 0 behind K, the
 * outputs rounded up to Np, a multiple of 16, with w = b = 0 behind N (act(0) = 0 for every activation here, so the padding of one
 * layer's outputs is the zero padding of the next layer's inputs).  v_mfma_f32_16x16x4_f32 with the bias as initial accumulator IS that
 * chain, four k at a time, for 16 rows x 16 outputs at once - the plain loop and the matrix-core form differ in nothing but speed.
 *
 * The blob (floats), layer after layer:  weights [Np / 16 column blocks][Kp / 4 row blocks][64 lanes], then Np biases.  Lane l of a
 * (column block cb, row block kb) holds w[k = 4 kb + (l >> 4)][o = 16 cb + (l & 15)]: the B operand of the MFMA as the lanes hold it,
 * one coalesced 256-byte load per fetch.
 */
#pragma once
#include <gq_device.h> /* angle brackets: the include path decides (csrc/ for the product, tests/simt_emu/ for the emulator) */
#include <cmath>
#include <cstddef>
#include <cstdint>

#define GQ_MLP_MAXL 4     /* linear layers */
#define GQ_MLP_MAXW 256   /* inputs / outputs of a layer */
#define GQ_MLP_ROWS 16    /* rows of a tile (the M of the MFMA) */
#define GQ_MLP_NOISE_STREAM 0x3b1fu /* word 3 of the noise's Philox counter (the PD policy's stream is 0x9011) */

namespace gq {

enum { MLP_ACT_NONE = 0, MLP_ACT_RELU = 1, MLP_ACT_ELU = 2, MLP_ACT_TANH = 3 };

/* the network's shape: layer l maps (l == 0 ? in_dim : width[l - 1]) inputs to width[l] outputs, act between layers, out_act at the end */
struct MlpNet {
  int32_t n_layers, in_dim, act, out_act;
  int32_t width[GQ_MLP_MAXL];
};
__host__ __device__ inline int mlp_kp(const int k) { return (k + 3) & ~3; }
__host__ __device__ inline int mlp_np(const int n) { return (n + 15) & ~15; }
__host__ __device__ inline int mlp_layer_in(const MlpNet& net, const int l) { return l == 0 ? net.in_dim : net.width[l - 1]; }
__host__ __device__ inline size_t mlp_layer_floats(const MlpNet& net, const int l) {
  return (size_t)mlp_np(net.width[l]) * (size_t)(mlp_kp(mlp_layer_in(net, l)) + 1);
}
__host__ __device__ inline size_t mlp_blob_floats(const MlpNet& net) {
  size_t n = 0;
  for (int l = 0; l < net.n_layers; l++) n += mlp_layer_floats(net, l);
  return n;
}

/* ---- the arithmetic both forms share: IEEE operations and fmaf, contraction off - the same bits from any compiler ---- */
__host__ __device__ inline float mlp_bits_float(const uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
__host__ __device__ inline uint32_t mlp_float_bits(const float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

/* x in [-88, 88]:  exp(x) - 1 = s p + (s - 1) with s = 2^n, n = round(x / ln 2), p = expm1(x - n ln 2) from a polynomial on |r| <= 0.347 */
__host__ __device__ inline float mlp_expm1(const float x) {
#pragma clang fp contract(off)
  const float t = x * 1.44269504f;
  const int n = (int)(t + (t < 0.0f ? -0.5f : 0.5f));
  const float fn = (float)n;
  float r = fmaf(fn, -0.693359375f, x);     /* ln 2 in two parts (Cody - Waite): the first product is exact */
  r = fmaf(fn, 2.12194440e-4f, r);
  float q = 2.48015873e-5f;                 /* 1 / 8! */
  q = fmaf(q, r, 1.98412698e-4f);
  q = fmaf(q, r, 1.38888889e-3f);
  q = fmaf(q, r, 8.33333333e-3f);
  q = fmaf(q, r, 4.16666667e-2f);
  q = fmaf(q, r, 1.66666667e-1f);
  q = fmaf(q, r, 0.5f);
  const float r2 = r * r;
  const float p = fmaf(q, r2, r);
  const float s = mlp_bits_float((uint32_t)(n + 127) << 23);
  const float sm1 = s - 1.0f;
  return fmaf(s, p, sm1);
}
/* n / d for d >= 1: a reciprocal from the exponent trick and four Newton steps, then one correction of the quotient */
__host__ __device__ inline float mlp_div(const float n, const float d) {
#pragma clang fp contract(off)
  float r = mlp_bits_float(0x7EF311C7u - mlp_float_bits(d));
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float e = fmaf(-d, r, 1.0f);
    r = fmaf(r, e, r);
  }
  const float y = n * r;
  const float res = fmaf(-d, y, n);
  return fmaf(res, r, y);
}
__host__ __device__ inline float mlp_elu(const float x) {
  if (!(x < 0.0f)) return x;          /* also NaN */
  if (x < -17.5f) return -1.0f;       /* exp(x) < 2^-25: the sum rounds to -1 */
  return mlp_expm1(x);
}
__host__ __device__ inline float mlp_tanh(const float x) {
#pragma clang fp contract(off)
  const float a = fabsf(x);
  if (!(a == a)) return x;
  float y = 1.0f;                     /* 1 - tanh(a) < 2^-25 from a = 9.02 */
  if (a < 9.02f) {
    const float t = mlp_expm1(a + a); /* tanh a = (e^2a - 1) / (e^2a + 1) = t / (t + 2) */
    const float d = t + 2.0f;
    y = mlp_div(t, d);
  }
  return x < 0.0f ? -y : y;
}
__host__ __device__ inline float mlp_activate(const int act, const float v) {
  switch (act) {
    case MLP_ACT_RELU: return v > 0.0f ? v : 0.0f;
    case MLP_ACT_ELU: return mlp_elu(v);
    case MLP_ACT_TANH: return mlp_tanh(v);
    default: return v;
  }
}
/* column c of the network's input row from column c of the observation row: (o - shift) * scale, each rounded; absent rows: identity */
__host__ __device__ inline float mlp_obs_in(const float o, const float* shift, const float* scale, const int c) {
#pragma clang fp contract(off)
  float v = o;
  if (shift) v = v - shift[c];
  if (scale) v = v * scale[c];
  return v;
}
/* standard normal from words 0, 1 of a Philox block (Box - Muller, u1 in (0, 1), u2 in [0, 1)) in fp64 from +, -, *, / and sqrt alone, each
 * rounded on its own: numpy's float64 gives the same bits (tests/policy_mlp_ref.py restates it line by line) */
__host__ __device__ inline float mlp_normal(const uint32_t x0, const uint32_t x1) {
#pragma clang fp contract(off)
  /* ln u1, u1 = (2 (x0 >> 8) + 1) 2^-25 = m 2^(e - 25), m in [1, 2) */
  const uint32_t v = 2u * (x0 >> 8) + 1u;
  int e = 31 - __builtin_clz(v);
  double m = (double)v / (double)(1u << e);
  if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
  const double s = (m - 1.0) / (m + 1.0), s2 = s * s;   /* ln m = 2 atanh s, |s| <= 0.1716 */
  double p = 1.0 / 15.0;
  p = p * s2 + 1.0 / 13.0;
  p = p * s2 + 1.0 / 11.0;
  p = p * s2 + 1.0 / 9.0;
  p = p * s2 + 1.0 / 7.0;
  p = p * s2 + 1.0 / 5.0;
  p = p * s2 + 1.0 / 3.0;
  p = p * s2 + 1.0;
  const double ln_u1 = (double)(e - 25) * 0.6931471805599453 + 2.0 * s * p;
  /* cos(2 pi u2), u2 = (x1 >> 8) 2^-24:  w = u2 - 1/2, a = |w|, b = a or 1/2 - a in [0, 1/4]; every step exact */
  const double u2 = (double)(x1 >> 8) * (1.0 / 16777216.0);
  const double w = u2 - 0.5, a = w < 0.0 ? -w : w;
  const bool fold = a > 0.25;
  const double b = fold ? 0.5 - a : a;
  const double th = 6.283185307179586 * b, t2 = th * th;
  double c = 1.0 / 20922789888000.0; /* 1 / 16! */
  c = 1.0 / 87178291200.0 - c * t2;
  c = 1.0 / 479001600.0 - c * t2;
  c = 1.0 / 3628800.0 - c * t2;
  c = 1.0 / 40320.0 - c * t2;
  c = 1.0 / 720.0 - c * t2;
  c = 1.0 / 24.0 - c * t2;
  c = 0.5 - c * t2;
  c = 1.0 - c * t2;                  /* cos(2 pi b); cos(2 pi u2) = -cos(2 pi a) = fold ? c : -c */
  const double z = sqrt(-2.0 * ln_u1) * (fold ? c : -c);
  return (float)z;
}

/* ---- form 1, THE DEFINITION: one row, plain loops ---- */
/* layer l alone: x[Kp] (zero behind K) -> y[Np]; w = the layer's place in the blob */
__host__ __device__ inline void mlp_row_layer(const MlpNet& net, const int l, const float* w, const float* x, float* y) {
  const int kp = mlp_kp(mlp_layer_in(net, l)), np = mlp_np(net.width[l]), nkb = kp >> 2;
  const int act = l == net.n_layers - 1 ? net.out_act : net.act;
  const float* bias = w + (size_t)np * kp;
  for (int o = 0; o < np; o++) {
    float acc = bias[o];
    const float* wo = w + (size_t)(o >> 4) * nkb * 64 + (o & 15);
    for (int k = 0; k < kp; k++) acc = fmaf(x[k], wo[(k >> 2) * 64 + (k & 3) * 16], acc);
    y[o] = mlp_activate(act, acc);
  }
}
/* x: the in_dim values of the input row (shift / scale applied); y: the 12 outputs */
__host__ __device__ inline void mlp_row_forward(const MlpNet& net, const float* blob, const float* x, float* y) {
  float buf[2][GQ_MLP_MAXW];
  const int kp0 = mlp_kp(net.in_dim);
  for (int c = 0; c < kp0; c++) buf[0][c] = c < net.in_dim ? x[c] : 0.0f;
  int cur = 0;
  const float* w = blob;
  for (int l = 0; l < net.n_layers; l++) {
    mlp_row_layer(net, l, w, buf[cur], buf[cur ^ 1]);
    w += mlp_layer_floats(net, l);
    cur ^= 1;
  }
  for (int j = 0; j < net.width[net.n_layers - 1]; j++) y[j] = buf[cur][j];
}

#if defined(__HIPCC__)
/* ---- form 2: one wavefront takes a tile of 16 rows through the layers on the matrix cores ----
 * An activation buffer holds a tile TRANSPOSED, xt[k][row] (GQ_MLP_MAXW x 16 floats): the A operand of row block kb - lane l: x[row l & 15]
 * [k = 4 kb + (l >> 4)] - is the 64 consecutive words from 64 kb (no bank conflict), and the four results a lane holds of a column block
 * - rows 4 (l >> 4) .. + 3 of output 16 cb + (l & 15) - are one 16-byte store.  A row's chain reads that row's words only: its result
 * does not depend on the rows beside it, on its slot or on how full the tile is. */
typedef float mlp_f32x4 __attribute__((ext_vector_type(4)));
/* the shape out of the device block (constant address space: scalar loads) into registers */
__device__ __forceinline__ MlpNet mlp_net_load(const GQ_MODEL MlpNet& s) {
  MlpNet n;
  n.n_layers = s.n_layers; n.in_dim = s.in_dim; n.act = s.act; n.out_act = s.out_act;
#pragma unroll
  for (int l = 0; l < GQ_MLP_MAXL; l++) n.width[l] = s.width[l];
  return n;
}

/* NB column blocks from cb0 on, side by side: NB independent accumulator chains share every A fetch (the dependent latency of the
 * instruction is 40 cycles, its issue interval 32) */
template <int NB>
__device__ __forceinline__ void mlp_tile_blocks(const float* __restrict__ w, const float* __restrict__ bias, const int cb0, const int nkb, const int act,
                                                const float* xin, float* xout, const int lane) {
  mlp_f32x4 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const float b = gptr(bias)[(cb0 + i) * 16 + (lane & 15)];
    acc[i] = mlp_f32x4{b, b, b, b};
  }
  const GQ_GLOBAL float* wp = gptr(w) + (size_t)cb0 * nkb * 64 + lane;
  /* the weights come from the L2 (a microsecond away): the operands of MLP_KU row blocks are fetched while the previous MLP_KU are
   * multiplied.  Each accumulator still takes its row blocks in ascending order. */
  constexpr int MLP_KU = 4;
  const int nfull = nkb & ~(MLP_KU - 1);
  float a0[MLP_KU], b0[NB][MLP_KU];
  if (nfull) {
#pragma unroll
    for (int u = 0; u < MLP_KU; u++) {
      a0[u] = xin[u * 64 + lane];
#pragma unroll
      for (int i = 0; i < NB; i++) b0[i][u] = wp[((size_t)i * nkb + u) * 64];
    }
  }
  for (int kb = 0; kb < nfull; kb += MLP_KU) {
    float a1[MLP_KU], b1[NB][MLP_KU];
    const bool more = kb + MLP_KU < nfull;
    if (more) {
#pragma unroll
      for (int u = 0; u < MLP_KU; u++) {
        a1[u] = xin[(kb + MLP_KU + u) * 64 + lane];
#pragma unroll
        for (int i = 0; i < NB; i++) b1[i][u] = wp[((size_t)i * nkb + kb + MLP_KU + u) * 64];
      }
    }
#pragma unroll
    for (int u = 0; u < MLP_KU; u++)
#pragma unroll
      for (int i = 0; i < NB; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b0[i][u], acc[i], 0, 0, 0);
    if (more) {
#pragma unroll
      for (int u = 0; u < MLP_KU; u++) {
        a0[u] = a1[u];
#pragma unroll
        for (int i = 0; i < NB; i++) b0[i][u] = b1[i][u];
      }
    }
  }
  for (int kb = nfull; kb < nkb; kb++) {
    const float a = xin[kb * 64 + lane];
#pragma unroll
    for (int i = 0; i < NB; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[((size_t)i * nkb + kb) * 64], acc[i], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < NB; i++) {
    mlp_f32x4 y;
#pragma unroll
    for (int r = 0; r < 4; r++) y[r] = mlp_activate(act, acc[i][r]);
    *reinterpret_cast<mlp_f32x4*>(xout + ((cb0 + i) * 16 + (lane & 15)) * GQ_MLP_ROWS + (lane >> 4) * 4) = y;
  }
}
/* the tile staged in xt0 (every word of rows 0 .. 15, columns 0 .. Kp of layer 0 - zero where there is no row or no column); returns the
 * buffer that holds the outputs, out[j][row].  Wave-uniform control flow; net in scalar registers. */
__device__ __forceinline__ float* mlp_tile_forward(const MlpNet& net, const float* __restrict__ blob, float* xt0, float* xt1) {
  const int lane = lane_id() & (GQ_WAVE - 1);
  const float* w = blob;
  float* xin = xt0;
  float* xout = xt1;
#pragma unroll /* (in full: width[l] with a constant l is a register, with a variable one the struct goes to scratch) */
  for (int l = 0; l < GQ_MLP_MAXL; l++) {
    if (l >= net.n_layers) break;
    const int kp = mlp_kp(mlp_layer_in(net, l)), np = mlp_np(net.width[l]), nkb = kp >> 2, ncb = np >> 4;
    const int act = l == net.n_layers - 1 ? net.out_act : net.act;
    const float* bias = w + (size_t)np * kp;
    wave_barrier(); /* the layer's inputs were stored by other lanes */
    int cb = 0;
    for (; cb + 4 <= ncb; cb += 4) mlp_tile_blocks<4>(w, bias, cb, nkb, act, xin, xout, lane);
    if (cb + 2 <= ncb) { mlp_tile_blocks<2>(w, bias, cb, nkb, act, xin, xout, lane); cb += 2; }
    if (cb < ncb) mlp_tile_blocks<1>(w, bias, cb, nkb, act, xin, xout, lane);
    w += mlp_layer_floats(net, l);
    float* t = xin; xin = xout; xout = t;
  }
  wave_barrier();
  return xin;
}
/* stage a tile: value(row, column) for every word the first layer reads (the caller returns 0 where the tile has no row / the row no
 * column).  Lane l handles row l & 15, columns (l >> 4) + 4 i: consecutive lanes store consecutive words. */
template <class F>
__device__ __forceinline__ void mlp_tile_stage(const MlpNet& net, float* xt0, F value) {
  const int lane = lane_id() & (GQ_WAVE - 1), r = lane & 15, kp0 = mlp_kp(net.in_dim);
  wave_barrier(); /* whoever still read the buffers has done so */
  for (int c = lane >> 4; c < kp0; c += 4) xt0[c * GQ_MLP_ROWS + r] = value(r, c);
}
#endif /* __HIPCC__ */

/* the seat's part of a call's device block (PolicyDev, gq_policy_dev.h): the network, the leading columns of the input row, the loop */
struct LearnFeetDev;
struct PolicyMlpDev {
  MlpNet net;
  int32_t in_obs, feed_last;    /* leading observation columns fed to the net; 1: the env's last action (12) follows them */
  int32_t decimation, pad_;
  const float* blob;
  const float* shift; const float* scale; /* [in_obs] or NULL */
  int32_t col_q[12], col_qd[12];          /* columns of the joint angles / velocities in the observation row */
  float kp[12], kd[12], q_default[12], action_scale[12], sigma[12];
  float clip;                   /* > 0: actions are clipped to +- clip */
  uint32_t seed_lo, seed_hi; int32_t step0, env_id_offset; /* noise: Philox block (joint, step0 + k, global env id, GQ_MLP_NOISE_STREAM), key = seed */
  int32_t pad2_;
  int32_t* issued;              /* [N] actions issued per env in this call (the policy's private count) */
  float* held;                  /* [N][12] the action the env tracks until its next policy step */
  float* last;                  /* [N][12] the env's previous policy action (feed_last) */
  float* policy_actions;        /* [n_steps / decimation][N][12] record, or NULL */
  const LearnFeetDev* learn;    /* a learning call's block (gq_learn.h): read by policy_mlp_kernel<1> and <2> alone */
};
}  // namespace gq
