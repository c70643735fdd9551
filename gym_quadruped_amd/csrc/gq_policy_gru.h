/*
 * gq_policy_gru.h - the RECURRENT policy of the closed-loop rollout (gq_rollout_policy_gru, gq_policy_gru_eval): one GRU cell followed by an
 * MLP head, the law in two forms that give the same bits, the weight blob both read and THE EPISODE RULE of the hidden state (the device
 * block of a call: gq_policy_dev.h).  Plain C++ for host and device like gq_policy_mlp.h, on which everything here is built: a gate's pre-activation IS a layer
 * of that header (y_o = the k-ascending fmaf chain from the bias, Kp | 4, Np | 16, what v_mfma_f32_16x16x4_f32 computes), the transcendental
 * arithmetic is its bit-defined mlp_tanh and nothing else.  Contraction off; the ORDER of the operations below is the definition.
 *
 * THE LAW.  Input row x (in_dim = in_obs + 12 feed_last_action <= 256), hidden row h (H values, 1 <= H <= 128), gates in torch's order
 * (r, z, n) with both bias vectors kept, as torch.nn.GRUCell keeps them:
 *   gi_g = layer(x; W_ig, b_ig)   gh_g = layer(h; W_hg, b_hg)     g in {r, z, n}, no activation
 *   sig(v) = fmaf(0.5f, mlp_tanh(0.5f * v), 0.5f)
 *   r  = sig(gi_r + gh_r)          z = sig(gi_z + gh_z)           one rounded add each
 *   n  = mlp_tanh(fmaf(r, gh_n, gi_n))
 *   h' = fmaf(z, h - n, n)                                         (= (1 - z) n + z h)
 *   a  = head(h')                                                  an MlpNet of 1 to 3 layers from H to 12 outputs
 * PADDING.  The hidden columns behind H (up to Hp = H rounded up to 16) stay EXACTLY 0 through the gate law: their weights and biases are 0,
 * so gi = gh = 0, sig(0) = fmaf(0.5, 0, 0.5) = 0.5, n = mlp_tanh(fmaf(0.5, 0, 0)) = 0 and h' = fmaf(0.5, 0 - 0, 0) = 0.  The head's first
 * layer reads h' with the zero padding of its inputs (Kp of H <= Hp): it relies on this.
 *
 * THE BLOB (floats): the six gate layers in the per-layer layout of gq_policy_mlp.h ([Np / 16][Kp / 4][64] weights, then Np biases), in the
 * order  W_ir b_ir | W_hr b_hr | W_iz b_iz | W_hz b_hz | W_in b_in | W_hn b_hn  (GRU_W_*), then the head's layers as mlp_blob_floats lays
 * them out.  gru_blob_floats is checked on entry.
 *
 * THE EPISODE RULE (gru_episode_rule, one routine for the kernel and the host).  At the visit of env e for step k - the observation after
 * step k - 1 is out - BEFORE any cell evaluation of that visit:
 *   k == 0   the env waits for its re-spawn (pending[e]):            its hidden row := 0
 *   k >= 1   the `terminated` byte after step k - 1 is set:          its hidden row := 0      (the byte learn_visit reads)
 * The learning modes' closing visit k = K applies the same rule; the plain mode has no closing visit, and a fall in step K - 1 is caught by
 * the next call's k == 0 rule (the env is pending then).  The zeroing is EAGER - done at the visit that sees the flag - so nothing but the
 * hidden rows themselves crosses a call.  Consequence: the hidden state fed at policy step s + 1 is zero exactly when window s (steps D s ..
 * D s + D - 1) contained a termination - exactly when dones[s] is set in the learning modes: the mask h <- (1 - done) h of a recurrent
 * learner.  The fed-back last action (feed_last_action) keeps its semantics: zeros at the first policy step of a call, kept across a
 * re-spawn.
 */
#pragma once
#include "gq_policy_mlp.h"
#include "gq_learn.h" /* LearnPlain / LearnPub: the memory access of the episode rule */

#define GQ_GRU_MAXH 128   /* hidden units */
#define GQ_GRU_HEAD_MAXL 3 /* linear layers of the head */

namespace gq {

struct GruNet {
  int32_t in_dim, hidden;
};
enum { GRU_W_IR = 0, GRU_W_HR = 1, GRU_W_IZ = 2, GRU_W_HZ = 3, GRU_W_IN = 4, GRU_W_HN = 5 };

/* a gate's pre-activation as a one-layer network of gq_policy_mlp.h without activation: K inputs, N outputs */
__host__ __device__ inline MlpNet gru_gate_net(const int K, const int N) {
  MlpNet n{};
  n.n_layers = 1; n.in_dim = K; n.act = MLP_ACT_NONE; n.out_act = MLP_ACT_NONE; n.width[0] = N;
  return n;
}
__host__ __device__ inline size_t gru_gate_floats(const int K, const int N) { return (size_t)mlp_np(N) * (size_t)(mlp_kp(K) + 1); }
__host__ __device__ inline size_t gru_cell_floats(const GruNet& G) { return 3 * (gru_gate_floats(G.in_dim, G.hidden) + gru_gate_floats(G.hidden, G.hidden)); }
__host__ __device__ inline size_t gru_blob_floats(const GruNet& G, const MlpNet& head) { return gru_cell_floats(G) + mlp_blob_floats(head); }
/* where layer `which` (GRU_W_*) starts in the blob */
__host__ __device__ inline const float* gru_gate_blob(const GruNet& G, const float* blob, const int which) {
  const size_t gi = gru_gate_floats(G.in_dim, G.hidden), gh = gru_gate_floats(G.hidden, G.hidden);
  return blob + (size_t)(which >> 1) * (gi + gh) + (size_t)(which & 1) * gi;
}

/* ---- the gate law, elementwise: what both forms call ---- */
__host__ __device__ inline float gru_sig(const float v) {
#pragma clang fp contract(off)
  const float hv = 0.5f * v;
  return fmaf(0.5f, mlp_tanh(hv), 0.5f);
}
__host__ __device__ inline float gru_gate(const float gi, const float gh) { /* r and z */
#pragma clang fp contract(off)
  const float s = gi + gh;
  return gru_sig(s);
}
__host__ __device__ inline float gru_cand(const float r, const float gi_n, const float gh_n) { return mlp_tanh(fmaf(r, gh_n, gi_n)); }
__host__ __device__ inline float gru_blend(const float z, const float h, const float n) {
#pragma clang fp contract(off)
  const float d = h - n;
  return fmaf(z, d, n);
}

/* ---- form 1, THE DEFINITION: one row, plain loops ---- */
/* x: the in_dim values of the input row (shift / scale applied); h: H values; hn: Hp values out, H rounded up to 16 - every column the
 * layers compute goes through the gate law, as in the tile form, and the ones behind H come out 0 (head comment); may not alias h */
__host__ __device__ inline void gru_row_cell(const GruNet& G, const float* blob, const float* x, const float* h, float* hn) {
  const int H = G.hidden, kpx = mlp_kp(G.in_dim), hp = mlp_np(H);
  float xb[GQ_MLP_MAXW], hb[GQ_GRU_MAXH], gi[GQ_GRU_MAXH], gh[GQ_GRU_MAXH], r[GQ_GRU_MAXH], n[GQ_GRU_MAXH];
  for (int c = 0; c < kpx; c++) xb[c] = c < G.in_dim ? x[c] : 0.0f;
  for (int c = 0; c < hp; c++) hb[c] = c < H ? h[c] : 0.0f;
  const MlpNet nx = gru_gate_net(G.in_dim, H), nh = gru_gate_net(H, H);
  mlp_row_layer(nx, 0, gru_gate_blob(G, blob, GRU_W_IR), xb, gi);
  mlp_row_layer(nh, 0, gru_gate_blob(G, blob, GRU_W_HR), hb, gh);
  for (int c = 0; c < hp; c++) r[c] = gru_gate(gi[c], gh[c]);
  mlp_row_layer(nx, 0, gru_gate_blob(G, blob, GRU_W_IN), xb, gi);
  mlp_row_layer(nh, 0, gru_gate_blob(G, blob, GRU_W_HN), hb, gh);
  for (int c = 0; c < hp; c++) n[c] = gru_cand(r[c], gi[c], gh[c]);
  mlp_row_layer(nx, 0, gru_gate_blob(G, blob, GRU_W_IZ), xb, gi);
  mlp_row_layer(nh, 0, gru_gate_blob(G, blob, GRU_W_HZ), hb, gh);
  for (int c = 0; c < hp; c++) hn[c] = gru_blend(gru_gate(gi[c], gh[c]), hb[c], n[c]);
}
/* the whole policy: a[12] = head(h'), hn[Hp] = h'.  head.in_dim == G.hidden */
__host__ __device__ inline void gru_row_forward(const GruNet& G, const MlpNet& head, const float* blob, const float* x, const float* h, float* a, float* hn) {
  gru_row_cell(G, blob, x, h, hn);
  mlp_row_forward(head, blob + gru_cell_floats(G), hn, a);
}

#if defined(__HIPCC__)
/* ---- form 2: one wavefront takes a tile of 16 rows through the cell and the head on the matrix cores ----
 * LDS: three regions of GQ_MLP_MAXW x 16 floats (16 KB each, 48 KB), every buffer a transposed tile as in gq_policy_mlp.h:
 *   region 0   x          [256][16]
 *   region 1   h | A      [128][16] each
 *   region 2   B | R      [128][16] each
 * The gates run one after the other, every chain through mlp_tile_blocks (the same MFMA sequence as a layer of the MLP):
 *   r-phase  A = gi_r, B = gh_r, R = sig(A + B)
 *   n-phase  A = gi_n, B = gh_n, R = tanh(fmaf(R, B, A))
 *   z-phase  A = gi_z, B = gh_z, h = fmaf(sig(A + B), h - R, R)   in place
 * The elementwise passes touch, in every lane, the words that lane's chains stored (mlp_tile_blocks: output 16 cb + (l & 15), rows
 * 4 (l >> 4) .. + 3): no exchange between lanes; only the in-place update of h waits until every lane's chains have read h.  The head then
 * runs mlp_tile_forward with region 1 as its input buffer and region 2 as the other one.  A row's chains read that row's words only: its
 * result does not depend on the rows beside it, on its slot or on how full the tile is. */
#define GQ_GRU_REGION (GQ_MLP_MAXW * GQ_MLP_ROWS)
#define GQ_GRU_LDS_FLOATS (3 * GQ_GRU_REGION)
__device__ __forceinline__ GruNet gru_net_load(const GQ_MODEL GruNet& s) {
  GruNet n;
  n.in_dim = s.in_dim; n.hidden = s.hidden;
  return n;
}
/* stage ncol columns of a transposed tile: lane l handles row l & 15, columns (l >> 4) + 4 i (consecutive lanes, consecutive words) */
template <class F>
__device__ __forceinline__ void gru_tile_stage(const int ncol, float* dst, F value) {
  const int lane = lane_id() & (GQ_WAVE - 1), r = lane & 15;
  for (int c = lane >> 4; c < ncol; c += 4) dst[c * GQ_MLP_ROWS + r] = value(r, c);
}
/* one gate layer over the tile: K inputs in xin, N outputs to xout, no activation */
__device__ __forceinline__ void gru_tile_layer(const float* __restrict__ w, const int K, const int N, const float* xin, float* xout, const int lane) {
  const int kp = mlp_kp(K), np = mlp_np(N), nkb = kp >> 2, ncb = np >> 4;
  const float* bias = w + (size_t)np * kp;
  int cb = 0;
  for (; cb + 4 <= ncb; cb += 4) mlp_tile_blocks<4>(w, bias, cb, nkb, MLP_ACT_NONE, xin, xout, lane);
  if (cb + 2 <= ncb) { mlp_tile_blocks<2>(w, bias, cb, nkb, MLP_ACT_NONE, xin, xout, lane); cb += 2; }
  if (cb < ncb) mlp_tile_blocks<1>(w, bias, cb, nkb, MLP_ACT_NONE, xin, xout, lane);
}
/* the cell: x staged in region 0 (columns 0 .. Kp of in_dim), h in the first half of region 1 (columns 0 .. Hp), zero where the tile has no
 * row or the row no column; afterwards h' stands where h stood (still zero behind H).  xt: GQ_GRU_LDS_FLOATS floats, 16-byte aligned. */
__device__ __forceinline__ void gru_tile_cell(const GruNet& G, const float* __restrict__ blob, float* xt) {
  const int lane = lane_id() & (GQ_WAVE - 1), H = G.hidden, ncb = mlp_np(H) >> 4;
  float* const x = xt;
  float* const h = xt + GQ_GRU_REGION;
  float* const A = h + GQ_GRU_REGION / 2;
  float* const B = xt + 2 * GQ_GRU_REGION;
  float* const R = B + GQ_GRU_REGION / 2;
  const int own = (lane & 15) * GQ_MLP_ROWS + (lane >> 4) * 4; /* this lane's four words of column block 0 */
  wave_barrier(); /* the tile was staged by other lanes */
  gru_tile_layer(gru_gate_blob(G, blob, GRU_W_IR), G.in_dim, H, x, A, lane);
  gru_tile_layer(gru_gate_blob(G, blob, GRU_W_HR), H, H, h, B, lane);
  for (int cb = 0; cb < ncb; cb++) {
    const int at = cb * 16 * GQ_MLP_ROWS + own;
    const mlp_f32x4 a = *reinterpret_cast<const mlp_f32x4*>(A + at), b = *reinterpret_cast<const mlp_f32x4*>(B + at);
    mlp_f32x4 y;
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = gru_gate(a[i], b[i]);
    *reinterpret_cast<mlp_f32x4*>(R + at) = y;
  }
  gru_tile_layer(gru_gate_blob(G, blob, GRU_W_IN), G.in_dim, H, x, A, lane);
  gru_tile_layer(gru_gate_blob(G, blob, GRU_W_HN), H, H, h, B, lane);
  for (int cb = 0; cb < ncb; cb++) {
    const int at = cb * 16 * GQ_MLP_ROWS + own;
    const mlp_f32x4 a = *reinterpret_cast<const mlp_f32x4*>(A + at), b = *reinterpret_cast<const mlp_f32x4*>(B + at), r = *reinterpret_cast<const mlp_f32x4*>(R + at);
    mlp_f32x4 y;
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = gru_cand(r[i], a[i], b[i]);
    *reinterpret_cast<mlp_f32x4*>(R + at) = y;
  }
  gru_tile_layer(gru_gate_blob(G, blob, GRU_W_IZ), G.in_dim, H, x, A, lane);
  gru_tile_layer(gru_gate_blob(G, blob, GRU_W_HZ), H, H, h, B, lane);
  wave_barrier(); /* every lane's chains have read h */
  for (int cb = 0; cb < ncb; cb++) {
    const int at = cb * 16 * GQ_MLP_ROWS + own;
    const mlp_f32x4 a = *reinterpret_cast<const mlp_f32x4*>(A + at), b = *reinterpret_cast<const mlp_f32x4*>(B + at), n = *reinterpret_cast<const mlp_f32x4*>(R + at);
    const mlp_f32x4 h0 = *reinterpret_cast<const mlp_f32x4*>(h + at);
    mlp_f32x4 y;
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = gru_blend(gru_gate(a[i], b[i]), h0[i], n[i]);
    *reinterpret_cast<mlp_f32x4*>(h + at) = y;
  }
  wave_barrier(); /* h' is read by other lanes */
}
/* the whole policy over a staged tile.  store_h(hn): called between the cell and the head with hn[c][row] = h' (the head's second layer
 * overwrites it).  Returns the buffer that holds the 12 outputs, out[j][row].  Wave-uniform control flow. */
template <class F>
__device__ __forceinline__ float* gru_tile_forward(const GruNet& G, const MlpNet& head, const float* __restrict__ blob, const float* __restrict__ head_blob, float* xt, F store_h) {
  gru_tile_cell(G, blob, xt);
  store_h((const float*)(xt + GQ_GRU_REGION));
  return mlp_tile_forward(head, head_blob, xt + GQ_GRU_REGION, xt + 2 * GQ_GRU_REGION);
}
#endif /* __HIPCC__ */

/* THE EPISODE RULE (head comment): the visit of env e for step k.  Returns whether the row was zeroed.  Mem: LearnPlain on the host,
 * LearnPub in the rollout (the flags are the step side's stores of this launch; the row is written by the env's own lane alone). */
template <class Mem>
__host__ __device__ inline bool gru_episode_rule(const uint8_t* terminated, const uint8_t* pending, float* hidden_state, const int H, const int e, const int k) {
  const bool reset = k == 0 ? (pending != nullptr && Mem::ld_u8(pending + e) != 0) : Mem::ld_u8(terminated + e) != 0;
  if (reset)
    for (int c = 0; c < H; c++) Mem::st(hidden_state + (size_t)e * H + c, 0.0f);
  return reset;
}
}  // namespace gq
