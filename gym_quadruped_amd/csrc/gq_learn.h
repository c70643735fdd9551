/*
 * gq_learn.h - THE WINDOW LAW of the learning rollout (gq_rollout_policy_learn, gq_rollout_policy_learn_feet): which physics steps earn, what
 * a re-spawn step does, what the tail of a window after a fall does, when a window flushes and what the closing visit does - and the ONE
 * routine that gathers a step's words and evaluates the step law (gq_reward.h, continued by gq_reward_feet.h with FEET).  Plain C++ for host
 * and device like the two reward headers: policy_mlp_kernel<1 / 2> calls learn_visit with device-scope memory access, reward_eval_kernel
 * calls learn_step with plain loads, tests/foot_reward_host.cpp compiles both with g++ and plays whole windows on the host.  Contraction
 * off, IEEE operations only; the ORDER of the operations below is the definition.
 *
 * Per env three words carry the window across visits - acc (the window's reward so far), wstate (LEARN_*) and, with FEET, the four air
 * times - all private to the env's lane.  The visit for step k (the observation after step k - 1 is out):
 *   k == 0      an env that waits for its re-spawn (pending) spends step 0 on it: LEARN_RESPAWN.
 *   k >= 1      step k - 1 is evaluated.  It EARNS unless the window is dead or the step was the env's re-spawn: acc = acc + r, and a
 *               termination in an earning step makes the window dead and done.  With FEET the air times advance in every step that is not
 *               a re-spawn - also in a dead window's tail, which earns nothing but in which feet leave the ground - and are zeroed at the
 *               re-spawn step.  `terminated` after step k - 1 makes step k the re-spawn.
 *   k % D == 0  window k / D - 1 is complete: rewards, dones are written, acc and the flags start over (LEARN_RESPAWN stays).
 * k = K is the closing visit: it evaluates step K - 1 and flushes the last window.
 */
#pragma once
#include "gq_reward_feet.h"

namespace gq {

/* what a call of gq_rollout_policy_learn adds to the policy's block (PolicyDev::seat.learn points at it; device pointers) */
struct LearnDev {
  RewardLaw law;
  int32_t has_reward, pad_;
  const uint8_t* terminated;    /* [N] the batch's flag: the step side stores it before it publishes the step */
  const uint8_t* pending;       /* [N] 1: the env re-spawns at its next step (next-step auto-reset), or NULL */
  float* acc;                   /* [N] the window's reward so far (private to the env's lane) */
  int32_t* wstate;              /* [N] bit 0: the window is dead, bit 1: it saw a termination, bit 2: the env's next step is its re-spawn */
  float* prev;                  /* [N][12] the policy action before the held one */
  float* rewards;               /* [n_steps / decimation][N] or NULL */
  uint8_t* dones;               /* [n_steps / decimation][N] or NULL */
  float* policy_obs;            /* [n_steps / decimation][N][in_dim] or NULL */
  float* policy_means;          /* [n_steps / decimation][N][12] or NULL */
};
enum { LEARN_DEAD = 1, LEARN_DONE = 2, LEARN_RESPAWN = 4 };

/* the block of every learning call and of gq_reward_eval / gq_reward_eval_feet: LearnDev and the feet (read with FEET alone) */
struct LearnFeetDev {
  LearnDev learn;
  FootLaw feet;
  float* air_time;              /* [N][4] the feet's air times, canonical order: caller-owned, in / out (private to the env's lane) */
};

/* ONE STEP: every load is issued before the first word is used - the foot columns, the air times, then the twelve terms' words - then the
 * step law.  row: column -> float; air: foot -> float; u, a, a_prev: joint -> float.  A step that does not earn (FEET alone: a dead
 * window's tail) advances the foot state and returns 0.  t[4]: the air times, loaded, advanced and left to the caller to store. */
template <bool FEET, class LdRow, class LdAir, class LdU, class LdA, class LdAp>
__host__ __device__ inline float learn_step(const RewardLaw& R, const FootLaw& F, const bool earns, const int terminated, LdRow row, LdAir air, LdU u, LdA a, LdAp a_prev,
                                            float t[4]) {
  FootIn fin;
  if constexpr (FEET) {
    foot_gather_row(F, row, fin);
    if (F.w[FW_AIR_TIME] != 0.0f) {
#pragma unroll
      for (int i = 0; i < 4; i++) t[i] = air(i);
    }
  }
  RewardIn in;
  if (earns) {
    reward_gather_row(R, row, in);
    if (reward_needs_u(R)) {
#pragma unroll
      for (int j = 0; j < 12; j++) in.u[j] = u(j);
    }
    if (reward_needs_a(R)) {
#pragma unroll
      for (int j = 0; j < 12; j++) { in.a[j] = a(j); in.a_prev[j] = a_prev(j); }
    }
  }
  {
#pragma clang fp contract(off)
    if constexpr (FEET) {
      if (earns) return foot_reward_step(R, F, in, fin, terminated, t);
      (void)foot_sum(F, fin, R.dt, 0.0f, t); /* the state advances, nothing is earned */
      return 0.0f;
    } else {
      return reward_step(R, in, terminated);
    }
  }
}

/* plain memory access: the host, and whatever no other wavefront writes while the kernel runs */
struct LearnPlain {
  __host__ __device__ static int ld(const int32_t* p) { return *p; }
  __host__ __device__ static float ld(const float* p) { return *p; }
  __host__ __device__ static int ld_u8(const uint8_t* p) { return (int)*p; }
  __host__ __device__ static void st(int32_t* p, const int v) { *p = v; }
  __host__ __device__ static void st(float* p, const float v) { *p = v; }
};
#if defined(__HIPCC__)
/* a flag byte that another wavefront stored earlier in this launch: device scope, as ld_pub (the vector L1 may hold the byte's old line) */
__device__ __forceinline__ int ld_pub_u8(const uint8_t* p) { return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
/* the rollout: every word of the visit is another wavefront's store of this launch, or this lane's of an earlier visit */
struct LearnPub {
  __device__ static int ld(const int32_t* p) { return ld_pub(p); }
  __device__ static float ld(const float* p) { return ld_pub(p); }
  __device__ static int ld_u8(const uint8_t* p) { return ld_pub_u8(p); }
  __device__ static void st(int32_t* p, const int v) { st_pub(p, v); }
  __device__ static void st(float* p, const float v) { st_pub(p, v); }
};
#endif

/* ONE VISIT of env e at step k (head comment).  LF: a LearnFeetDev in whatever address space; row: the env's observation row after step
 * k - 1; u: the torques applied in step k - 1 [12]; held: the held policy action [12]; N: envs (the stride of rewards / dones). */
template <bool FEET, class Mem, class Block>
__host__ __device__ inline void learn_visit(const Block& LF, const float* row, const float* u, const float* held, const int e, const int k, const int D, const int N) {
  const auto& L = LF.learn;
  int ws = Mem::ld(L.wstate + e);
  float acc = Mem::ld(L.acc + e);
  if (k == 0) {
    if (L.pending && Mem::ld_u8(L.pending + e)) ws |= LEARN_RESPAWN; /* the env spends step 0 on its re-spawn */
  } else {
    const int term = Mem::ld_u8(L.terminated + e);
    const bool earns = !(ws & (LEARN_DEAD | LEARN_RESPAWN));
    FootLaw F;
    float* air = nullptr;
    if constexpr (FEET) { F = foot_law_load(LF.feet); air = LF.air_time + (size_t)e * 4; }
    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (FEET ? !(ws & LEARN_RESPAWN) : earns) {
      const RewardLaw R = reward_law_load(L.law);
      const float* const prev = L.prev + (size_t)e * 12;
      const float r = learn_step<FEET>(R, F, earns, term, [&](const int c) { return Mem::ld(row + c); }, [&](const int i) { return Mem::ld(air + i); },
                                       [&](const int j) { return Mem::ld(u + j); }, [&](const int j) { return Mem::ld(held + j); }, [&](const int j) { return Mem::ld(prev + j); }, t);
      {
#pragma clang fp contract(off)
        if (earns) acc = acc + r;
      }
      if (earns && term) ws |= LEARN_DEAD | LEARN_DONE;
    }
    if constexpr (FEET) {
      if (F.w[FW_AIR_TIME] != 0.0f) { /* (t is still zero at the env's re-spawn step) */
#pragma unroll
        for (int i = 0; i < 4; i++) Mem::st(air + i, t[i]);
      }
    }
    ws = (ws & ~LEARN_RESPAWN) | (term ? LEARN_RESPAWN : 0);
    if (k % D == 0) { /* the window k / D - 1 is complete */
      const size_t at = (size_t)(k / D - 1) * N + e;
      if (L.rewards) L.rewards[at] = acc;
      if (L.dones) L.dones[at] = (uint8_t)((ws & LEARN_DONE) != 0);
      acc = 0.0f;
      ws &= LEARN_RESPAWN;
    }
  }
  Mem::st(L.acc + e, acc);
  Mem::st(L.wstate + e, ws);
}
}  // namespace gq
