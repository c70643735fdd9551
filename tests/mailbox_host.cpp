/*
 * TEST INFRASTRUCTURE - the closed-loop rollout's mailbox protocol (gym_quadruped_amd/csrc/gq_mailbox.h) on the host: a stand-alone program
 * around the header's own functions and text, compiled with g++ against the emulator's shim (tests/simt_emu on the include path, where
 * ld_pub / st_pub / add_pub are plain memory operations).  It prints a report of `key value...` lines that tests/test_mailbox_host.py reads;
 * nothing here decides what passes.
 *
 *   mailbox_host            the whole report
 *
 * What runs: the item word over every lap boundary of four queue sizes; the envs of a queue; the host's clamps of the two grids and the
 * 32-bit bound; the three waits (GQ_MB_WAIT_ITEM, GQ_MB_POLICY_REGISTER, GQ_MB_POLICY_IDLE) as ONE wavefront sees them, abort codes
 * included; and the lap rule as a SEQUENTIAL MODEL of one queue - see lap_model below for what the model assumes.  Concurrency itself
 * (several wavefronts, memory visibility) is not modelled: that stays with the GPU tests.
 */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gq_mailbox.h"

/* what the shim declares for its coroutine wavefront: one lane here, nothing to switch to */
EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
void emu_yield() {}
uint32_t emu_slot[2][GQ_WAVE];
int emu_phase[GQ_WAVE];

using namespace gq;

static constexpr int64_t kTicketBound = ((int64_t)1 << 31) - 65536; /* the issue's figure, restated: MB_MAX_TICKETS is compared with it */

/* ---- item word: for every lap boundary L * qcap below the ticket bound, the push tickets around it, four envs each */
static void item_round_trip() {
  const int qcaps[4] = {64, 128, 4096, 1 << 21};
  for (const int qcap : qcaps) {
    const int qshift = __builtin_ctz(qcap);
    const int envs[4] = {0, 1, qcap - 1 /* N - 1 of the largest batch this queue size serves */, (1 << 24) - 2};
    long long cases = 0, bad_env = 0, bad_own = 0, bad_neighbour = 0, bad_wrap = 0, empty_accepted = 0;
    for (int64_t edge = 0; edge < kTicketBound; edge += qcap) {
      for (int d = -1; d <= 1; d++) {
        const int64_t s64 = edge + d;
        if (s64 < 0 || s64 >= kTicketBound) continue;
        const int s = (int)s64;
        for (const int e : envs) {
          const int item = mb_item(s, qshift, e);
          cases++;
          bad_env += mb_item_env(item) != e;
          bad_own += !mb_item_is(item, s, qshift);
          /* the tickets that wait on the same slot one lap earlier / later must not take it */
          if (s64 - qcap >= 0) bad_neighbour += mb_item_is(item, s - qcap, qshift);
          if (s64 + qcap < kTicketBound) bad_neighbour += mb_item_is(item, (int)(s64 + qcap), qshift);
          /* ... and 128 laps later the 7-bit lap has come round (the header says so) */
          if (s64 + 128 * (int64_t)qcap < kTicketBound) bad_wrap += !mb_item_is(item, (int)(s64 + 128 * (int64_t)qcap), qshift);
        }
        /* an empty slot - never written, or a lap number without an env - is accepted by no ticket */
        empty_accepted += mb_item_is(0, s, qshift) + mb_item_is(mb_lap(s, qshift) << MB_ITEM_LAP_SHIFT, s, qshift);
      }
    }
    std::printf("item qcap %d cases %lld bad_env %lld bad_own %lld bad_neighbour %lld bad_wrap %lld empty_accepted %lld empty_env %d\n", qcap, cases, bad_env, bad_own,
                bad_neighbour, bad_wrap, empty_accepted, mb_item_env(0));
  }
}

/* ---- counters and the envs of a queue */
static void queues() {
  const int Ns[6] = {1, 7, 63, 65, 1000, 4096}, nqs[4] = {1, 2, 4, 8};
  for (const int N : Ns)
    for (const int nq : nqs) {
      int sum = 0, most = 0, members = 0;
      for (int q = 0; q < nq; q++) {
        const int n = mb_queue_envs(N, q, nq);
        sum += n; most = n > most ? n : most;
        for (int i = 0; i < n; i++) members += (q + nq * i < N) && ((q + nq * i) % nq == q); /* e = q + nq * i are envs of the batch, and of this queue */
      }
      std::printf("queue N %d nq %d sum %d members %d max %d bound %d tickets7 %lld\n", N, nq, sum, members, most, mb_queue_envs(N, 0, nq),
                  (long long)mb_queue_tickets(N, 0, nq, 7));
    }
  int32_t base[1];
  std::printf("ctr stride %d words8 %zu pop2 %td push2 %td policy2 %td\n", GQ_MB_QSTRIDE, mb_ctr_words(8), mb_ctr(base, 2, MB_CTR_POP) - base,
              mb_ctr(base, 2, MB_CTR_PUSH) - base, mb_ctr(base, 2, MB_CTR_POLICY) - base);
  std::printf("fits envs_max %d envs_over %d steps_max %d steps_over %d bound_equal %d\n", (int)mb_rollout_fits((1 << 24) - 1, 8, 1), (int)mb_rollout_fits(1 << 24, 8, 1),
              (int)mb_rollout_fits(4096, 8, 4194175), (int)mb_rollout_fits(4096, 8, 4194176), (int)(MB_MAX_TICKETS == kTicketBound));
}

/* ---- the host's clamps */
static void clamps() {
  const int nqs[4] = {1, 2, 4, 8}, asked[4] = {0, 1, 100, 4096};
  for (const int nq : nqs)
    for (const int a : asked)
      std::printf("policy_waves nq %d asked %d pd %d mlp %d\n", nq, a, mb_policy_waves(a, 64, 256, nq), mb_policy_waves(a, 128, 1024, nq));
  const int Ns[6] = {1, 7, 9, 63, 65, 4096}, sw[3] = {0, 1, 2048};
  for (const int nq : nqs)
    for (const int N : Ns)
      for (const int a : sw) std::printf("step_waves nq %d N %d asked %d got %d\n", nq, N, a, mb_step_waves(a, N, nq));
}

/* ---- the three waits, as one wavefront (lane 0) sees them.  The shim's clock advances 100 ticks per look. */
struct Rig {
  int32_t status[8] = {}, ctr[2 * MB_CTR_COUNT * GQ_MB_QSTRIDE] = {}, items[64] = {}, alive = 0;
  MailboxDev MB{};
  Rig() { MB.status = status; MB.q_ctr = ctr; MB.q_items = items; MB.alive = &alive; MB.qcap = 64; MB.timeout_ticks = 5000; }
};
/* 1: the item came, env in *out; 0: left */
static int wait_item(Rig& r, const int ticket, int* out) {
  const MailboxDev& MB = r.MB;
  const int32_t* const items = r.items;
  const int qmask = 63, qshift = 6;
  GQ_MB_WAIT_ITEM(env, return 0;)
  *out = env;
  return 1;
}
/* 1: registered; 0: returned from the "kernel" */
static int policy_register_done = 0, policy_rank = -1, policy_mine = -1;
static void policy_register(Rig& r, const int nq, const int q) {
  const MailboxDev& MB = r.MB;
  const int lane = 0;
  policy_register_done = 0;
  GQ_MB_POLICY_REGISTER()
  (void)t_last;
  policy_register_done = 1; policy_rank = rank; policy_mine = mine;
}
/* passes of an idle policy loop until it breaks */
static int policy_idle(Rig& r, const bool writer, const int who) {
  const MailboxDev& MB = r.MB;
  const long long t_last = wall_clock64();
  int passes = 0;
  for (;; passes++) {
    GQ_MB_POLICY_IDLE(writer, who)
  }
  return passes;
}
static void waits() {
  threadIdx.x = 0;
  {
    Rig r; int env = -2;
    r.items[5] = mb_item(64 + 5, 6, 41); /* the item of push 69, in slot 5 */
    const int got = wait_item(r, 69, &env);
    std::printf("wait own_lap got %d env %d status %d\n", got, env, r.status[0]);
  }
  {
    Rig r; int env = -2;
    r.items[5] = mb_item(5, 6, 41);      /* slot 5 holds the item of the lap before: ticket 69 must wait it out, to its deadline */
    const int got = wait_item(r, 69, &env);
    std::printf("wait other_lap got %d status %d who %d\n", got, r.status[0], r.status[1]);
  }
  {
    Rig r; int env = -2;
    r.status[0] = MB_ABORT_POLICY_ABSENT; /* the abort word is up: leave, and leave the word as it is */
    const int got = wait_item(r, 3, &env);
    std::printf("wait aborted got %d status %d who %d\n", got, r.status[0], r.status[1]);
  }
  {
    Rig r;
    gridDim.x = 1; policy_register(r, 1, 0); /* the only policy wavefront, one queue */
    std::printf("register alone done %d rank %d mine %d alive %d status %d\n", policy_register_done, policy_rank, policy_mine, r.alive, r.status[0]);
  }
  {
    Rig r;
    gridDim.x = 1; policy_register(r, 2, 0); /* two queues, and queue 1 got no policy wavefront */
    std::printf("register no_policy done %d status %d who %d\n", policy_register_done, r.status[0], r.status[1]);
  }
  {
    Rig r;
    gridDim.x = 2; policy_register(r, 1, 0); /* the second wavefront of the launch never reports in */
    std::printf("register deadline done %d status %d who %d\n", policy_register_done, r.status[0], r.status[1]);
  }
  {
    Rig r;
    const int passes = policy_idle(r, true, 77);
    std::printf("idle deadline passes_gt0 %d status %d who %d\n", (int)(passes > 0), r.status[0], r.status[1]);
  }
  {
    Rig r;
    const int passes = policy_idle(r, false, 77); /* not the lane that speaks for the wavefront */
    std::printf("idle silent passes_gt0 %d status %d\n", (int)(passes > 0), r.status[0]);
  }
  {
    Rig r;
    r.status[0] = MB_ABORT_STEP_DEADLINE;
    const int passes = policy_idle(r, true, 77);
    std::printf("idle aborted passes %d status %d who %d\n", passes, r.status[0], r.status[1]);
  }
}

/* ---- the lap rule, as a sequential model of one queue (qcap 64).
 * R step wavefronts hold pop tickets 0 .. R - 1 before anything is pushed (R > qcap: a small batch under thousands of resident step
 * wavefronts); a reader that takes an item draws the next pop ticket, as mailbox_step_body does.  E envs are pushed in ticket order with the
 * header's producer (mb_push_ticket, mb_push_item), K times each, an env again only after its item was taken.
 * THE MODEL'S CONDITION: between any two pushes every outstanding reader looks at its slot once.  This fairness is the DELIVERY ASSUMPTION of
 * gq_mailbox.h - a ticket holder polls far more often than qcap pushes pass - put in by construction: the model does not measure it, and
 * says nothing about a reader that stays away for a lap.
 * lapless: the acceptance test replaced by "slot non-empty" - what the protocol would be without the lap number. */
static void lap_model(const int R, const bool lapless) {
  const int qcap = 64, qmask = qcap - 1, qshift = 6, E = 5, K = 1700, P = E * K; /* P = 8500 pushes: past 128 laps, where the lap number wraps */
  std::vector<int32_t> items(qcap, 0);
  int32_t tail = 0, pop = 0;
  std::vector<int> slot_push(qcap, -1), taken(P, 0), pushed_of(E, 0), reader(R);
  std::vector<char> ready(E, 1);
  for (int r = 0; r < R; r++) reader[r] = pop++;
  long long n_taken = 0, wrong_item = 0, double_take = 0, early = 0, rounds = 0;
  int pushes = 0, next_env = 0;
  while (n_taken < P && rounds < 4LL * P + 1000) {
    rounds++;
    for (int i = 0; i < E && pushes < P; i++) { /* one push: the next env, round-robin, that is ready and has steps left */
      const int e = (next_env + i) % E;
      if (!ready[e] || pushed_of[e] >= K) continue;
      const int s = mb_push_ticket(&tail);
      mb_push_item(items.data(), qmask, qshift, s, e);
      slot_push[s & qmask] = s; ready[e] = 0; pushed_of[e]++; pushes++; next_env = (e + 1) % E;
      break;
    }
    for (int r = 0; r < R; r++) { /* every outstanding reader looks once */
      const int t = reader[r];
      if (t >= P) continue; /* the queue's total is claimed: this wavefront has left */
      const int item = items[t & qmask];
      const bool accept = lapless ? mb_item_env(item) >= 0 : mb_item_is(item, t, qshift);
      if (!accept) continue;
      const int s = slot_push[t & qmask], e = mb_item_env(item);
      if (s != t) wrong_item++;       /* the ticket took the item of a push with another number */
      if (t >= pushes) early++;       /* ... of a push that has not happened */
      if (++taken[s] > 1) double_take++; /* the env of push s is being stepped by two wavefronts */
      else { n_taken++; ready[e] = 1; }
      reader[r] = pop++;
    }
  }
  int each_once = 1;
  for (int s = 0; s < P; s++) each_once &= taken[s] == 1;
  std::printf("lap_model R %d lapless %d pushes %d taken %lld wrong_item %lld double_take %lld early %lld each_once %d\n", R, (int)lapless, pushes, n_taken, wrong_item,
              double_take, early, each_once);
}

int main() {
  item_round_trip();
  queues();
  clamps();
  waits();
  const int Rs[4] = {1, 64, 65, 256};
  for (const int R : Rs) lap_model(R, false);
  for (const int R : Rs) lap_model(R, true);
  return 0;
}
