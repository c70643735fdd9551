"""The closed-loop rollout's mailbox protocol without a GPU (gym_quadruped_amd/csrc/gq_mailbox.h, the one definition the step kernel, the
policy kernels and the host share): tests/mailbox_host.cpp - a stand-alone g++ program around the header's own functions and text, built
against the emulator's shim - is built and run once, and its report is held to the numbers the protocol states.  What it cannot show is
concurrency itself: several wavefronts and memory visibility stay with tests/test_gpu_closed_loop.py and the policy rollouts' GPU tests."""
import subprocess
import tempfile
import time
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
TICKET_BOUND = 2 ** 31 - 65536
QCAP = 64   # of the lap model


@pytest.fixture(scope='module')
def report():
    """{first word: [the rest of each such line, as {key: int}]}"""
    with tempfile.TemporaryDirectory() as d:
        exe = Path(d) / 'mailbox_host'
        subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Wno-unknown-pragmas', '-Wno-unused-function', '-I', str(ROOT / 'tests' / 'simt_emu'),
                        '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'), '-o', str(exe), str(ROOT / 'tests' / 'mailbox_host.cpp')], check=True)
        t0 = time.perf_counter()
        text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
        print(f'mailbox_host ran {time.perf_counter() - t0:.2f} s')
    out = {}
    for line in text.splitlines():   # `head [case] key value key value ...`
        print(line)
        head, *rest = line.split()
        if len(rest) % 2:
            head, rest = f'{head} {rest[0]}', rest[1:]
        out.setdefault(head, []).append({k: int(v) for k, v in zip(rest[::2], rest[1::2])})
    return out


def test_item_word_round_trips_over_every_lap_boundary(report):
    """qcap in {64, 128, 4096, 2^21}; envs 0, 1, N - 1, 2^24 - 2; the push tickets s - 1, s, s + 1 around every lap boundary s = L qcap below
    the 2^31 - 65536 bound: mb_item_env gives the env back, the ticket with the push's number accepts the item, the tickets that wait on the
    same slot one lap earlier and later do not, and no ticket accepts an empty slot"""
    rows = {r['qcap']: r for r in report['item']}
    assert sorted(rows) == [64, 128, 4096, 2 ** 21]
    for qcap, r in rows.items():
        edges = -(-TICKET_BOUND // qcap)
        assert r['cases'] == 4 * (3 * edges - 1), 'every boundary, three tickets each but for ticket -1, four envs'
        assert r['bad_env'] == 0 and r['bad_own'] == 0 and r['bad_neighbour'] == 0
        assert r['bad_wrap'] == 0, 'after 128 laps the 7-bit lap number comes round: the header says so, the delivery assumption covers it'
        assert r['empty_accepted'] == 0 and r['empty_env'] == -1


def test_queue_envs_sum_to_the_batch_and_queue_0_holds_the_most(report):
    rows = report['queue']
    assert {(r['N'], r['nq']) for r in rows} == {(N, nq) for N in (1, 7, 63, 65, 1000, 4096) for nq in (1, 2, 4, 8)}
    for r in rows:
        assert r['sum'] == r['N'] == r['members']
        assert r['bound'] == r['max'] == -(-r['N'] // r['nq']), 'the host checks the ticket bound on queue 0: it is the fullest'
        assert r['tickets7'] == 7 * r['bound']
    (c,) = report['ctr']
    assert c == dict(stride=32, words8=8 * 3 * 32, pop2=6 * 32, push2=7 * 32, policy2=8 * 32), 'q_ctr + (3 q + i) * GQ_MB_QSTRIDE, i = pop, push, policy'
    (f,) = report['fits']
    assert f == dict(envs_max=1, envs_over=0, steps_max=1, steps_over=0, bound_equal=1), 'N <= 2^24 - 1 and 512 envs x n_steps < 2^31 - 65536'


# The clamps, restated from the rollouts' inline code before the header: policy wavefronts default 64 (PD) / 128 (MLP), cap 256 / 1024, at
# least 2 nq; step workgroups default N, at least 4 nq.
def _policy(asked, dflt, cap, nq):
    w = dflt if asked <= 0 else asked
    return max(min(w, cap), 2 * nq)


def test_policy_wave_clamp(report):
    rows = report['policy_waves']
    assert len(rows) == 16
    for r in rows:
        assert r['pd'] == _policy(r['asked'], 64, 256, r['nq']) and r['mlp'] == _policy(r['asked'], 128, 1024, r['nq'])
    at8 = {r['asked']: (r['pd'], r['mlp']) for r in rows if r['nq'] == 8}
    assert at8 == {0: (64, 128), 1: (16, 16), 100: (100, 100), 4096: (256, 1024)}, 'an MI355X in SPX mode shows 8 XCDs'


def test_step_wave_clamp(report):
    rows = report['step_waves']
    assert len(rows) == 4 * 6 * 3
    for r in rows:
        want = max(r['N'] if r['asked'] <= 0 else r['asked'], 4 * r['nq'])
        assert r['got'] == want and r['got'] >= 4 * r['nq']
    got = {(r['nq'], r['N'], r['asked']): r['got'] for r in rows}
    assert got[8, 4096, 0] == 4096 and got[8, 1, 0] == 32 and got[8, 9, 2048] == 2048 and got[8, 7, 1] == 32


def test_waits_of_one_wavefront_raise_the_named_codes(report):
    """the header's three text pieces, expanded in the host program: codes 1, 2, 4 with the `who` each states; an abort word that is already
    up is left as it is"""
    assert report['wait own_lap'] == [dict(got=1, env=41, status=0)]
    assert report['wait other_lap'] == [dict(got=0, status=1, who=69)], 'the item of the lap before is never taken: the ticket waits to its deadline'
    assert report['wait aborted'] == [dict(got=0, status=3, who=0)]
    assert report['register alone'] == [dict(done=1, rank=0, mine=1, alive=1, status=0)]
    assert report['register no_policy'] == [dict(done=0, status=4, who=1)]
    assert report['register deadline'] == [dict(done=0, status=2, who=-1)]
    assert report['idle deadline'] == [dict(passes_gt0=1, status=2, who=77)]
    assert report['idle silent'] == [dict(passes_gt0=1, status=0)]
    assert report['idle aborted'] == [dict(passes=0, status=1, who=0)]


def test_abort_codes_have_their_public_names():
    """include/gq.h GQ_CLOSED_ABORT_* and cabi.GQ_CLOSED_ABORT name the values the header's enum has (gq_api.hip holds the header to gq.h
    with a static_assert; the program above shows the header's values)"""
    import abi_layout
    from gym_quadruped_amd import cabi
    names = {f'GQ_CLOSED_ABORT_{k.upper()}': v for k, v in cabi.GQ_CLOSED_ABORT.items()}
    header = abi_layout.header_constants()
    assert names == {k: header[k] for k in names} == dict(GQ_CLOSED_ABORT_STEP_DEADLINE=1, GQ_CLOSED_ABORT_POLICY_DEADLINE=2, GQ_CLOSED_ABORT_POLICY_ABSENT=3,
                                                           GQ_CLOSED_ABORT_XCD_NO_POLICY=4)


@pytest.mark.parametrize('R', [1, QCAP, QCAP + 1, 4 * QCAP])
def test_lap_rule_gives_every_ticket_the_push_with_its_number(report, R):
    """A sequential model of one queue, qcap 64: R pop tickets are outstanding before any push; 5 envs are pushed with the header's producer in
    ticket order, 1700 times each (8500 pushes: past the 128 laps after which the lap number wraps), an env again only after its item was
    taken.  CONDITION OF THE MODEL, not a measurement: every outstanding reader looks at its slot between any two pushes - the delivery
    assumption of gq_mailbox.h (a ticket holder polls far more often than qcap pushes pass), put in by construction."""
    (r,) = [x for x in report['lap_model'] if x['R'] == R and x['lapless'] == 0]
    assert r['pushes'] == 8500 and r['taken'] == r['pushes'], 'as many items taken as pushed'
    assert r['wrong_item'] == 0 and r['early'] == 0 and r['each_once'] == 1, 'every ticket takes exactly the item of the push with its own number'
    assert r['double_take'] == 0, 'no env is taken twice'


@pytest.mark.parametrize('R', [QCAP + 1, 4 * QCAP])
def test_the_model_without_the_lap_number_double_takes(report, R):
    """the same model with the acceptance test replaced by `slot non-empty`: with more outstanding tickets than slots two of them wait on one
    slot and both take its item - the model can fail, and the lap number is what keeps it from failing"""
    (r,) = [x for x in report['lap_model'] if x['R'] == R and x['lapless'] == 1]
    print(f'lap-less model, R = {R}: {r["double_take"]} double takes, {r["wrong_item"]} items taken by a ticket with another number')
    assert r['double_take'] > 0
