"""The observation history without a GPU (gym_quadruped_amd/policy.py ObsHistory, csrc/gq_policy_hist.h, include/gq.h GqPolicyHist): the
store, the episode rule and the push played on the host against a ten-line numpy reference, the input row's accounting and its refusals,
the torch import, and the new struct and entry point of the ABI."""
import ctypes

import numpy as np
import pytest

import policy_hist_ref as R


def _sequences():
    """the hand-made two-call sequences of test_policy_gru_host.py::test_episode_rule_on_hand_made_flag_sequences (D = 4, K = 8, n = 7)"""
    D, K, n = 4, 8, 7
    term = np.zeros((2, K, n), dtype=np.int32)
    pend = np.zeros((2, n), dtype=np.int32)
    term[0, 3, 0] = 1                      # env 0: a fall in the last substep of a window
    term[0, 1, 1] = 1                      # env 1: a fall mid-window
    term[0, 4, 2] = term[0, 6, 2] = 1      # env 2: two falls in one window (step 5 is the re-spawn)
    term[0, 7, 3] = 1                      # env 3: a fall in the last step of a call ...
    pend[0, 4] = 1                         # env 4: waiting for its re-spawn at k = 0 of the first call
    term[1, 2, 5] = term[1, 7, 5] = 1      # env 5: falls in both windows of the second call; env 6: none
    pend[1] = term[0, K - 1]               # ... which leaves the env pending before the next call
    return D, K, n, pend, term


def test_the_slot_index_by_multiplication_is_the_division():
    assert R.host_div_mismatches() == 0, '(hc * ceil(2^16 / F)) >> 16 == hc // F for every F in 1 .. 256 and hc in 0 .. 255'


@pytest.mark.parametrize('closing', [False, True])
@pytest.mark.parametrize('L', [1, 2, 3])
def test_store_rule_and_push_on_hand_made_flag_sequences(L, closing):
    """the header's routines over two consecutive calls: the rows fed and the store after each call equal the reference word for word - every
    word is marked by env, step and place, so a misplaced one shows - and the history fed at s + 1 is zero exactly where window s fell"""
    D, K, n, pend, term = _sequences()
    F, S = 5, K // D
    hist0, cur = R.marks(n, L, F, 2 * S)
    got_cur, got_fed, got_after, ctl = R.host_play(pend, term, L, F, D, closing)
    assert np.array_equal(got_cur.reshape(2 * S, n, F), cur)
    hist = hist0
    for c in range(2):
        fed, hist = R.fed_history(cur[c * S:(c + 1) * S], hist, pend[c], term[c], D, closing)
        assert np.array_equal(got_fed[c], fed), f'call {c}: the frames fed'
        assert np.array_equal(got_after[c], hist), f'call {c}: the store after the call'
    # (the store wraps: with K / D = 2 policy steps per call every one of the L <= 3 slots has been replaced after the two calls)
    fed_all = got_fed.reshape(2 * S, n, L * F)
    windows = term.reshape(2 * S, D, n).any(axis=1)
    zero = (fed_all == 0).all(axis=2)
    assert np.array_equal(zero[1:], windows[:-1]) and np.array_equal(zero[0], pend[0].astype(bool)), 'fed[s + 1] == 0 <=> a termination in window s'
    nz = fed_all[1:][~zero[1:]].reshape(-1, L, F)[:, 0]
    assert (nz != 0).all(), 'elsewhere the newest frame has no zero word'
    # the state after a call: the closing visit empties the env that fell in the last step; the plain mode leaves it to the next call's k == 0
    after_zero = (got_after == 0).all(axis=(2, 3))
    assert bool(after_zero[0, 3]) == closing and bool(after_zero[1, 5]) == closing and not after_zero[:, 6].any()
    assert ((ctl & ~3) == 0).all(), 'a control word is parity and VALID'


def _mlp(in_dim, rng, widths=(33, 12), **kw):
    from gym_quadruped_amd.policy import MlpPolicy
    ws, bs, k = [], [], in_dim
    for w in widths:
        ws.append((rng.standard_normal((k, w)) / np.sqrt(k)).astype(np.float32))
        bs.append((0.1 * rng.standard_normal(w)).astype(np.float32))
        k = w
    return MlpPolicy(ws, bs, **kw)


def test_in_dim_accounting_and_refusals():
    from gym_quadruped_amd.policy import GruPolicy, HeightScan, ObsHistory
    rng = np.random.default_rng(0)
    p = _mlp(144, rng, feed_last_action=True, history=ObsHistory(3))
    assert (p.in_obs, p.hist_cols, p.hist_words, p.in_dim) == (24, 24, 36, 24 + 12 + 3 * 36)
    p = _mlp(111, rng, feed_last_action=True, history=ObsHistory(3, 13))
    assert (p.in_obs, p.hist_cols, p.hist_words) == (24, 13, 25) and 24 + 12 + 3 * 25 == 111
    p = _mlp(72, rng, feed_last_action=True, history=ObsHistory(1, 24))
    assert (p.in_obs, p.hist_words) == (24, 36)
    p = _mlp(30, rng, history=ObsHistory(2, 3))
    assert (p.in_obs, p.hist_words) == (24, 3)
    p = _mlp(24 + 15 + 12 + 2 * 36, rng, feed_last_action=True, height_scan=HeightScan(3, 5), history=ObsHistory(2))
    assert (p.in_obs, p.hist_words) == (24, 36)
    assert _mlp(36, rng, feed_last_action=True).history is None
    for frames, cols, word in ((0, None, 'frames'), (-1, None, 'frames'), (1.5, None, 'frames'), (2, 0, 'cols'), (2, -3, 'cols')):
        with pytest.raises(ValueError, match=word):
            ObsHistory(frames, cols)
    with pytest.raises(ValueError, match='cols = 25'):
        _mlp(24 + 12 + 2 * 37, rng, feed_last_action=True, history=ObsHistory(2, 25))   # in_obs comes out as 24: cols > in_obs
    with pytest.raises(ValueError, match='257'):
        _mlp(257, rng, feed_last_action=True, history=ObsHistory(3))
    with pytest.raises(ValueError, match='in_dim = 145'):
        _mlp(145, rng, feed_last_action=True, history=ObsHistory(3))   # 145 - 48 is no multiple of 4
    with pytest.raises(ValueError, match='ObsHistory'):
        _mlp(144, rng, feed_last_action=True, history=3)
    H = 8
    gru = lambda **kw: GruPolicy(np.zeros((36, 3 * H)), np.zeros((H, 3 * H)), np.zeros(3 * H), np.zeros(3 * H), [np.zeros((H, 12))], [np.zeros(12)], **kw)
    assert gru(feed_last_action=True).in_obs == 24
    with pytest.raises(ValueError, match='GruPolicy takes no history'):
        gru(feed_last_action=True, history=ObsHistory(1))


def test_from_torch_on_a_history_width_first_layer_agrees_with_torch_in_float64():
    import torch
    import torch.nn as nn
    from gym_quadruped_amd.policy import MlpPolicy, ObsHistory
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    net = nn.Sequential(nn.Linear(111, 33), nn.ELU(), nn.Linear(33, 12))
    shift, scale = rng.standard_normal(24).astype(np.float32), (0.5 + rng.random(24)).astype(np.float32)
    p = MlpPolicy.from_torch(net, feed_last_action=True, history=ObsHistory(3, 13), obs_shift=shift, obs_scale=scale)
    assert (p.in_dim, p.in_obs, p.hist_words, p.widths) == (111, 24, 25, [33, 12])
    rows = rng.standard_normal((9, 111)).astype(np.float32)
    x = rows.astype(np.float64)
    x[:, :24] = (x[:, :24] - shift) * scale
    for i in range(3):   # a frame's observation words take the shift / scale of their original column, its action words none
        c0 = 36 + 25 * i
        x[:, c0:c0 + 13] = (x[:, c0:c0 + 13] - shift[:13]) * scale[:13]
    with torch.no_grad():
        want = net.double()(torch.from_numpy(x)).numpy()
    assert np.abs(p.reference(rows) - want).max() < 1e-12
    for bad, hist in ((110, ObsHistory(3)), (87, ObsHistory(3, 13))):   # no in_obs >= 1 satisfies the formula
        with pytest.raises(ValueError, match=f'in_dim = {bad}'):
            MlpPolicy.from_torch(nn.Sequential(nn.Linear(bad, 12)), feed_last_action=True, history=hist)


def test_policy_hist_struct_and_export_are_in_the_abi_and_the_version_stays():
    from gym_quadruped_amd import _lib, cabi
    # (layout and export against the header: tests/test_host_and_abi.py discovers every struct and symbol)
    assert 'gq_rollout_policy_hist' in _lib.EXPORTS
    g = cabi.GqPolicyHist
    assert [f[0] for f in g._fields_] == ['struct_size', 'frames', 'cols', 'in_dim', 'state', 'ctl'] and ctypes.sizeof(g) == 32
    assert (g.frames.offset, g.cols.offset, g.in_dim.offset, g.state.offset, g.ctl.offset) == (4, 8, 12, 16, 24)
    assert _lib.LIB_PATH.exists(), 'build the HIP extension first (__graft_entry__.build())'
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert L.gq_version() == 660 and cabi.GQ_ABI_VERSION == 660
    assert L.gq_rollout_policy_hist
    # a stale binding is refused before anything else is looked at (no device is touched: the handle is never reached)
    L.gq_last_error.restype = ctypes.c_char_p
    L.gq_rollout_policy_hist.argtypes = _lib.ABI['gq_rollout_policy_hist'][1]
    m = cabi.GqPolicyMlp(struct_size=ctypes.sizeof(cabi.GqPolicyMlp), n_layers=1)
    stale = g(struct_size=ctypes.sizeof(g) - 8, frames=1, cols=1)
    args = (0, 0, 0.0, cabi.GqState(), cabi.GqObsOut(), None, None, None, None, None, None, None, None)
    assert L.gq_rollout_policy_hist(None, 0, ctypes.byref(m), None, ctypes.byref(stale), *args) == -1
    assert b'GqPolicyHist' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
    assert L.gq_rollout_policy_hist(None, 0, ctypes.byref(m), None, None, *args) == -1 and b'gq_rollout_policy_hist' in L.gq_last_error()
