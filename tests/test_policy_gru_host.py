"""The recurrent policy without a GPU (gym_quadruped_amd/policy.py GruPolicy, csrc/gq_policy_gru.h, include/gq.h GqPolicyGru): the packed
blob, the law's definition (gru_row_forward in tests/policy_gru_host.cpp, a stand-alone g++ program) against float64 under a derived bound,
the torch import, the episode rule played on the host, and the new struct and entry points of the ABI."""
import ctypes

import numpy as np
import pytest

import policy_gru_ref as R

CASES = [(shape, act, out) for shape in ('odd', 'wide', 'minimal') for act, out in (('elu', None), ('tanh', 'tanh'), ('relu', None))]


@pytest.mark.parametrize('shape', ['odd', 'wide', 'minimal'])
def test_pack_follows_the_layout_formula_and_padded_hidden_columns_stay_zero(shape):
    p = R.make_policy(shape)
    blob = p.pack()
    assert blob.dtype == np.float32 and blob.size == p.blob_floats()
    rng = np.random.default_rng(3)
    at, used = 0, np.zeros(blob.size, dtype=bool)
    H = p.hidden
    # the documented order: W_ir b_ir | W_hr b_hr | W_iz b_iz | W_hz b_hz | W_in b_in | W_hn b_hn, then the head's layers
    order = []
    for g in range(3):
        order += [(p.w_ih[:, g * H:(g + 1) * H], p.b_ih[g * H:(g + 1) * H]), (p.w_hh[:, g * H:(g + 1) * H], p.b_hh[g * H:(g + 1) * H])]
    order += list(zip(p.head_weights, p.head_biases))
    assert order[0][0].shape == (p.in_dim, H) and order[1][0].shape == (H, H) and order[6][0].shape[0] == H
    for w, b in order:
        k, n = w.shape
        kp, npad = (k + 3) & ~3, (n + 15) & ~15
        idx = lambda kk, o: at + ((o >> 4) * (kp // 4) + (kk >> 2)) * 64 + (kk & 3) * 16 + (o & 15)   # include/gq.h
        ks, os_ = rng.integers(0, k, 200), rng.integers(0, n, 200)
        for kk, o in list(zip(ks, os_)) + [(0, 0), (k - 1, n - 1), (k - 1, 0), (0, n - 1)]:
            assert blob[idx(kk, o)] == w[kk, o]
        kk, o = np.meshgrid(np.arange(k), np.arange(n), indexing='ij')
        used[idx(kk, o).reshape(-1)] = True
        assert np.array_equal(blob[at + npad * kp:at + npad * kp + n], b)
        used[at + npad * kp:at + npad * kp + n] = True
        at += npad * (kp + 1)
    assert at == blob.size and not blob[~used].any(), 'every word that is no weight and no bias is zero'
    # a step from a zero-padded h: the columns behind H come out EXACTLY 0 (sig(0) = 0.5, n = 0, h' = fmaf(0.5, 0, 0)), which the head's padding relies on
    rows, h = R.rows_for(p, 9)
    _, hn = R.host_forward(p, rows, h)
    assert hn.shape[1] == (H + 15) & ~15 and hn.shape[1] > H or H % 16 == 0
    assert np.array_equal(hn[:, H:].view(np.uint32), np.zeros_like(hn[:, H:], dtype=np.uint32)), 'padded hidden columns are +0'
    assert np.abs(hn[:, :H]).min() > 0


@pytest.mark.parametrize('shape,act,out', CASES)
def test_row_forward_is_within_the_derived_bound_of_float64(shape, act, out):
    p = R.make_policy(shape, act, out)
    rows, h = R.rows_for(p, 24)
    a, hn = R.host_forward(p, rows, h)
    (ra, rh), (ea, eh) = R.step_bound(p, rows, h)
    want_a, want_h = p.reference(rows, h)
    assert np.abs(ra - want_a).max() < 1e-12 and np.abs(rh - want_h).max() < 1e-12, 'the bound is evaluated on reference() (float64: gate by gate or in one product)'
    err_a, err_h = np.abs(a - ra), np.abs(hn[:, :p.hidden] - rh)
    print(f'{shape} {act} {out}: worst error / bound: actions {float((err_a / ea).max()):.2e}, hidden {float((err_h / eh).max()):.2e}; '
          f'allowances sig {R.sig_allowance():.3f}, tanh {R.M.activation_allowance("tanh"):.3f} x 2^-24')
    assert (err_h <= eh).all(), float((err_h / eh).max())
    assert (err_a <= ea).all(), float((err_a / ea).max())
    assert float(err_h.max()) > 0, 'float32 against float64: some rounding shows'


def test_sig_error_is_measured_and_small():
    """the ratio the gate bounds are built on, measured as activation_error measures elu and tanh (profiles/gru_policy_law_error.txt)"""
    r = R.sig_error()
    print(f'sig: {r:.4f} x 2^-24 max(1, |y|)')
    assert r < 4.0
    x = np.asarray([0.0, -0.0, 100.0, -100.0, np.inf, -np.inf], dtype=np.float32)
    assert np.array_equal(R.host_sig(x), np.asarray([0.5, 0.5, 1.0, 0.0, 1.0, 0.0], dtype=np.float32))


def test_from_torch_agrees_with_torch_and_refuses_what_it_does_not_know():
    import torch
    import torch.nn as nn
    from gym_quadruped_amd.policy import GruPolicy
    torch.manual_seed(0)
    cell, head = nn.GRUCell(49, 20), nn.Sequential(nn.Linear(20, 33), nn.ELU(), nn.Linear(33, 12), nn.Tanh())
    p = GruPolicy.from_torch(cell, head, feed_last_action=True)
    assert (p.in_dim, p.in_obs, p.hidden, p.widths, p.activation, p.out_activation) == (49, 37, 20, [33, 12], 'elu', 'tanh')
    rows, h = R.rows_for(p, 24)
    with torch.no_grad():
        th = cell.double()(torch.from_numpy(rows).double(), torch.from_numpy(h).double())
        ta = head.double()(th).numpy()
        th = th.numpy()
    cell.float(), head.float()
    ra, rh = p.reference(rows, h)
    assert np.abs(ra - ta).max() < 1e-12 and np.abs(rh - th).max() < 1e-12
    a, hn = R.host_forward(p, rows, h)
    _, (ea, eh) = R.step_bound(p, rows, h)
    assert (np.abs(a - ta) <= ea).all() and (np.abs(hn[:, :20] - th) <= eh).all(), 'the law agrees with torch.nn.GRUCell + head within the derived bound'
    # a one-layer unidirectional GRU holds the same cell
    gru = nn.GRU(49, 20, num_layers=1)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(cell.weight_ih); gru.weight_hh_l0.copy_(cell.weight_hh); gru.bias_ih_l0.copy_(cell.bias_ih); gru.bias_hh_l0.copy_(cell.bias_hh)
    assert np.array_equal(GruPolicy.from_torch(gru, head, feed_last_action=True).pack(), p.pack())
    nb = GruPolicy.from_torch(nn.GRUCell(24, 8, bias=False), nn.Sequential(nn.Linear(8, 12)))
    assert not nb.b_ih.any() and not nb.b_hh.any() and nb.widths == [12]
    ok_head = nn.Sequential(nn.Linear(20, 12))
    for bad_cell in (nn.GRU(49, 20, num_layers=2), nn.GRU(49, 20, bidirectional=True), nn.LSTMCell(49, 20), nn.RNNCell(49, 20), nn.Linear(49, 20), nn.GRUCell(49, 129),
                     nn.GRUCell(257, 20)):
        with pytest.raises(ValueError):
            GruPolicy.from_torch(bad_cell, ok_head if getattr(bad_cell, 'hidden_size', 20) == 20 else nn.Sequential(nn.Linear(129, 12)))
    for bad_head in (nn.Sequential(nn.Linear(20, 16), nn.Sigmoid(), nn.Linear(16, 12)), nn.Sequential(nn.Linear(20, 16), nn.ReLU(), nn.LayerNorm(16), nn.Linear(16, 12)),
                     nn.Linear(20, 12), nn.Sequential(nn.Linear(20, 11)), nn.Sequential(nn.Linear(21, 12)), nn.Sequential(nn.Linear(20, 300), nn.ReLU(), nn.Linear(300, 12)),
                     nn.Sequential(*[m for _ in range(3) for m in (nn.Linear(20, 20), nn.ReLU())], nn.Linear(20, 12))):
        with pytest.raises(ValueError):
            GruPolicy.from_torch(nn.GRUCell(49, 20), bad_head)


@pytest.mark.parametrize('closing', [False, True])
def test_episode_rule_on_hand_made_flag_sequences(closing):
    """gru_episode_rule played by the C++ routine over two consecutive calls (D = 4, K = 8): the rows fed at every policy step and left after
    each call are zero exactly where a ten-line loop says, and h_in[s + 1] == 0 <=> window s contained a termination"""
    D, K, H, n = 4, 8, 3, 7
    term = np.zeros((2, K, n), dtype=np.int32)
    pend = np.zeros((2, n), dtype=np.int32)
    term[0, 3, 0] = 1                      # env 0: a fall in the last substep of a window
    term[0, 1, 1] = 1                      # env 1: a fall mid-window
    term[0, 4, 2] = term[0, 6, 2] = 1      # env 2: two falls in one window (step 5 is the re-spawn)
    term[0, 7, 3] = 1                      # env 3: a fall in the last step of a call ...
    pend[0, 4] = 1                         # env 4: waiting for its re-spawn at k = 0 of the first call
    term[1, 2, 5] = term[1, 7, 5] = 1      # env 5: falls in both windows of the second call; env 6: none
    pend[1] = term[0, K - 1]               # ... which leaves the env pending before the next call
    fed, after = R.host_rule(pend, term, H, D, closing)
    zero_fed, zero_after = R.rule_expectation(pend, term, D, closing)
    assert fed.shape == (2, K // D, n, H) and after.shape == (2, n, H)
    assert np.array_equal((fed == 0).all(axis=3), zero_fed) and np.array_equal((fed != 0).all(axis=3), ~zero_fed), 'a row is all zero or has no zero'
    assert np.array_equal((after == 0).all(axis=2), zero_after) and np.array_equal((after != 0).all(axis=2), ~zero_after)
    # the rows that were not zeroed are what the cell left: 1 before the first step, then 2 + the index of the previous policy step
    seq = fed.reshape(2 * (K // D), n, H)
    for s in range(seq.shape[0]):
        assert np.array_equal(seq[s][seq[s] != 0], np.full(int((seq[s] != 0).sum()), 1.0 if s == 0 else 1.0 + s, dtype=np.float32))
    # h_in[s + 1] == 0 <=> a termination in window s, over both calls (the boundary between them included); h_in[0] == 0 <=> pending
    windows = term.reshape(2 * (K // D), D, n).any(axis=1)
    zf = zero_fed.reshape(2 * (K // D), n)
    assert np.array_equal(zf[1:], windows[:-1]) and np.array_equal(zf[0], pend[0].astype(bool))
    assert zf[:, 6].sum() == 0 and zf[1, 0] and zf[1, 1] and zf[2, 2] and zf[2, 3] and zf[0, 4] and zf[3, 5]
    # the state after a call: the closing visit zeroes the env that fell in the last step; the plain mode leaves it to the next call's k == 0
    assert bool(zero_after[0, 3]) == closing and bool(zero_after[1, 5]) == closing and not zero_after[:, 6].any()


def test_policy_gru_struct_and_exports_are_in_the_abi_and_the_version_stays():
    from gym_quadruped_amd import _lib, cabi
    # (layout and export against the header: tests/test_host_and_abi.py discovers every struct and symbol)
    assert 'gq_rollout_policy_gru' in _lib.EXPORTS and 'gq_policy_gru_eval' in _lib.EXPORTS
    g = cabi.GqPolicyGru
    assert [f[0] for f in g._fields_] == ['struct_size', 'hidden', 'blob', 'blob_floats', 'hidden_state', 'hidden_seq'] and ctypes.sizeof(g) == 40
    assert (g.hidden.offset, g.blob.offset, g.blob_floats.offset, g.hidden_state.offset, g.hidden_seq.offset) == (4, 8, 16, 24, 32)
    assert _lib.LIB_PATH.exists(), 'build the HIP extension first (__graft_entry__.build())'
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert L.gq_version() == 660 and cabi.GQ_ABI_VERSION == 660
    assert L.gq_rollout_policy_gru and L.gq_policy_gru_eval
    # a stale binding of either struct is refused before anything else is looked at (no device is touched: the handle is never reached)
    L.gq_last_error.restype = ctypes.c_char_p
    L.gq_policy_gru_eval.argtypes = _lib.ABI['gq_policy_gru_eval'][1]
    m = cabi.GqPolicyMlp(struct_size=ctypes.sizeof(cabi.GqPolicyMlp), n_layers=1)
    stale = g(struct_size=ctypes.sizeof(g) - 8, hidden=8)
    assert L.gq_policy_gru_eval(None, ctypes.byref(m), ctypes.byref(stale), None, None, 0, 0, None, None, None) == -1
    assert b'GqPolicyGru' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
    m.struct_size -= 8
    assert L.gq_policy_gru_eval(None, ctypes.byref(m), ctypes.byref(g(struct_size=ctypes.sizeof(g), hidden=8)), None, None, 0, 0, None, None, None) == -1
    assert b'GqPolicyMlp' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
