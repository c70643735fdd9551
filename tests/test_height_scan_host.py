"""The height scan without a GPU (gym_quadruped_amd/policy.py HeightScan, csrc/gq_policy_scan.h, include/gq.h GqPolicyScan): the law's
definition (height_scan_cell in tests/height_scan_host.cpp, a stand-alone g++ program) against its numpy float32 restatement bit for bit, the
input-row arithmetic of both policies, and the new struct and entry points of the ABI."""
import ctypes

import numpy as np
import pytest

import height_scan_ref as H


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_header_law_equals_the_numpy_restatement_bit_for_bit():
    rng = np.random.default_rng(7)
    n = 400
    z_base = rng.uniform(0.1, 0.7, n)
    clip = rng.uniform(0.05, 1.5, n)
    offset = rng.uniform(-0.5, 0.5, n)
    # hits spread so that a third of the records saturates on either side
    z_hit = (z_base - offset) - rng.uniform(-1.5, 1.5, n) * clip
    scale = rng.uniform(-5.0, 5.0, n)
    rec = np.stack([z_base, z_hit, offset, clip, scale], axis=1).astype(np.float32)
    f = np.float32
    zb, off, cl = f(0.3125), f(0.25), f(0.5)
    pz = f(np.float64(zb) + 0.6 - 0.07)   # the ray's origin; a ray that hits nothing lands at pz + 1
    edges = [
        (zb, (zb - off) - cl, off, cl, f(2.0)),            # d == +clip exactly
        (zb, (zb - off) + cl, off, cl, f(2.0)),            # d == -clip exactly
        (zb, np.nextafter((zb - off) - cl, f(-9)), off, cl, f(2.0)),   # just beyond +clip
        (zb, np.nextafter((zb - off) + cl, f(9)), off, cl, f(2.0)),    # just beyond -clip
        (zb, pz + f(1.0), off, cl, f(3.0)),                # the miss value: saturates at -clip
        (zb, pz + f(1.0), f(0.0), f(0.125), f(1.0)),
        (zb, f(0.01), off, cl, f(0.0)),                    # scale = 0, d > 0: +0
        (zb, f(0.9), off, cl, f(0.0)),                     # scale = 0, d < 0: -0
        (zb, zb - off, off, cl, f(-1.0)),                  # d == 0 and a negative scale: -0
        (zb, f(0.0), f(-0.4), cl, f(1.0)),                 # a negative offset raises the reference height
        (zb, f(0.6), f(-0.4), f(2.0), f(1.5)),
        (f(0.0), f(0.0), f(0.0), f(1.0), f(1.0)),
        (f(1e-3), f(-1e-3), f(1e-4), f(1e-2), f(1e3)),
    ]
    rec = np.concatenate([rec, np.asarray(edges, dtype=np.float32)])
    got = H.host_law(rec)
    want = H.scan_law(rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4])
    assert got.shape == want.shape == (n + len(edges),)
    assert np.array_equal(_bits(got), _bits(want)), np.nonzero(_bits(got) != _bits(want))[0]
    e = got[n:]
    assert e[0] == cl * 2 and e[1] == -cl * 2 and e[2] == cl * 2 and e[3] == -cl * 2
    assert e[4] == -cl * 3 and e[5] == f(-0.125), 'a ray that hits nothing saturates at -clip'
    assert _bits(e[6]) == 0 and _bits(e[7]) == 0x80000000 and _bits(e[8]) == 0x80000000
    assert e[9] == f(0.5) and e[10] == (f(0.3125) - f(-0.4) - f(0.6)) * f(1.5)
    sat = np.abs(got[:n]) == np.abs(rec[:n, 3] * rec[:n, 4])
    assert 0.2 * n < sat.sum() < 0.8 * n, 'the random records hold saturated and unsaturated ones'


def _layers(in_dim, hidden=8):
    z = lambda *s: np.zeros(s, np.float32)
    return [z(in_dim, hidden), z(hidden, 12)], [z(hidden), z(12)]


def _cell(in_dim, H_=8):
    z = lambda *s: np.zeros(s, np.float32)
    return (z(in_dim, 3 * H_), z(H_, 3 * H_), z(3 * H_), z(3 * H_), [z(H_, 12)], [z(12)])


@pytest.mark.parametrize('kind', ['mlp', 'gru'])
def test_in_obs_for_every_combination_of_scan_and_last_action(kind):
    from gym_quadruped_amd.policy import GruPolicy, HeightScan, MlpPolicy
    make = (lambda k, **kw: MlpPolicy(*_layers(k), **kw)) if kind == 'mlp' else (lambda k, **kw: GruPolicy(*_cell(k), **kw))
    spec = HeightScan(3, 5, offset=0.3, clip=0.5, scale=2.0)
    assert (spec.rows, spec.cols, spec.cells, spec.offset, spec.clip, spec.scale) == (3, 5, 15, 0.3, 0.5, 2.0)
    for scan, feed, in_obs in ((None, False, 40), (None, True, 28), (spec, False, 25), (spec, True, 13)):
        p = make(40, feed_last_action=feed, height_scan=scan)
        assert (p.in_dim, p.in_obs, p.height_scan) == (40, in_obs, scan)
    assert make(27, feed_last_action=True, height_scan=spec).in_obs == 0, 'a policy may read the scan and its last action alone'
    with pytest.raises(ValueError, match='15 cells'):
        make(26, feed_last_action=True, height_scan=spec)
    with pytest.raises(ValueError, match='15 cells'):
        make(14, height_scan=spec)
    with pytest.raises(ValueError, match='feed_last_action needs'):
        make(11, feed_last_action=True)
    with pytest.raises(ValueError, match='HeightScan'):
        make(40, height_scan=(3, 5))
    # the existing limit: 256 input columns are accepted, 257 refused - with the scan inside them
    wide = HeightScan(11, 17)
    p = make(256, feed_last_action=True, height_scan=wide)
    assert (p.in_dim, p.in_obs) == (256, 256 - 187 - 12)
    with pytest.raises(ValueError, match='256'):
        make(257, feed_last_action=True, height_scan=wide)
    # shift / scale tables cover the first in_obs columns alone
    p = make(40, feed_last_action=True, height_scan=spec, obs_shift=0.5, obs_scale=np.arange(13))
    assert p.obs_shift.shape == (13,) and p.obs_scale.shape == (13,)
    for bad in (dict(rows=0, cols=3), dict(rows=3, cols=-1), dict(rows=2.5, cols=3), dict(rows=3, cols=3, clip=0.0), dict(rows=3, cols=3, clip=-1.0),
                dict(rows=3, cols=3, clip=float('inf')), dict(rows=3, cols=3, offset=float('nan')), dict(rows=3, cols=3, scale=float('inf'))):
        with pytest.raises(ValueError):
            HeightScan(**bad)
    assert HeightScan(3, 3, scale=0.0).scale == 0.0 and HeightScan(3, 3, offset=-0.2).offset == -0.2


def test_reference_leaves_scan_columns_unscaled():
    from gym_quadruped_amd.policy import HeightScan
    spec = HeightScan(2, 3)
    for p in (H.make_mlp(7, spec), H.make_gru(7, spec)):
        assert (p.in_dim, p.in_obs) == (7 + 6 + 12, 7) and p.obs_shift.shape == (7,)
    p, q = H.make_mlp(7, spec), H.make_mlp(7, spec)
    rng = np.random.default_rng(2)
    rows = rng.uniform(-2, 2, (9, p.in_dim)).astype(np.float32)
    # the same network without tables, fed the rows with the tables applied to the first in_obs columns only, gives reference()
    q.obs_shift = q.obs_scale = None
    pre = rows.astype(np.float64)
    pre[:, :7] = (pre[:, :7] - p.obs_shift.astype(np.float64)) * p.obs_scale.astype(np.float64)
    assert np.array_equal(p.reference(rows), q.reference(pre))
    moved = rows.copy()
    moved[:, 7:13] += 1.0
    assert np.abs(p.reference(moved) - p.reference(rows)).max() > 1e-3, 'the scan columns reach the network'
    g = H.make_gru(7, spec)
    h = rng.uniform(-1, 1, (9, g.hidden)).astype(np.float32)
    g2 = H.make_gru(7, spec)
    g2.obs_shift = g2.obs_scale = None
    pre = rows.astype(np.float64)
    pre[:, :7] = (pre[:, :7] - g.obs_shift.astype(np.float64)) * g.obs_scale.astype(np.float64)
    for got, want in zip(g.reference(rows, h), g2.reference(pre, h)):
        assert np.array_equal(got, want)


def test_from_torch_passes_the_scan_on():
    import torch.nn as nn
    from gym_quadruped_amd.policy import GruPolicy, HeightScan, MlpPolicy
    spec = HeightScan(4, 4, clip=0.3)
    p = MlpPolicy.from_torch(nn.Sequential(nn.Linear(50, 16), nn.ELU(), nn.Linear(16, 12)), feed_last_action=True, height_scan=spec)
    assert (p.in_dim, p.in_obs, p.height_scan) == (50, 22, spec)
    g = GruPolicy.from_torch(nn.GRUCell(50, 8), nn.Sequential(nn.Linear(8, 12)), height_scan=spec)
    assert (g.in_dim, g.in_obs, g.height_scan) == (50, 34, spec)


def test_policy_scan_struct_and_exports_are_in_the_abi_and_the_version_stays():
    from gym_quadruped_amd import _lib, cabi
    # (layout and export against the header: tests/test_host_and_abi.py discovers every struct and symbol)
    assert 'gq_rollout_policy_scan' in _lib.ABI and 'gq_height_scan_eval' in _lib.ABI
    assert 'gq_rollout_policy_scan' in _lib.EXPORTS and 'gq_height_scan_eval' in _lib.EXPORTS
    s = cabi.GqPolicyScan
    assert [f[0] for f in s._fields_] == ['struct_size', 'rows', 'cols', 'offset', 'clip', 'scale'] and ctypes.sizeof(s) == 24
    assert (s.rows.offset, s.cols.offset, s.offset.offset, s.clip.offset, s.scale.offset) == (4, 8, 12, 16, 20)
    assert len(_lib.ABI['gq_rollout_policy_scan'][1]) == len(_lib.ABI['gq_rollout_policy_gru'][1]) + 1
    assert _lib.LIB_PATH.exists(), 'build the HIP extension first (__graft_entry__.build())'
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert L.gq_version() == 660 and cabi.GQ_ABI_VERSION == 660
    assert L.gq_rollout_policy_scan and L.gq_height_scan_eval
    # a stale binding is refused before anything else is looked at (no device is touched: the handle is never reached)
    L.gq_last_error.restype = ctypes.c_char_p
    L.gq_height_scan_eval.argtypes = _lib.ABI['gq_height_scan_eval'][1]
    L.gq_rollout_policy_scan.argtypes = _lib.ABI['gq_rollout_policy_scan'][1]
    stale = s(struct_size=ctypes.sizeof(s) - 4, rows=3, cols=3, clip=1.0, scale=1.0)
    assert L.gq_height_scan_eval(None, ctypes.byref(stale), None, None, 0, None, None) == -1
    assert b'GqPolicyScan' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
    m = cabi.GqPolicyMlp(struct_size=ctypes.sizeof(cabi.GqPolicyMlp), n_layers=1)
    args = (0, 0, 5.0, cabi.GqState(), cabi.GqObsOut(), None, None, None, None, None, None, None, None)
    assert L.gq_rollout_policy_scan(None, 4, ctypes.byref(m), None, ctypes.byref(stale), *args) == -1
    assert b'GqPolicyScan' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
    fresh = s(struct_size=ctypes.sizeof(s), rows=3, cols=3, clip=1.0, scale=1.0)
    assert L.gq_rollout_policy_scan(None, 4, ctypes.byref(m), None, ctypes.byref(fresh), *args) == -1
    assert b'stale binding' not in L.gq_last_error() and b'bad argument' in L.gq_last_error(), 'a null batch is refused next'
    assert L.gq_rollout_policy_scan(None, 4, ctypes.byref(m), None, None, *args) == -1 and b'bad argument' in L.gq_last_error()
