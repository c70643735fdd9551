"""The MLP policy without a GPU (gym_quadruped_amd/policy.py, csrc/gq_policy_mlp.h, include/gq.h GqPolicyMlp): the packed blob, the
law's definition (mlp_row_forward in tests/policy_mlp_host.cpp, a stand-alone g++ program) against a float64 evaluation layer by layer,
the header's activations and noise, the torch import, and the new struct and entry points of the ABI."""
import ctypes

import numpy as np
import pytest

import policy_mlp_ref as R

CASES = [(shape, act, out) for shape in ('odd', 'wide', 'single') for act, out in (('relu', None), ('elu', 'tanh'), ('tanh', None))]


@pytest.mark.parametrize('shape,act,out', CASES)
def test_pack_follows_the_layout_formula_and_pads_with_zeros(shape, act, out):
    p = R.make_policy(shape, act, out)
    blob = p.pack()
    assert blob.dtype == np.float32 and blob.size == p.blob_floats()
    rng = np.random.default_rng(3)
    at, used = 0, np.zeros(blob.size, dtype=bool)
    for w, b in zip(p.weights, p.biases):
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


@pytest.mark.parametrize('shape,act,out', CASES)
def test_row_forward_is_within_the_fma_chain_bound_of_every_layer(shape, act, out):
    p = R.make_policy(shape, act, out)
    rows = R.rows_for(p, 24)
    layers = R.host_forward(p, rows)
    for l, (y64, bound) in enumerate(R.layer_bounds(p, layers, rows)):
        err = np.abs(layers[l].astype(np.float64) - y64)
        print(f'{shape} {act} layer {l}: worst error / bound {float((err / bound).max()):.3f}')
        assert (err <= bound).all(), (l, float((err / bound).max()))
    ref, nb = R.network_bound(p, rows)
    assert np.array_equal(ref, p.reference(rows))
    assert (np.abs(layers[-1] - ref) <= nb).all()


@pytest.mark.parametrize('name', ['elu', 'tanh'])
def test_activation_error_is_measured_and_small(name):
    """the ratio the bounds above are built on (profiles/mlp_policy_law_error.txt holds one measurement); a polynomial that lost a term
    would show here as a ratio in the hundreds"""
    r = R.activation_error(name)
    print(f'{name}: {r:.4f} x 2^-24 max(1, |y|)')
    assert r < 4.0
    x = np.asarray([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0, np.inf, -np.inf], dtype=np.float32)
    from gym_quadruped_amd.policy import _ACT64
    assert np.allclose(R.host_activation(name, x), _ACT64[name](x.astype(np.float64)), rtol=1e-6, atol=0)


def test_noise_restatement_has_the_header_s_bits():
    rng = np.random.default_rng(0)
    x0 = rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
    x1 = rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
    x0[:4], x1[:4] = [0, 0xffffffff, 0x100, 0x80000000], [0, 0xffffffff, 0x40000000, 0xc0000000]
    got, want = R.host_normal(x0, x1), R.normal_ref(x0, x1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    u1, u2 = ((x0 >> 8).astype(np.float64) + 0.5) / 2 ** 24, (x1 >> 8).astype(np.float64) / 2 ** 24
    z = np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    assert np.abs(got - z).max() <= 6 * 2.0 ** -24   # |z| < 6: the float32 rounding of the result and nothing else


def test_from_torch_round_trips_and_refuses_what_it_does_not_know():
    import torch
    import torch.nn as nn
    from gym_quadruped_amd.policy import MlpPolicy
    torch.manual_seed(0)
    for act, mod in (('relu', nn.ReLU), ('elu', nn.ELU), ('tanh', nn.Tanh)):
        for tail in ([], [nn.Tanh()]):
            net = nn.Sequential(nn.Linear(49, 20), mod(), nn.Linear(20, 33), mod(), nn.Linear(33, 12), *tail)
            p = MlpPolicy.from_torch(net, feed_last_action=True)
            assert (p.activation, p.out_activation, p.in_obs, p.widths) == (act, 'tanh' if tail else 'none', 37, [20, 33, 12])
            x = np.random.default_rng(1).uniform(-2, 2, (9, 49)).astype(np.float32)
            want = net.double()(torch.from_numpy(x).double()).detach().numpy()
            assert np.abs(p.reference(x) - want).max() < 1e-12
    assert MlpPolicy.from_torch(nn.Sequential(nn.Linear(24, 12))).widths == [12]
    for bad in (nn.Sequential(nn.Linear(24, 16), nn.Sigmoid(), nn.Linear(16, 12)), nn.Sequential(nn.Linear(24, 16), nn.Linear(16, 12)),
                nn.Sequential(nn.Linear(24, 16), nn.ReLU(), nn.Linear(16, 16), nn.Tanh(), nn.Linear(16, 12)), nn.Sequential(nn.Linear(24, 16), nn.ELU(alpha=0.5), nn.Linear(16, 12)),
                nn.Sequential(nn.Linear(24, 16), nn.ReLU(), nn.LayerNorm(16), nn.Linear(16, 12)), nn.Sequential(nn.Linear(24, 12), nn.ReLU()), nn.Linear(24, 12),
                nn.Sequential(nn.Linear(24, 16), nn.ReLU(), nn.Linear(16, 11)), nn.Sequential(nn.Linear(24, 300), nn.ReLU(), nn.Linear(300, 12)),
                nn.Sequential(*[m for _ in range(4) for m in (nn.Linear(24, 24), nn.ReLU())], nn.Linear(24, 12))):
        with pytest.raises(ValueError):
            MlpPolicy.from_torch(bad)


def test_policy_mlp_struct_layout_matches_header_and_the_abi_keeps_its_version():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.cabi import GqPolicyMlp
    # (layout and export: tests/test_host_and_abi.py, for every struct and symbol)
    assert 'gq_rollout_policy' in _lib.EXPORTS and 'gq_policy_mlp_eval' in _lib.EXPORTS
    assert _lib.LIB_PATH.exists(), 'build the HIP extension first (__graft_entry__.build())'
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert L.gq_version() == 660
    assert L.gq_rollout_policy and L.gq_policy_mlp_eval
    # a stale binding is refused before anything else is looked at (no device is touched: the handle is never reached)
    L.gq_last_error.restype = ctypes.c_char_p
    m = GqPolicyMlp(struct_size=ctypes.sizeof(GqPolicyMlp) - 8, n_layers=1)
    L.gq_policy_mlp_eval.argtypes = _lib.ABI['gq_policy_mlp_eval'][1]
    assert L.gq_policy_mlp_eval(None, ctypes.byref(m), None, 0, 0, None, None) == -1 and b'stale binding' in L.gq_last_error()
