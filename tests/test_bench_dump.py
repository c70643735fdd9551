"""bench.py --dump-outputs on the host: file names, dtypes, values, the seeded row sample past the size cap, and the
one-row-per-env condition the sample relies on (fake env tensors; the GPU run is tests/test_gpu_boundary.py)."""
import types

import numpy as np
import pytest
import torch

import bench


def _fake(n):
    g = torch.Generator().manual_seed(0)
    env = types.SimpleNamespace(num_envs=n, qpos=torch.randn(n, 19, generator=g, dtype=torch.float64), qvel=torch.randn(n, 18, generator=g))
    obs = {'qpos': torch.randn(n, 19, generator=g), 'feet_pos:base': torch.randn(n, 12, generator=g)}
    info = {'time': torch.rand(n, generator=g), 'step_num': torch.arange(n, dtype=torch.int32), 'episode': torch.arange(n, dtype=torch.int64),
            'invalid_contacts': torch.arange(n) % 3 == 0, 'note': 'not a tensor'}
    last = (obs, torch.randn(n, generator=g), torch.arange(n) % 2 == 0, torch.zeros(n, dtype=torch.bool), info)
    return env, last


def test_dump_writes_every_output_as_float32_or_float64(tmp_path):
    env, last = _fake(8)
    bench.dump_outputs(tmp_path, env, last, None)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted(['obs_qpos.npy', 'obs_feet_pos@base.npy', 'reward.npy', 'terminated.npy', 'truncated.npy', 'qpos.npy', 'qvel.npy',
                            'info_time.npy', 'info_step_num.npy', 'info_episode.npy', 'info_invalid_contacts.npy'])
    want = {'obs_qpos': (last[0]['qpos'], np.float32), 'obs_feet_pos@base': (last[0]['feet_pos:base'], np.float32), 'reward': (last[1], np.float32),
            'terminated': (last[2], np.float32), 'truncated': (last[3], np.float32), 'qpos': (env.qpos, np.float64), 'qvel': (env.qvel, np.float32),
            'info_time': (last[4]['time'], np.float32), 'info_step_num': (last[4]['step_num'], np.float32),
            'info_episode': (last[4]['episode'], np.float64), 'info_invalid_contacts': (last[4]['invalid_contacts'], np.float32)}
    for k, (t, dt) in want.items():
        a = np.load(tmp_path / f'{k}.npy')
        assert a.dtype == dt, k
        np.testing.assert_array_equal(a, t.numpy().astype(dt), err_msg=k)


def test_dump_past_the_cap_is_a_fixed_sample_of_env_rows(tmp_path, monkeypatch):
    n = 4096
    env, last = _fake(n)
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 100_000)
    for d in ('a', 'b'):
        bench.dump_outputs(tmp_path / d, env, last, None)
    assert sum(p.stat().st_size for p in (tmp_path / 'a').iterdir()) <= 100_000
    idx = np.load(tmp_path / 'a' / 'env_index.npy')
    assert idx.dtype == np.float64 and 0 < len(idx) < n and np.all(np.diff(idx) > 0) and idx[-1] < n
    keep = idx.astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'qpos.npy'), env.qpos.numpy()[keep])
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'obs_feet_pos@base.npy'), last[0]['feet_pos:base'].numpy()[keep])
    for p in (tmp_path / 'a').iterdir():
        np.testing.assert_array_equal(np.load(p), np.load(tmp_path / 'b' / p.name), err_msg=p.name)


def test_dump_refuses_an_array_that_is_not_one_row_per_env(tmp_path):
    env, last = _fake(8)
    last[4]['time'] = torch.zeros(3)
    with pytest.raises(ValueError, match='info_time'):
        bench.dump_outputs(tmp_path, env, last, None)
    assert not tmp_path.joinpath('qpos.npy').exists()
