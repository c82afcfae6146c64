"""bench.py --dump-outputs and the timed step count.

* CPU: dump_outputs writes the parameters, the TF-Adam slots and the scalars of an engine as float32 .npy files, by variable
  name; outputs larger than 64 MB are cut to a fixed, seeded sample of the large arrays, the small ones stay whole.
* GPU: `--steps K` times exactly K steps, and they continue the seeded training trajectory of the restored state: the same
  arguments give the same arrays bit for bit, and `--restore-steps 30 --steps 4` ends where `--restore-steps 31 --steps 3` does.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _HostEngine(object):
    """the attributes of cfl.engine.PairEngine that dump_outputs reads, on the host"""

    def __init__(self, D, L, K):
        import bench
        from cfl import hipabi as H
        self.shape = H.make_shape(D, L, K, 'pcd', False, True)
        self.params = bench.init_params(D, L, K)
        self.theta = H.pack_theta(self.shape, self.params, None, 1e-6, 'cpu')
        self.m = self.theta * 0.5
        self.v = self.theta.abs()

    def read_scalars(self):
        from cfl import hipabi as H
        return {k: 0.25 * i for i, k in enumerate(H.SCALAR_NAMES)}


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, '*.npy')))}


def test_dump_outputs_names_dtypes_values(tmp_path):
    import bench
    from cfl import hipabi as H
    eng = _HostEngine(256, 6, 3)
    bench.dump_outputs(str(tmp_path), eng)
    got = _load(str(tmp_path))
    names = ['outputs_W', 'outputs_b', 'proto_W', 'proto_b', 'threshold']
    assert set(got) == {'%s_%s' % (t, n) for t in ('param', 'adam_m', 'adam_v') for n in names} | {'scalars'}
    assert all(a.dtype == np.float32 for a in got.values())
    for n in ('outputs/W', 'outputs/b', 'proto/W', 'proto/b'):
        key = n.replace('/', '_')
        assert np.array_equal(got['param_' + key], eng.params[n])
        assert np.array_equal(got['adam_m_' + key], eng.params[n] * np.float32(0.5))
    assert got['param_threshold'].tolist() == [np.float32(1e-6)]
    assert got['scalars'].tolist() == [0.25 * i for i in range(len(H.SCALAR_NAMES))]


def test_dump_outputs_stays_within_64_mb(tmp_path):
    import bench
    eng = _HostEngine(4096, 400, 4)                 # 3 x 4096 x 2000 floats = 98 MB before sampling
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), eng)
    sizes = [os.path.getsize(f) for f in glob.glob(str(tmp_path / 'a' / '*.npy'))]
    assert sum(sizes) <= 64 * 10 ** 6
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)        # a fixed sample
    assert a['scalars'].shape == (14,) and a['param_proto_b'].shape == (1600,)     # small arrays whole
    n = a['param_proto_W'].size
    assert 0 < n < 4096 * 1600
    # the same entries of every array of that size: the slots sit beside the parameters they belong to
    assert np.array_equal(a['adam_m_proto_W'], a['param_proto_W'] * np.float32(0.5))
    assert set(a['param_proto_W'].tolist()) <= set(eng.params['proto/W'].ravel().tolist())


def _bench(out_dir, restore_steps, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
           '--restore-steps', str(restore_steps), '--pool-mib', '64', '--no-cpu-baseline', '--no-kernel-profile', '--no-cli-loop',
           '--no-other-configs', '--no-dp-form', '--no-live-traffic', '--dump-outputs', out_dir]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), _load(out_dir)


@pytest.mark.gpu
def test_bench_times_k_steps_and_dumps_reproducible_outputs(tmp_path):
    line, a = _bench(str(tmp_path / 'a'), 30, 4)
    assert line['steps'] == 4 and line['repeats'] == 1 and line['timed_steps'] == 4 and line['value'] > 0
    assert len(a) == 16 and all(np.isfinite(x).all() for x in a.values())
    assert abs(float(a['scalars'][0]) - line['config']['final_loss']) <= 1e-6 * max(1.0, abs(line['config']['final_loss']))
    _, b = _bench(str(tmp_path / 'b'), 30, 4)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # 30 restored + 4 timed steps == 31 restored + 3 timed steps: the timed steps are the next steps of the same trajectory
    _, c = _bench(str(tmp_path / 'c'), 31, 3)
    assert set(a) == set(c) and all(np.array_equal(a[k], c[k]) for k in a), \
        [k for k in a if not np.array_equal(a[k], c[k])]
