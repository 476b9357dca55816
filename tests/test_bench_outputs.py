"""bench.py's plain run and `--dump-outputs` (CPU, the oracle backend through tests/dist_driver.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(*args):
  out = subprocess.run(
      [sys.executable, os.path.join(ROOT, 'tests', 'dist_driver.py'), '--gpus', '1', '--workload', 'tiny',
       '--device', 'cpu', *args],
      capture_output=True, text=True, timeout=900, cwd=ROOT,
      env={k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')},
  )
  assert out.returncode == 0, out.stderr[-3000:]
  lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, out.stdout[-2000:]
  return json.loads(lines[0])


def _arrays(d):
  return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
  recs, dumps = [], []
  for run in ('a', 'b'):
    d = str(tmp_path / run)
    recs.append(_bench('--steps', '3', '--warmup', '1', '--dump-outputs', d))
    dumps.append(_arrays(d))
  rec = recs[0]
  assert rec['steps'] == 3 and rec['warmup'] == 1
  for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
    assert k in rec, k
  expect = rec['config']['global_batch'] * rec['steps'] / (rec['ms_per_step'] * rec['steps'] / 1e3)
  assert abs(rec['value'] - expect) / expect < 1e-3
  for k in ('roofline', 'kernels', 'cpu_baseline', 'f32_exact', 'c4'):   # (--full only)
    assert k not in rec, k
  a, b = dumps
  assert a.keys() == b.keys()
  for k in ('scores_poses.npy', 'best_index.npy', 'map_t_query.t.npy', 'map.bev_matching.features.npy'):
    assert k in a, sorted(a)
  assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
  for k, v in a.items():
    assert v.dtype in (np.float32, np.float64), (k, v.dtype)
    np.testing.assert_array_equal(v, b[k], err_msg=k)
  manifest = json.load(open(os.path.join(str(tmp_path / 'a'), 'manifest.json')))
  assert sorted(f + '.npy' for f in manifest) == sorted(a)
  assert manifest['scores_poses']['shape'] == list(a['scores_poses.npy'].shape)


def test_dump_outputs_samples_large_arrays_within_the_budget(tmp_path, monkeypatch):
  import bench
  monkeypatch.setattr(bench, 'DUMP_ELEMS', 1000)
  monkeypatch.setattr(bench, 'DUMP_BYTES', 12000)
  g = torch.Generator().manual_seed(0)
  tree = {'big': torch.randn(50, 70, generator=g), 'small': torch.arange(10, dtype=torch.int64),
          'mask': torch.rand(40, 40, generator=g) > 0.5, 'half': torch.randn(8, generator=g).to(torch.bfloat16)}
  for run in ('a', 'b'):
    bench.dump_outputs(tree, str(tmp_path / run))
  a, b = _arrays(str(tmp_path / 'a')), _arrays(str(tmp_path / 'b'))
  assert sorted(a) == ['big.npy', 'half.npy', 'mask.npy', 'small.npy']
  assert sum(v.nbytes for v in a.values()) <= 12000
  for k in a:
    np.testing.assert_array_equal(a[k], b[k])
  assert a['small.npy'].dtype == np.float64 and (a['small.npy'] == np.arange(10)).all()
  assert a['half.npy'].dtype == np.float32 and a['half.npy'].shape == (8,)
  man = json.load(open(str(tmp_path / 'a' / 'manifest.json')))
  assert man['big']['shape'] == [50, 70] and 'sample' in man['big'] and 'sample' not in man['small']
  n = man['big']['sample']['elements']
  idx = torch.randint(0, 3500, (n,), generator=torch.Generator().manual_seed(man['big']['sample']['seed'])).sort().values
  np.testing.assert_array_equal(a['big.npy'], tree['big'].reshape(-1)[idx].numpy())
