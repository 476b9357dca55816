"""The float64 restatement ``vote_recall_reference`` against analytic answers, and the host side of
``recall_from_votes`` (``recall_thresholds``, ``recall_table``) against hand-computed ones.  No GPU."""
import math

import numpy as np
import pytest
import torch

import vote_recall_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids


@pytest.mark.parametrize('rho2,count', sorted(ref.LATTICE_COUNTS.items()))
def test_lattice_point_counts(rho2, count):
  assert len(ref.disc_offsets(rho2)) == count


@pytest.mark.parametrize('rho2', sorted(ref.LATTICE_COUNTS))
@pytest.mark.parametrize('half_r', (0, 1, 2))
def test_uniform_volume_interior_ball(rho2, half_r):
  """A uniform unmasked volume: an interior ball holds N(rho2) (2 half_r + 1) of the R Ho Wo cells; a corner ball the
  quarter disc that is inside."""
  shape = (7, 13, 15)
  v = np.full(shape, -3.25, dtype=np.float32)
  out = ref.vote_recall(v, (rho2,), (half_r,), [(0, 6, 7), (6, 0, 0)], scale=0.7)
  n = ref.LATTICE_COUNTS[rho2] * (2 * half_r + 1)
  want = math.log(n / np.prod(shape))
  rho = math.isqrt(rho2)
  inner = out['maps'][0][:, rho:shape[1] - rho, rho:shape[2] - rho]
  assert np.abs(inner - want).max() <= 1e-14
  assert abs(out['centre'][0, 0] - want) <= 1e-14             # rotation 0: the window wraps to 6
  quarter = sum(1 for da, db in ref.disc_offsets(rho2) if da >= 0 and db >= 0) * (2 * half_r + 1)
  assert abs(out['centre'][1, 0] - math.log(quarter / np.prod(shape))) <= 1e-14
  assert abs(out['log_z'] - (float(np.float32(0.7)) * -3.25 + math.log(np.prod(shape)))) <= 1e-12
  assert out['count'].tolist() == [int(np.prod(shape)), 0, 0, 0]


@pytest.mark.parametrize('cell', [(0, 0, 0), (0, 8, 10), (5, 12, 0), (3, 6, 7)])
@pytest.mark.parametrize('rho2,half_r', [(0, 0), (2, 1), (25, 2), (1024, 0)])
def test_one_finite_cell_gives_the_mirrored_ball(cell, rho2, half_r):
  """One finite cell: a cell's ball holds it exactly when the cell lies in the ball around it (the ball is symmetric),
  clipped at the corner in a and b and wrapped at rotation 0; the map is 0 there and -inf elsewhere."""
  shape = (6, 13, 11)
  v = np.full(shape, -np.inf, dtype=np.float32)
  v[cell] = 1.5
  out = ref.vote_recall(v, (rho2,), (half_r,), [cell], gt_index=tuple(float(x) for x in cell))
  mask = ref.ball_mask(shape, cell, rho2, half_r)
  assert (out['maps'][0][mask] == 0).all() and np.isneginf(out['maps'][0][~mask]).all()
  rho = math.isqrt(rho2)
  inside = sum(1 for da, db in ref.disc_offsets(rho2) if 0 <= cell[1] + da < shape[1] and 0 <= cell[2] + db < shape[2])
  assert mask.sum() == inside * (2 * half_r + 1) and rho <= 32
  if half_r and cell[0] == 0:
    assert mask[shape[0] - 1].any()                           # the circular wrap
  assert out['centre'][0, 0] == 0 and out['gt'][0] == 0 and out['count'].tolist() == [1, 0, 1, 0]
  index, value = ref.best_of(ref.round_log_mass(out['maps']))
  assert value[0] == 0 and mask[tuple(index[0])] and index[0].tolist() == list(np.argwhere(mask)[0])


def test_patterns_of_the_special_cases():
  shared = ref.shared()
  c, out = shared['all_masked']
  assert np.isneginf(out['maps']).all() and np.isneginf(out['centre']).all() and np.isneginf(out['gt']).all()
  assert out['count'].tolist() == [0, 0, 1, 0] and out['log_z'] == -np.inf
  index, value = ref.best_of(ref.round_log_mass(out['maps']))
  assert (index == -1).all() and np.isneginf(value).all()
  c, out = shared['nan_inf']
  assert out['count'].tolist() == [8 * 31 * 33 - 8, 3, 1, 0]
  assert np.isneginf(out['centre'][0, 0]) and np.isfinite(out['centre'][0, 1])   # a NaN cell alone; with neighbours
  c, out = shared['empty_rows_gt_out_of_range']
  live = np.isfinite(out['centre'][:, 0])
  assert live.tolist() == [False, True, False, False, False, False, False, False, True]
  assert np.isnan(out['gt']).all() and out['count'][2] == 0
  assert np.isnan(shared['gt_not_finite'][1]['gt']).all()
  assert shared['gt_wraps'][1]['gt_cell'] == (7, 0, 32)
  assert shared['odd_L8'][1]['gt_cell'] == (0, 30, 0)         # 7.5 -> 8 -> 0, 0.5 -> 0: half to even
  c, out = shared['ball_covers_volume']
  assert np.abs(out['maps']).max() <= 1e-14
  for name, (c, out) in shared.items():
    assert (out['maps'] <= 0).all() and not np.isnan(out['maps']).any(), name
    # a larger ball holds more: levels ordered by both thresholds are ordered by mass
    for i in range(len(c['rho2'])):
      for j in range(len(c['rho2'])):
        if c['rho2'][i] <= c['rho2'][j] and c['half_r'][i] <= c['half_r'][j]:
          assert (out['maps'][i] <= out['maps'][j] + 1e-12).all(), (name, i, j)


def test_planted_clusters_are_decided_on_the_reference():
  """The planted cases are clear: the reference's best cell beats every cell outside its own ball by far more than the
  8 f32 ulps (+ the float64 slack) the GPU test allows for, and the planted pose lies in that ball."""
  for name, (c, out) in ref.shared().items():
    if c['planted'] is None:
      continue
    m32 = ref.round_log_mass(out['maps'])
    index, value = ref.best_of(m32)
    for l in range(len(c['rho2'])):
      ball = ref.ball_mask(c['votes'].shape, index[l], c['rho2'][l], c['half_r'][l])
      assert ball[c['planted']], (name, l)
      margin = float(value[l]) - float(m32[l][~ball].max())
      assert margin > 1e-3, (name, l, margin)


def test_recall_thresholds_by_hand():
  grid = grids.Grid2D((32, 32), 0.25)
  rho2, half_r = pev.recall_thresholds(pev.RECALL_THRESHOLDS, grid, 36)
  # 0.5 m = 2 cells, 1 m = 4, 2 m = 8: whole numbers of cells, excluded by the strict <; 36 rotations = 10 degrees a bin
  assert rho2.tolist() == [3, 15, 63] and half_r.tolist() == [0, 0, 0] and rho2.dtype == np.int32
  rho2, half_r = pev.recall_thresholds(((0.6, 10), (0.6, 10.5), (5, 25), (0.1, 0.5)), grid, 36)
  # (0.6 / 0.25)^2 = 5.76 -> 5; 10 degrees = exactly one bin -> 0, 10.5 -> 1; 20^2 -> 399, 2.5 bins -> 2; 0.16 -> 0
  assert rho2.tolist() == [5, 5, 399, 0] and half_r.tolist() == [0, 1, 2, 0]
  # 0.2 is not a binary fraction: 1 / 0.2 must still be exactly 5 cells
  rho2, half_r = pev.recall_thresholds(((1, 2), (0.6, 3)), grids.Grid2D((16, 16), 0.2), 256)
  assert rho2.tolist() == [24, 8] and half_r.tolist() == [1, 2]           # 2 * 256 / 360 = 1.42, 3 -> 2.13
  for bad in (((9, 1),), ((1, 60),), ((0, 1),), ((1, 0),), ((1, float('nan')),), (), ((1, 1),) * 9, ((1, 2, 3),)):
    with pytest.raises(ValueError):
      pev.recall_thresholds(bad, grid, 36)
  with pytest.raises(ValueError):
    pev.recall_thresholds(((1, 200),), grid, 2)               # 1.11 bins -> half_r = 1: 2 half_r + 1 > R = 2
  assert pev.recall_thresholds(((1, 200),), grid, 3)[1].tolist() == [1]


def test_recall_table_by_hand():
  pred = [0.05, 0.15, 0.12, 0.95, 1.0, 0.5, float('nan'), 0.55]
  hit = [0, 1, 0, 1, 1, 0, 1, 1]
  t = pev.recall_table(pred, hit, bins=10)
  assert t['count'].tolist() == [1, 2, 0, 0, 0, 2, 0, 0, 0, 2] and t['total'] == 7
  assert t['mean_pred'][[0, 1, 5, 9]].tolist() == pytest.approx([0.05, 0.135, 0.525, 0.975])
  assert t['hit_rate'][[0, 1, 5, 9]].tolist() == [0.0, 0.5, 0.5, 1.0]
  assert np.isnan(t['mean_pred'][2]) and np.isnan(t['hit_rate'][2])
  assert t['ece'] == pytest.approx((1 * 0.05 + 2 * 0.365 + 2 * 0.025 + 2 * 0.025) / 7)
  assert t['edges'].tolist() == pytest.approx(np.linspace(0, 1, 11).tolist())
  valid = [True] * 7 + [False]
  t2 = pev.recall_table(torch.tensor(pred), torch.tensor(hit, dtype=torch.bool), bins=2, valid=valid)
  assert t2['count'].tolist() == [3, 3] and t2['hit_rate'].tolist() == pytest.approx([1 / 3, 2 / 3])
  empty = pev.recall_table([], [])
  assert empty['total'] == 0 and math.isnan(empty['ece'])
  with pytest.raises(ValueError):
    pev.recall_table([0.5], [1, 0])
  # a calibrated predictor: hits drawn with the predicted probability
  rng = np.random.default_rng(0)
  p = rng.uniform(0, 1, 20000)
  t = pev.recall_table(p, rng.uniform(0, 1, p.size) < p, bins=10)
  assert t['ece'] < 0.02 and np.abs(t['hit_rate'] - t['mean_pred']).max() < 0.05
