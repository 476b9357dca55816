"""CPU: the numpy restatement ``vote_rebase_reference`` pinned from outside (scipy's linear interpolation), and
``pose_exhaustive_voting.rebase_table`` pinned against the index <-> transform pair it inverts.  No GPU."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import vote_rebase_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids


def _cases():
  return {c['name']: c for c in ref.all_inputs()}


def _tfm(phi, tau):
  return geometry.Transform2D(torch.tensor(float(phi), dtype=torch.float64), torch.tensor(tau, dtype=torch.float64))


def _turn_about_index(phi, about, grid, shift=(0.0, 0.0)):
  """The change of map frame that turns the lattice by ``phi`` about the index point ``about`` and then moves it by
  ``shift`` cells: index ``about`` is the centre-frame position (about - (extent - 1.5)) cell_size."""
  c, s = (0.0 if abs(v) < 2.0 ** -40 else v for v in (math.cos(phi), math.sin(phi)))
  rot = np.array([[c, -s], [s, c]])
  centre = np.asarray(grid.extent_meters) / 2
  pivot = (np.asarray(about, np.float64) - (np.asarray(grid.extent) - 1.5)) * grid.cell_size   # centre frame
  sigma = pivot - rot @ pivot + np.asarray(shift, np.float64) * grid.cell_size
  tau = sigma - (rot @ centre - centre)
  return _tfm(phi, tau.tolist())


@pytest.mark.parametrize('name', ['ragged', 'quarter'])
def test_gather_is_scipy_linear_interpolation(name):
  """``map_coordinates(order=1, mode='constant', cval=0)`` of the mass array, the rotation axis padded circularly by
  hand.  That mode does not interpolate between an edge cell and the outside, which the operator does (a tap outside
  contributes 0), so the planes also get one ring of zeros, by hand as well."""
  c = _cases()[name]
  p = ref.masses(c['src'], c['scale'])[0]
  R, Ho, Wo = p.shape
  k, sa, sb = ref.coordinates(p.shape, c['table'])
  padded = np.pad(np.concatenate([p, p, p[:1]], 0), ((0, 0), (1, 1), (1, 1)))   # planes -R .. R, a zero ring
  coords = np.stack([np.broadcast_to((k + R)[:, None, None], p.shape), np.broadcast_to(sa[None] + 1, p.shape),
                     np.broadcast_to(sb[None] + 1, p.shape)])
  want = ndimage.map_coordinates(padded, coords, order=1, mode='constant', cval=0.0)
  got, any_tap = ref.gather(p, c['table'])
  assert np.isfinite(got).all() and (got > 0).any() and (got == 0).any()
  assert np.abs(got - want).max() <= 1e-12 * p.max()
  assert not got[~any_tap].any()


@pytest.mark.parametrize('R', [4, 8, 36])
def test_rebase_table_inverts_the_index_of_the_composed_pose(R):
  rng = np.random.default_rng(R)
  worst = 0.0
  for extent, cell in (((12, 10), 0.5), ((7, 16), 0.2)):
    grid = grids.Grid2D(extent, cell)
    for _ in range(4):
      new_t_old = _tfm(rng.uniform(-math.pi, math.pi), rng.uniform(-2, 2, 2).tolist())
      dk, A, o = pev.rebase_table(new_t_old, grid, R)
      assert 0.0 <= dk < R and A.dtype == np.float64 and o.dtype == np.float64
      for _ in range(8):
        idx = np.array([rng.integers(0, R), rng.uniform(0, 2 * extent[0] - 2), rng.uniform(0, 2 * extent[1] - 2)])
        pose = pev.exhaustive_index_to_tfm(torch.tensor(idx, dtype=torch.float64), grid, R)
        pose = geometry.Transform2D(pose.angle.to(torch.float64), pose.t.to(torch.float64))
        want = pev.exhaustive_tfm_to_index(new_t_old @ pose, grid, R).numpy()
        got = np.concatenate([[(idx[0] + dk) % R], A.T @ (idx[1:] - o)])       # the table gathers: its inverse
        dk_err = abs((got[0] - want[0] + R / 2) % R - R / 2)
        worst = max(worst, dk_err, np.abs(got[1:] - want[1:]).max())
  print(f'R = {R}: largest difference {worst:.2e} index units')
  assert worst < 1e-5                      # (exhaustive_index_to_tfm rounds the pose to f32)


def test_identity_table():
  dk, A, o = pev.rebase_table(_tfm(0.0, [0.0, 0.0]), grids.Grid2D((12, 10), 0.5), 8)
  assert dk == 0.0 and (A == np.eye(2)).all() and (o == 0).all()
  assert not np.signbit(dk) and not np.signbit(A).any() and not np.signbit(o).any()
  c = _cases()['identity']
  out, stats, count = ref.vote_rebase(c['src'], (dk, A, o), c['scale'])
  assert stats[1] == 1.0 and count[3] == 0 and (np.isfinite(out) == np.isfinite(c['src'])).all()


def test_quarter_turn_is_rot90_and_a_roll():
  """The lattice's middle, index (Ho - 1) / 2, lies half a cell from the map centre, index extent - 1.5 (the +0.5 cell
  offset of ``exhaustive_index_to_tfm``): the quarter turn that permutes the lattice is the one about its middle."""
  R, H = 8, 8
  grid = grids.Grid2D((H, H), 0.25)
  table = pev.rebase_table(_turn_about_index(math.pi / 2, (H - 1, H - 1), grid), grid, R)
  want_table = ref.index_table(math.pi / 2, (0, 0), 6.0, (R, 2 * H - 1, 2 * H - 1))
  assert table[0] == want_table[0] and (table[1] == want_table[1]).all() and (table[2] == want_table[2]).all()
  c = _cases()['quarter_lattice']
  src, scale = c['src'], c['scale']
  p = ref.masses(src, scale)[0]
  mass, any_tap = ref.gather(p, table)
  assert any_tap.all()
  assert (mass == np.roll(np.rot90(p, k=1, axes=(1, 2)), 6, axis=0)).all()        # r' = r + dk: exact, cell for cell
  out, stats, count = ref.vote_rebase(src, table, scale)
  lz = stats[0]
  with np.errstate(invalid='ignore'):
    norm = np.roll(np.rot90(float(np.float32(scale)) * src.astype(np.float64) - lz, k=1, axes=(1, 2)), 6, axis=0)
  assert ((out == -np.inf) == (norm == -np.inf)).all() and stats[1] == 1.0
  fin = np.isfinite(out)
  assert (np.abs(out[fin] - norm[fin]) <= ref.bound(src, table, scale)[fin]).all()
  # the same turn about the map centre moves whole cells too, but one row leaves the lattice and one is not covered
  about_centre = pev.rebase_table(_tfm(math.pi / 2, [2 * H * 0.25 / 2, 0.0]), grid, R)
  case = _cases()['quarter']['table']
  assert about_centre[0] == case[0] and (about_centre[1] == case[1]).all() and (about_centre[2] == case[2]).all()
  assert ref.vote_rebase(src, about_centre, scale)[2][3] == R * (2 * H - 1)


def test_there_and_back_returns_a_delta_to_its_cell():
  R, extent = 36, (16, 17)
  grid = grids.Grid2D(extent, 0.25)
  shape = (R, 2 * extent[0] - 1, 2 * extent[1] - 1)
  new_t_old = _tfm(0.37, [0.61, -0.43])
  for cell in ((5, 12, 20), (30, 17, 9), (0, 15, 16)):
    src = np.full(shape, -np.inf, np.float32)
    src[cell] = 0.0
    there = ref.vote_rebase(src, pev.rebase_table(new_t_old, grid, R))[0].astype(np.float32)
    assert 1 <= np.isfinite(there).sum() <= 2 * 9          # (the cells whose source position lies within one cell of it)
    back = ref.vote_rebase(there, pev.rebase_table(new_t_old.inv, grid, R))[0]
    assert np.unravel_index(np.argmax(np.where(np.isfinite(back), back, -np.inf)), shape) == cell


def test_whole_cell_translation_is_an_exact_shift():
  c = _cases()['shift']
  src, scale = c['src'], c['scale']
  R, Ho, Wo = src.shape
  grid = grids.Grid2D(((Ho + 1) // 2, (Wo + 1) // 2), 0.25)
  table = pev.rebase_table(_tfm(0.0, [2 * 0.25, -3 * 0.25]), grid, R)
  assert table[0] == c['table'][0] and (table[1] == c['table'][1]).all() and (table[2] == c['table'][2]).all()
  p = ref.masses(src, scale)[0]
  mass, any_tap = ref.gather(p, table)
  want = np.zeros_like(p)
  want[:, 2:, :Wo - 3] = p[:, :Ho - 2, 3:]                 # destination (a + 2, b - 3) holds source (a, b)
  covered = np.zeros(p.shape, bool)
  covered[:, 2:, :Wo - 3] = True
  assert (mass == want).all() and (any_tap == covered).all()
  out = ref.vote_rebase(src, table, scale)[0]
  assert (out[~covered] == -np.inf).all() and np.isfinite(out[covered]).any()
