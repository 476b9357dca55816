"""CPU: the float64 reference of ``vote_raster`` (tests/vote_raster_reference.py) and the host table
(``pose_exhaustive_voting.raster_prior``) pinned to things that are not themselves: scipy's bilinear sampler, the pose
of an index (``exhaustive_indices_to_tfm``), the symmetry of the second harmonic, ``vote_posterior_reference`` for a
constant raster, finite differences of log_z in the strength, and every documented ValueError."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import vote_posterior_reference as pref
import vote_raster_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids


def test_bilin_is_scipys_order_one_sampler():
  """With NaN standing for "outside": ``map_coordinates(order=1, mode='constant', cval=nan)`` on the NaN-marked plane."""
  rng = np.random.default_rng(1)
  X, Y, Ho, Wo = 9, 11, 14, 13
  plane = rng.standard_normal((X, Y))
  ok = rng.random((X, Y)) > 0.15
  marked = np.where(ok, plane, np.nan)
  for n, f in (((-2, -3), (0.0, 0.0)), ((-2, 1), (0.25, 0.0)), ((0, -3), (0.0, 0.625)), ((-1, -1), (0.375, 0.75))):
    tab = dict(planes=np.array([[f[0], f[1], 1, 0]], np.float32))
    w = ref.weights(tab)[0]
    got, _, taps = ref.bilin(np.where(ok, plane, 0.0), ok, n, w, Ho, Wo)
    assert taps == (1 + (f[0] != 0)) * (1 + (f[1] != 0))
    a, b = np.meshgrid(np.arange(Ho) + n[0] + f[0], np.arange(Wo) + n[1] + f[1], indexing='ij')
    # a whole coordinate touches no second tap; scipy multiplies it by 0 and spreads a NaN: sample per axis as needed
    want = ndimage.map_coordinates(marked, [a, b], order=1, mode='constant', cval=np.nan)
    if f[0] == 0 or f[1] == 0:
      lone = np.full((Ho, Wo), np.nan)
      for i in range(Ho):
        for j in range(Wo):
          x, y = i + n[0], j + n[1]
          taps_ij = [(x + di, y + dj, (f[0] if di else 1 - f[0]) * (f[1] if dj else 1 - f[1]))
                     for di in (0, 1) for dj in (0, 1)]
          taps_ij = [t for t in taps_ij if t[2] != 0]
          if all(0 <= tx < X and 0 <= ty < Y and ok[tx, ty] for tx, ty, _ in taps_ij):
            lone[i, j] = sum(wt * plane[tx, ty] for tx, ty, wt in taps_ij)
      # where scipy is finite it must agree; where only a zero-weight tap is missing the brute-force sum decides
      both = np.isfinite(want)
      assert np.allclose(got[both], want[both], rtol=0, atol=1e-12) and (np.isfinite(lone) | ~both).all()
      want = lone
    assert (np.isnan(got) == np.isnan(want)).all()
    fin = np.isfinite(want)
    assert fin.any() and (~fin).any()
    assert np.abs(got[fin] - want[fin]).max() < 1e-12


@pytest.mark.parametrize('extent', ((6, 8), (5, 7)), ids=('even', 'odd'))
@pytest.mark.parametrize('sensor', (None, (0.3, 1.1)), ids=('centred', 'off-centre'))
def test_the_offsets_are_the_pose_of_the_index(extent, sensor):
  """o_k against ``exhaustive_indices_to_tfm`` applied to ``sensor_q``, in float64, to 1e-9 cells, for every rotation."""
  R, cell, origin = 12, 0.25, (0.35, -0.2)
  grid = grids.Grid2D(extent, cell)
  shape = (R, 2 * extent[0] - 1, 2 * extent[1] - 1)
  A = np.zeros((4, 5))
  prior = pev.raster_prior(grid, R, log_area=A, origin=origin, sensor_q=sensor)
  tab = ref.table(shape, cell, A, origin=origin, sensor_q=sensor)
  assert prior.shape == shape and np.abs(prior.offset - tab['offset']).max() < 1e-12
  assert (prior.offsets == tab['offsets']).all() and (prior.planes == tab['planes']).all()
  assert np.abs(prior.offsets + prior.planes[:, :2].astype(np.float64) - prior.offset).max() < 2.0 ** -24
  assert ((prior.planes[:, :2] >= 0) & (prior.planes[:, :2] < 1)).all()
  if sensor is None and extent[0] % 2 == 0:                      # on the BEV grid itself (origin 0): one tap
    assert (pev.raster_prior(grid, R, log_area=A).planes[:, :2] == 0).all()
  s = np.asarray(grid.extent_meters, np.float64)[:2] / 2 if sensor is None else np.asarray(sensor, np.float64)
  rng = np.random.default_rng(2)
  for k in range(R):
    a, b = int(rng.integers(0, shape[1])), int(rng.integers(0, shape[2]))
    tfm = pev.exhaustive_indices_to_tfm(torch.tensor([[k, a, b]]), grid, R)
    angle = -2 * np.pi * k / R                                   # (the f32 angle of the transform, in float64)
    assert abs(float(tfm.angle[0]) - angle) < 1e-6
    # the float64 pose of the index: c @ (-alpha, xy_cell) @ c^-1 with xy_cell = ((a, b) - extent + 1.5) cell
    c = np.asarray(extent, np.float64) * cell / 2
    rot = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    t = c + (np.array([a, b]) - np.asarray(extent) + 1.5) * cell - rot @ c
    assert np.abs(t - tfm.t[0].double().numpy()).max() < 1e-5   # (the f32 transform agrees with the float64 one)
    p = rot @ s + t
    x = (p - np.asarray(origin)) / cell - 0.5
    assert np.abs(x - (np.array([a, b]) + prior.offset[k])).max() < 1e-9
    assert np.abs(p - ref.sensor_position(shape, cell, k, a, b, s)).max() < 1e-12


def test_log_prior_of_the_table_is_the_reference():
  shape = (8, 9, 11)
  grid = grids.Grid2D((5, 6), 0.25)
  A, ok, phi, kap = ref.random_raster(7, 6, 3)
  for h in (1, 2):
    kw = dict(log_area=A, valid=ok, heading=phi, concentration=kap, harmonic=h, outside=-3.0, origin=(0.1, 0.2),
              sensor_q=(0.2, 1.0))
    prior = pev.raster_prior(grid, 8, strengths=(0.5, 2.0), **kw)
    tab = ref.table(shape, 0.25, strengths=(0.5, 2.0), **kw)
    assert np.array_equal(prior.raster, tab['raster']) and prior.strengths.tolist() == [0.5, 2.0]
    g = ref.log_prior(tab)[0]
    k, a, b = np.meshgrid(np.arange(8), np.arange(9), np.arange(11), indexing='ij')
    assert np.abs(prior.log_prior(k, a, b) - g).max() < 1e-12
    assert (g == -3.0).any() and (g != -3.0).any()


def test_the_second_harmonic_does_not_see_a_reversed_lane():
  shape = (12, 9, 11)
  A, ok, phi, kap = ref.random_raster(8, 9, 4)
  flip = np.random.default_rng(5).random(phi.shape) < 0.5
  g = {}
  for h in (1, 2):
    for name, heading in (('as given', phi), ('reversed', np.where(flip, phi + np.pi, phi))):
      tab = ref.table(shape, 0.25, A, ok, heading, kap, harmonic=h, sensor_q=(0.4, 0.9))
      g[h, name] = ref.log_prior(tab)[0]
  fin = np.isfinite(g[2, 'as given'])
  assert fin.any() and np.abs(g[2, 'as given'][fin] - g[2, 'reversed'][fin]).max() < 1e-4   # (f32 planes of kappa <= 40)
  assert np.abs(g[1, 'as given'][fin] - g[1, 'reversed'][fin]).max() > 1.0


def test_a_constant_raster_is_vote_posterior():
  """A = a constant, kappa = 0, a raster that covers the lattice: log_z_s = the posterior reference's log_z + lambda_s A,
  and ``out`` equals the normalised votes.  (The four f32 weights of an off-centre sensor sum to 1 within 2^-23, so the
  interpolated constant is the constant within 3e-7; a centred sensor has one tap of weight 1 and is held to 1e-9.)"""
  shape = (4, 7, 7)
  v = ref.random_votes(shape, 6)
  const = -1.25
  for sensor, tol in (((0.3, 0.8), 3e-7), (None, 1e-9)):
    tab = ref.table(shape, 0.25, np.full((12, 12), const), heading=np.zeros((12, 12)), concentration=0.0,
                    origin=(-0.75, -0.75), sensor_q=sensor, strengths=ref.LADDERS[3])
    assert (tab['planes'][:, :2] == 0).all() == (sensor is None)
    _constant_raster_case(v, tab, const, tol)


def _constant_raster_case(v, tab, const, tol):
  want = ref.vote_raster(v, tab, 0.7, write=1)
  assert want['count'] == [int(np.isfinite(v).sum()), 0, 0]
  post = pref.vote_posterior(v, np.float32(0.7), None)
  log_z = float(post[2][0])
  for s, lam in enumerate(tab['strengths']):
    assert abs(want['table'][s, 0] - (log_z + lam * const)) < 4 * tol
    assert abs(want['table'][s, 2] - const) < tol and want['table'][s, 3] < tol * tol
    assert abs(want['table'][s, 1] - (lam * const + np.log(v.size))) < 4 * tol
  assert abs(want['stats'][0] - log_z) < 1e-9
  fin = np.isfinite(v)
  assert (np.isfinite(want['out']) == fin).all()
  assert np.abs(want['out'][fin] - (np.float32(0.7) * v[fin].astype(np.float64) - log_z)).max() < 4 * tol


def test_mean_and_variance_are_derivatives_of_log_z():
  shape = (4, 7, 7)
  v = ref.random_votes(shape, 7)
  base = ref.synthetic(shape, 8, S=1, harmonic=1, taps=4, cover='covers', outside=-2.0)
  for lam in (0.25, 1.0, 3.0):
    h = 2.0 ** -10                                              # (lam +- h are f32 numbers)
    rows = []
    for l in (lam - h, lam, lam + h):
      tab = dict(base, strengths=np.array([l]))
      rows.append(ref.vote_raster(v, tab, 0.7)['table'][0])
    d1 = (rows[2][0] - rows[0][0]) / (2 * h)
    d2 = (rows[2][0] - 2 * rows[1][0] + rows[0][0]) / (h * h)
    assert abs(d1 - rows[1][2]) < 1e-5 * (1 + abs(d1)), (lam, d1, rows[1][2])
    assert abs(d2 - rows[1][3]) < 1e-3 * (1 + abs(d2)), (lam, d2, rows[1][3])


def test_the_bound_is_a_function_of_the_input_and_small():
  shape = (36, 31, 33)
  v = ref.random_votes(shape, 9)
  tab = ref.synthetic(shape, 10, S=3, harmonic=2, taps=4, cover='cut')
  b = ref.bound(v, tab, 0.7, write=2, gt=5)
  assert 0 < b['out'].max() < 1e-2 and (b['table'][:, :2] < 1e-4).all() and (b['table'] > 0).all()
  one = ref.bound(v, ref.synthetic(shape, 10, S=3, harmonic=2, taps=1, cover='cut'), 0.7, write=2)
  assert one['out'].max() < b['out'].max()                        # fewer taps, fewer roundings


GRID = grids.Grid2D((5, 6), 0.25)
ZERO = np.zeros((5, 6))
BAD = [
    ('A-nan', dict(log_area=np.where(np.eye(5, 6) > 0, np.nan, 0.0)), 'log_area is not finite'),
    ('A-inf', dict(log_area=np.where(np.eye(5, 6) > 0, -np.inf, 0.0)), 'log_area is not finite'),
    ('heading-nan', dict(log_area=ZERO, heading=np.where(np.eye(5, 6) > 0, np.nan, 0.3)), 'cosine plane is not finite'),
    ('kappa-negative', dict(heading=ZERO, concentration=-0.5), 'concentration'),
    ('kappa-701', dict(heading=ZERO, concentration=701.0), 'concentration'),
    ('kappa-nan', dict(heading=ZERO, concentration=np.nan), 'concentration'),
    ('harmonic-3', dict(log_area=ZERO, harmonic=3), 'harmonic must be 1'),
    ('harmonic-0', dict(log_area=ZERO, harmonic=0), 'harmonic must be 1'),
    ('strength-0', dict(log_area=ZERO, strengths=(1.0, 0.0)), 'strengths must be 1 to 8'),
    ('strength-negative', dict(log_area=ZERO, strengths=(-1.0,)), 'strengths must be 1 to 8'),
    ('strength-inf', dict(log_area=ZERO, strengths=(1e39,)), 'strengths must be 1 to 8'),
    ('strengths-9', dict(log_area=ZERO, strengths=tuple(range(1, 10))), 'strengths must be 1 to 8'),
    ('strengths-none', dict(log_area=ZERO, strengths=()), 'strengths must be 1 to 8'),
    ('offset', dict(log_area=ZERO, origin=(-0.25 * 2.0 ** 24, 0.0)), 'the limit is 2\\^23'),
    ('leaves-f32', dict(log_area=ZERO - 1e30, strengths=(1e8,)), 'leaves f32'),
    ('outside-nan', dict(log_area=ZERO, outside=np.nan), 'outside must be'),
    ('outside-inf', dict(log_area=ZERO, outside=np.inf), 'outside must be'),
    ('nothing', dict(), 'at least one of log_area and heading'),
    ('shapes', dict(log_area=ZERO, heading=np.zeros((5, 5))), r'heading \[X, Y\]'),
]


@pytest.mark.parametrize('kw,match', [row[1:] for row in BAD], ids=[row[0] for row in BAD])
def test_raster_prior_refuses(kw, match):
  with pytest.raises(ValueError, match=match) as info:
    pev.raster_prior(GRID, 8, **kw)
  assert str(info.value).startswith('raster_prior:')


def test_invalid_cells_may_hold_anything_and_the_largest_concentration_is_accepted():
  A = np.where(np.eye(5, 6) > 0, np.nan, -1.0)
  prior = pev.raster_prior(GRID, 8, log_area=A, valid=np.eye(5, 6) == 0, heading=ZERO, concentration=700.0)
  assert np.isfinite(prior.raster).all() and (prior.raster[..., 3] == (np.eye(5, 6) == 0)).all()
  assert abs(prior.raster[0, 1, 0] - (-1.0 - np.log(np.i0(700.0)))) < 1e-4


def test_raster_prior_from_logits():
  rng = np.random.default_rng(11)
  z = rng.standard_normal((5, 6, 3)) * 3
  names = ('building', 'road', 'parking')
  prior = pev.raster_prior_from_logits(z, names, ('road', 'parking'), GRID, 8, floor=0.05)
  p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
  want = np.log(np.maximum(p[..., 1] + p[..., 2], 0.05))
  assert np.abs(prior.raster[..., 0] - want).max() < 1e-6 and (prior.raster[..., 1:3] == 0).all()
  assert want.min() == np.log(0.05)
  same = pev.raster_prior_from_logits(torch.tensor(z), names, (1, 2), GRID, 8, floor=0.05)
  assert np.array_equal(same.raster, prior.raster)
  for kw, match in ((dict(drivable=('river',)), 'must name classes'), (dict(drivable=()), 'at least one'),
                    (dict(drivable=('road',), floor=0.0), 'floor')):
    kw = dict(dict(drivable=('road',), floor=0.05), **kw)
    with pytest.raises(ValueError, match=match):
      pev.raster_prior_from_logits(z, names, kw['drivable'], GRID, 8, floor=kw['floor'])


def test_strength_fit_solves_on_tables_without_a_device():
  """``RasterStrengthFit.add_table`` / ``solve`` on reference tables (CPU tensors): the stationary point lies where the
  summed slope changes sign, and ``solve_temperature`` is the solver."""
  shape = (8, 9, 11)
  A, ok, phi, kap = ref.random_raster(7, 8, 12, invalid=False)
  lad = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0)
  prior = pev.raster_prior(GRID, 8, log_area=A, heading=phi, concentration=kap, outside=-8.0, strengths=lad)
  tab = dict(shape=shape, raster=prior.raster, offsets=prior.offsets, planes=prior.planes, outside=prior.outside,
             strengths=prior.strengths)
  g = ref.log_prior(tab)[0]
  fit = pev.RasterStrengthFit(GRID, 8, prior, temperature=0.7)
  rng = np.random.default_rng(13)
  nll = np.zeros(len(lad))
  for frame in range(6):
    v = ref.random_votes(shape, 20 + frame)
    fin = np.flatnonzero(np.isfinite(v.reshape(-1)))
    p = np.exp(0.7 * v.reshape(-1)[fin] + 0.8 * g.reshape(-1)[fin])        # the truth is drawn at lambda = 0.8
    gt = int(rng.choice(fin, p=p / p.sum()))
    want = ref.vote_raster(v, tab, 0.7, gt=gt)
    stats = np.concatenate([want['stats'], [0.0]])
    fit.add_table(torch.from_numpy(want['table']), torch.from_numpy(stats))
    nll += want['table'][:, 0] - (stats[1] + prior.strengths * stats[2])
  fit.add_table(torch.from_numpy(want['table']), torch.tensor([0.0, np.nan, np.nan, 0.0], dtype=torch.float64))
  out = fit.solve()
  assert out['frames'] == 6 and np.allclose(out['nll'], nll, rtol=0, atol=1e-9)
  assert out['argmin'] == int(np.argmin(nll)) and out['strengths'].tolist() == list(lad)
  if out['bracketed']:
    lo, hi = out['bracket']
    assert lo <= out['strength'] <= hi and abs(lad.index(lo) - out['argmin']) <= 1
  with pytest.raises(ValueError, match='increase strictly'):
    pev.RasterStrengthFit(GRID, 8, pev.raster_prior(GRID, 8, log_area=ZERO, strengths=(2.0, 1.0)))
  empty = pev.RasterStrengthFit(GRID, 8, prior).solve()
  assert empty['frames'] == 0 and np.isnan(empty['strength']) and empty['argmin'] == -1
