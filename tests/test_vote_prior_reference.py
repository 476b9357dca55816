"""CPU: the prior table of ``pose_exhaustive_voting.pose_prior`` against the pose mapping and against the independent
restatement ``vote_prior_reference.table``; the float64 reference of the operator against closed forms; the refusals of
``pose_prior``.  Nothing here needs a GPU or the built library's kernels."""
import numpy as np
import pytest
import torch

import vote_prior_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids

CELL = 0.25


def _grid(shape):
  return grids.Grid2D(((shape[1] + 1) // 2, (shape[2] + 1) // 2), CELL)


def _as_ref(prior):
  return dict(shape=prior.shape, weights=prior.weights, mu=prior.mu, centres=prior.centres, planes=prior.planes,
              comps=prior.comps)


@pytest.mark.parametrize('R,hw', [(4, (5, 8)), (36, (16, 17))])
def test_table_inverts_the_pose_mapping(R, hw):
  """For random (k, a, b) and a random sensor_q: a prior centred at the map position ``exhaustive_indices_to_tfm`` gives
  the sensor has mu_k = (a, b) in plane k.  The mapping is f32; its float64 restatement (``ref.sensor_position``) is
  compared to rounding, and the f32 one to f32 rounding of positions of a few metres."""
  grid = grids.Grid2D(hw, CELL)
  shape = (R, 2 * hw[0] - 1, 2 * hw[1] - 1)
  rng = np.random.default_rng(R)
  for _ in range(20):
    k, a, b = int(rng.integers(R)), int(rng.integers(shape[1])), int(rng.integers(shape[2]))
    sq = rng.uniform(-1.0, 5.0, 2)
    g = ref.sensor_position(shape, CELL, k, a, b, sq)
    tfm = pev.exhaustive_indices_to_tfm(torch.tensor([[k, a, b]], dtype=torch.int32), grid, R)
    ang = float(tfm.angle[0])
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    g32 = rot @ sq + tfm.t[0].numpy().astype(np.float64)
    assert np.abs(g32 - g).max() < 2e-5       # f32 positions of up to ~10 m: a few ulps of 1e-6
    prior = pev.pose_prior(grid, R, position=g, covariance=np.eye(2), sensor_q=sq)
    assert prior.shape == shape
    assert np.abs(prior.mu[0, k] - np.array([a, b])).max() < 1e-11
    mine = ref.table(shape, CELL, g, np.eye(2), sensor_q=sq)
    assert np.abs(prior.mu - mine['mu']).max() < 1e-11


def test_table_split_and_centre_sensor():
  grid = grids.Grid2D((16, 17), CELL)
  R = 36
  prior = pev.pose_prior(grid, R, position=[[1.234, 2.345], [3.3, 0.1]], covariance=[np.eye(2), 2 * np.eye(2)],
                         heading=[0.3, -2.0], concentration=[2.0, 0.0], weights=[1, 3], sensor_q=[0.7, 3.1])
  f = prior.planes[:, :, :2].astype(np.float64)
  assert prior.centres.dtype == np.int32 and prior.planes.dtype == np.float32 and prior.comps.dtype == np.float32
  assert np.abs(f).max() <= 0.5
  assert np.abs(prior.centres + f - prior.mu).max() < 2.0 ** -25     # f is rounded to f32 at magnitude <= 0.5
  assert np.ptp(prior.mu, axis=1).max() > 1.0                         # the lever arm moves the centre with k
  assert (prior.planes[:, :, 2] <= 0).all() and (prior.planes[1, :, 2] == 0).all()
  assert np.allclose(np.exp(prior.comps[:, 3].astype(np.float64)), [0.25, 0.75], rtol=1e-7)
  centre = pev.pose_prior(grid, R, position=[1.234, 2.345], covariance=np.eye(2))
  assert (centre.mu == centre.mu[:, :1]).all() and (centre.centres == centre.centres[:, :1]).all()
  mine = ref.table(prior.shape, CELL, [[1.234, 2.345], [3.3, 0.1]], [np.eye(2), 2 * np.eye(2)], [0.3, -2.0],
                   [2.0, 0.0], [1, 3], [0.7, 3.1])
  assert (mine['centres'] == prior.centres).all()
  assert np.abs(mine['planes'].astype(np.float64) - prior.planes).max() < 1e-6
  assert np.abs(mine['comps'].astype(np.float64) - prior.comps).max() < 1e-6 * np.abs(prior.comps).max()
  u_mine, _ = ref.log_prior(_as_ref(prior))
  k, a, b = np.meshgrid(np.arange(R), np.arange(31), np.arange(33), indexing='ij')
  assert np.abs(prior.log_prior(k, a, b) - u_mine).max() < 1e-9


def _normal_logpdf(x, mean, cov):
  try:
    from scipy import stats
    return stats.multivariate_normal(mean, cov).logpdf(x)
  except ImportError:
    d = x - mean
    prec = np.linalg.inv(cov)
    return -0.5 * np.einsum('...i,ij,...j->...', d, prec, d) - 0.5 * np.log(np.linalg.det(2 * np.pi * cov))


def test_reference_against_closed_forms():
  shape = (8, 9, 11)
  R = shape[0]
  pos, cov = np.array([1.1, 1.7]), np.array([[0.3, 0.1], [0.1, 0.2]])
  sq = np.array([0.4, 2.0])
  tab = ref.table(shape, CELL, pos, cov, heading=0.7, concentration=3.0, sensor_q=sq)
  u, _ = ref.log_prior(tab)
  # differences of u inside a plane = differences of the bivariate normal log-density of the sensor's map position
  for k in (0, 3):
    xy = np.array([[ref.sensor_position(shape, CELL, k, a, b, sq) for b in range(shape[2])] for a in range(shape[1])])
    lp = _normal_logpdf(xy, pos, cov)
    assert np.abs((u[k] - u[k, 0, 0]) - (lp - lp[0, 0])).max() < 1e-5      # the table is f32
  # differences across planes at the sensor-centred table = kappa cos differences
  tab_c = ref.table(shape, CELL, pos, cov, heading=0.7, concentration=3.0)
  uc, _ = ref.log_prior(tab_c)
  yk = 3.0 * np.cos(-2 * np.pi * np.arange(R) / R - 0.7)
  assert np.abs((uc[:, 4, 5] - uc[0, 4, 5]) - (yk - yk[0])).max() < 1e-6
  # two identical components = the single one
  tab2 = ref.table(shape, CELL, [pos, pos], [cov, cov], [0.7, 0.7], [3.0, 3.0], sensor_q=sq)
  u2, _ = ref.log_prior(tab2)
  assert np.abs(u2 - u).max() < 1e-6


@pytest.mark.parametrize('M', ref.COMPONENTS)
def test_gain_and_overlap_signs(M):
  for seed, shape in enumerate(((4, 7, 7), (36, 31, 33))):
    tab = ref.random_table(shape, M, 10 + seed)
    v = ref.random_votes(shape, 20 + seed)
    w = ref.vote_prior(v, tab, 0.7)
    s = w['stats']
    assert (s[4] - s[0]) + s[1] >= -1e-12                   # information gain
    assert (s[0] - s[2]) - s[1] <= 1e-12                    # log overlap
    assert abs(w['resp'].sum() - 1) < 1e-12
    assert abs(ref._lse(w['out'][np.isfinite(w['out'])])) < 1e-12
    bd = ref.bound(v, tab, 0.7)
    assert np.isfinite(bd['stats'][:3]).all() and (bd['out'] >= 0).all() and bd['stats'][0] < 1e-4


def test_two_gaussians_in_turn_equal_their_product():
  shape = (4, 15, 13)
  p1, c1 = np.array([1.0, 1.2]), np.array([[0.2, 0.05], [0.05, 0.3]])
  p2, c2 = np.array([1.4, 0.9]), np.array([[0.4, -0.1], [-0.1, 0.25]])
  prec = np.linalg.inv(c1) + np.linalg.inv(c2)
  c12 = np.linalg.inv(prec)
  p12 = c12 @ (np.linalg.inv(c1) @ p1 + np.linalg.inv(c2) @ p2)
  sq = np.array([0.3, 1.9])
  v = ref.random_votes(shape, 5)
  first = ref.vote_prior(v, ref.table(shape, CELL, p1, c1, sensor_q=sq), 1.3)
  second = ref.vote_prior(first['out'].astype(np.float32), ref.table(shape, CELL, p2, c2, sensor_q=sq), 1.0)
  both = ref.vote_prior(v, ref.table(shape, CELL, p12, c12, sensor_q=sq), 1.3)
  fin = np.isfinite(both['out'])
  assert (fin == np.isfinite(second['out'])).all()
  assert np.abs(second['out'][fin] - both['out'][fin]).max() < 2e-4       # f32 tables, `out` rounded to f32 in between


def test_pose_prior_refusals():
  grid = grids.Grid2D((16, 17), CELL)
  ok = dict(position=[1.0, 2.0], covariance=np.eye(2))
  pev.pose_prior(grid, 36, **ok)
  pev.pose_prior(grid, 36, heading=0.3, concentration=500.0)
  bad = [
      dict(),                                                                      # neither term
      dict(position=[np.nan, 2.0], covariance=np.eye(2)),                         # non-finite
      dict(position=[1.0, 2.0], covariance=[[np.inf, 0.0], [0.0, np.inf]]),
      dict(heading=np.inf),
      dict(heading=0.1, concentration=np.nan),
      dict(ok, sensor_q=[np.nan, 0.0]),
      dict(ok, weights=[np.inf]),
      dict(position=[1.0, 2.0], covariance=[[1.0, 2.0], [2.0, 1.0]]),             # not positive definite
      dict(position=[1.0, 2.0], covariance=[[1.0, 0.5], [0.4, 1.0]]),             # not symmetric
      dict(position=[1.0, 2.0], covariance=-np.eye(2)),
      dict(position=np.zeros((9, 2)), covariance=np.stack([np.eye(2)] * 9)),      # M = 9
      dict(position=np.zeros((0, 2)), covariance=np.zeros((0, 2, 2))),            # M = 0
      dict(position=np.zeros((2, 2)), covariance=np.stack([np.eye(2)] * 3)),      # mismatched
      dict(position=np.zeros((2, 2)), covariance=np.stack([np.eye(2)] * 2), weights=[1.0, 1.0, 1.0]),
      dict(position=np.zeros((2, 2)), covariance=np.stack([np.eye(2)] * 2), heading=[0.1, 0.2, 0.3]),
      dict(ok, weights=[0.0]),
      dict(heading=0.1, concentration=-1.0),
      dict(position=[1.0, 2.0], covariance=np.eye(2) * 1e-38),                    # the quadratic form leaves f32
      dict(position=[1.0, 2.0]),                                                  # position without covariance
  ]
  for kw in bad:
    with pytest.raises(ValueError, match='pose_prior'):
      pev.pose_prior(grid, 36, **kw)
  with pytest.raises(ValueError, match='pose_prior'):
    pev.pose_prior(grid, 65, **ok)


def test_prior_votes_refuses_a_foreign_table():
  grid = grids.Grid2D((16, 17), CELL)
  prior = pev.pose_prior(grid, 36, position=[1.0, 2.0], covariance=np.eye(2))
  with pytest.raises(ValueError, match='prior_votes'):
    pev.prior_votes(None, prior, grids.Grid2D((8, 8), CELL), 36, device='cuda')
  with pytest.raises(ValueError, match='prior_votes'):
    pev.prior_votes(None, object(), grid, 36, device='cuda')
