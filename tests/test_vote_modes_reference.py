"""The float64 restatement ``vote_modes_reference`` checked against what it must equal by construction, and the host
side of ``modes_from_votes`` (``nees_table``, the pose Jacobian) against independent computations.  No GPU."""
import math

import numpy as np
import pytest
import torch

import vote_modes_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids


@pytest.mark.parametrize('shape,K,win_r,win_xy', [((4, 5, 7), 16, 1, 4), ((4, 5, 7), 3, 0, 1), ((8, 31, 33), 16, 1, 4),
                                                  ((8, 31, 33), 5, 3, 32), ((8, 31, 33), 64, 2, 16)])
def test_ownership_agrees_with_the_literal_loops(shape, K, win_r, win_xy):
  peaks = ref.random_peaks(shape, K, seed=K)
  peaks[K // 2] = -1                                          # an empty row
  if K > 4:
    peaks[K - 1] = peaks[1]                                   # a duplicate
  owner, off = ref.ownership(shape, peaks, win_r, win_xy)
  assert (owner == ref.ownership_loops(shape, peaks, win_r, win_xy)).all()
  assert not (owner == K // 2).any() and (K <= 4 or not (owner == K - 1).any())
  owned = owner >= 0
  assert (np.abs(off[0][owned]) <= win_r).all() and (np.abs(off[1:][:, owned]) <= win_xy).all()


def test_ownership_on_the_special_tables():
  for c in ref.special_cases():
    if c['votes'].shape != (8, 31, 33) or c['win_xy'] > 16:
      continue
    owner, _ = ref.ownership(c['votes'].shape, c['peaks'], c['win_r'], c['win_xy'])
    assert (owner == ref.ownership_loops(c['votes'].shape, c['peaks'], c['win_r'], c['win_xy'])).all(), c['name']
    if c['name'] == 'ties_w1_4':
      assert (owner[2, 6:15, 12] == 0).all() and (owner[2, 10, 11] == 1) and (owner[2, 10, 13] == 0)
    if c['name'] == 'duplicate_w1_4':
      assert not (owner == 2).any() and not (owner == 4).any() and (owner == 3).any()
    if c['name'] == 'empty_rows_w1_4':
      assert set(np.unique(owner)) == {-1, 1, 13}


@pytest.mark.parametrize('case', ref.cases(), ids=lambda c: c['name'])
def test_partition_and_total_mass(case):
  """Every cell has at most one owner (one owner map), the modes' counts are the owned cells, and the masses of the
  modes plus the mass nobody owns are the whole: sum_k exp(log_mass_k) + unowned = exp(log_z) to 1e-12 relative."""
  v, scale = case['votes'], case['scale']
  stats, count, owner = ref.vote_modes(v, case['peaks'], case['win_r'], case['win_xy'], scale, case['gt'])
  finite = np.isfinite(v)
  K = len(case['peaks'])
  assert count[:, 0].sum() == int((finite & (owner >= 0)).sum())
  assert count[:, 1].sum() == int(((np.isnan(v) | (v == np.inf)) & (owner >= 0)).sum())
  assert (stats[:, 12:] == 0).all()
  for k in range(K):
    assert (count[k, 0] == 0) == (stats[k, 0] == -np.inf) == bool(np.isnan(stats[k, 2:11]).all())
  lz = ref.log_z(v, scale)
  if not np.isfinite(lz):
    assert (stats[:, 0] == -np.inf).all()
    return
  x = float(np.float32(scale)) * v.astype(np.float64)
  unowned = np.exp(x[finite & (owner < 0)] - lz).sum()
  total = np.exp(stats[:, 0] - lz).sum() + unowned
  assert abs(total - 1.0) <= 1e-12
  if case['gt'] is not None:
    assert ref.nees_condition(stats) <= 1e4


def _lattice_gaussian_bounds(sigma, delta, w):
  """One axis of a discretised Gaussian exp(-(n - delta)^2 / 2 sigma^2) over the integers n (offsets from the peak),
  truncated to |n| <= w -> (bound on |mean - delta|, bound on |variance - sigma^2|), derived, not tuned:

  TRUNCATION.  With p the distribution on all integers, eps = p(|n| > w), T1 = sum_{|n| > w} p |n|, T2 the same with
  n^2: E_w[f] - E[f] = eps E_w[f] - sum_{|n| > w} p f, so |mean_w - mean| <= eps w + T1 and |E_w[n^2] - E[n^2]| <=
  eps w^2 + T2, and the variances differ by at most that plus (|mean_w| + |mean|) (eps w + T1).
  DISCRETISATION.  By Poisson summation sum_n exp(-(n - mu)^2 / 2 sigma^2) is proportional to 1 + f(mu),
  f = 2 sum_k q^(k^2) cos(2 pi k mu), q = exp(-2 pi^2 sigma^2); mean - mu = sigma^2 (log(1 + f))' and
  variance - sigma^2 = sigma^4 (log(1 + f))'', bounded through F_j = 2 sum_k q^(k^2) (2 pi k)^j."""
  n = np.arange(-400, 401).astype(np.float64)
  p = np.exp(-0.5 * ((n - delta) / sigma) ** 2)
  p /= p.sum()
  out = np.abs(n) > w
  eps, T1, T2 = p[out].sum(), (p[out] * np.abs(n[out])).sum(), (p[out] * n[out] ** 2).sum()
  mean = (p * n).sum()
  mean_w_bound = abs(mean) + eps * w + T1
  trunc_mean = eps * w + T1
  trunc_var = eps * w * w + T2 + (mean_w_bound + abs(mean)) * trunc_mean
  k = np.arange(1, 12).astype(np.float64)
  q = math.exp(-2 * math.pi ** 2 * sigma ** 2)
  F0, F1, F2 = (2 * (q ** (k * k) * (2 * math.pi * k) ** j).sum() for j in (0, 1, 2))
  disc_mean = sigma ** 2 * F1 / (1 - F0)
  disc_var = sigma ** 4 * (F2 / (1 - F0) + (F1 / (1 - F0)) ** 2)
  return trunc_mean + disc_mean, trunc_var + disc_var, trunc_mean


def test_separable_gaussian():
  """Log-votes of a separable Gaussian with sigma = (0.8, 2.5, 1.7) cells centred off the lattice, one peak at the
  nearest cell, window (4, 16).  Every lattice cell outside the window is further than 5 sigma from the centre on its
  axis (r: 4.5 cells = 5.6 sigma, the largest window the contract has; a: 16.7 = 6.7 sigma; b: 16.6 = 9.8 sigma).

  The covariance is within the derived truncation + discretisation bound of diag(sigma^2) and the mean within the same
  kind of bound of the centre (``_lattice_gaussian_bounds``).  On the rotation axis sigma = 0.8 is narrow enough for
  the lattice to matter: a discretised Gaussian's mean is off its centre by up to 4 pi sigma^2 exp(-2 pi^2 sigma^2) =
  2.6e-5, times sin(2 pi offset).  The centre is therefore half a cell off the lattice in r, where that term vanishes
  by symmetry; the mean is then within 1e-6 on every axis, truncation included (3.1e-7 in r)."""
  sigma = np.array([0.8, 2.5, 1.7])
  shape, peak, delta = (12, 41, 41), np.array([6, 20, 20]), np.array([0.5, 0.3, -0.4])
  win_r, win_xy = 4, 16
  centre = peak + delta
  g = [-0.5 * ((np.arange(n) - c) / s) ** 2 for n, c, s in zip(shape, centre, sigma)]
  v = (g[0][:, None, None] + g[1][None, :, None] + g[2][None, None, :]).astype(np.float64)
  v32 = v.astype(np.float32)
  stats, count, owner = ref.vote_modes(v32, peak[None].astype(np.int32), win_r, win_xy, 1.0)
  assert count[0].tolist() == [9 * 33 * 33, 0]
  # The op takes f32 votes: rounding the log-votes multiplies weight i by exp(eta_i), eta_i = v32_i - v_i.  To first
  # order an expectation E[f] moves by sum p_i eta_i (f_i - E[f]), at most 2 sum p_i |eta_i| |f_i|; 2.1 covers the
  # higher orders (|eta| <= 4e-6).  Computed from the actual eta, so it is as small as the perturbation is.
  mine = owner == 0
  eta = np.abs(v32.astype(np.float64) - v)[mine]
  p = np.exp(v[mine] - v[mine].max())
  p /= p.sum()
  d = np.stack(np.nonzero(mine)).astype(np.float64) - peak[:, None]           # offsets from the peak [3, n]
  e_abs = np.abs(stats[0, 2:5] - peak)
  r1 = np.array([2.1 * (p * eta * np.abs(d[i])).sum() for i in range(3)])
  r2 = np.array([[2.1 * (p * eta * np.abs(d[i] * d[j])).sum() for j in range(3)] for i in range(3)])
  r_cov = r2 + (e_abs[:, None] + r1[:, None]) * r1[None] + (e_abs[None] + r1[None]) * r1[:, None]
  mean_err = np.abs(stats[0, 2:5] - centre)
  cov = np.array([[stats[0, 5], stats[0, 6], stats[0, 7]], [stats[0, 6], stats[0, 8], stats[0, 9]],
                  [stats[0, 7], stats[0, 9], stats[0, 10]]])
  for i, w in enumerate((win_r, win_xy, win_xy)):
    mean_bound, var_bound, trunc_mean = _lattice_gaussian_bounds(sigma[i], delta[i], w)
    print(f'axis {i}: |mean - centre| {mean_err[i]:.3e} (bound {mean_bound:.3e} + rounding {r1[i]:.3e}; truncation '
          f'alone {trunc_mean:.3e}), |var - sigma^2| {abs(cov[i, i] - sigma[i] ** 2):.3e} (bound {var_bound:.3e} + '
          f'rounding {r_cov[i, i]:.3e})')
    assert mean_err[i] <= mean_bound + r1[i]
    assert trunc_mean + r1[i] <= 1e-6 and mean_err[i] <= 1e-6
    assert abs(cov[i, i] - sigma[i] ** 2) <= var_bound + r_cov[i, i]
  off = cov - np.diag(np.diag(cov))
  # (separable weights over a box: the off-diagonal central moments vanish but for the rounding of the votes)
  print(f'off-diagonal: {np.abs(off).max():.3e} (rounding {r_cov.max():.3e})')
  assert (np.abs(off) <= r_cov + 1e-12).all()


def test_nees_table_quantiles_and_coverage():
  levels = (0.5, 0.9, 0.99)
  quant = [pev.chi2_3_quantile(q) for q in levels]
  for q, x in zip(levels, quant):
    assert abs(pev._chi2_3_cdf(x) - q) <= 1e-12
  try:
    from scipy.stats import chi2
  except ImportError:
    chi2 = None
  if chi2 is not None:
    assert np.allclose(quant, chi2.ppf(levels, 3), rtol=1e-10, atol=0)
  else:                                                        # (Abramowitz & Stegun, table 26.8, 3 degrees of freedom)
    assert np.allclose(quant, [2.36597, 6.25139, 11.3449], rtol=2e-6)
  rng = np.random.default_rng(3)
  n = 20000
  L = rng.standard_normal((3, 3)) + 2 * np.eye(3)
  cov = L @ L.T
  e = rng.standard_normal((n, 3)) @ L.T
  nees = np.einsum('ni,ij,nj->n', e, np.linalg.inv(cov), e)
  table = pev.nees_table(torch.from_numpy(nees), levels)
  assert table['count'] == n and np.allclose(table['quantile'], quant)
  for q, c in zip(levels, table['coverage']):
    assert abs(c - q) <= 3 * math.sqrt(q * (1 - q) / n), (q, c)
  # NaN samples and the mask drop out; too small a covariance shows as under-coverage
  with_nan = np.concatenate([nees, [np.nan, np.nan]])
  valid = np.ones(n + 2, dtype=bool)
  valid[:10] = False
  assert pev.nees_table(with_nan, levels, valid)['count'] == n - 10
  assert (pev.nees_table(4 * nees, levels)['coverage'] < np.array(levels) - 0.1).all()
  assert pev.nees_table([], levels)['count'] == 0


def test_pose_jacobian_against_finite_differences():
  R, extent, cell = 36, (32, 32), 0.25
  grid = grids.Grid2D(extent, cell)
  rng = np.random.default_rng(11)
  index = np.stack([rng.uniform(0, R, 6), rng.uniform(0, 62, 6), rng.uniform(0, 62, 6)], -1)
  angle, t, J = pev._mode_pose_and_jacobian(torch.from_numpy(index), grid, R)
  h = 1e-5
  for n, idx in enumerate(index):
    want = ref.index_to_pose(idx, extent, cell, R)
    got = np.array([float(angle[n]), float(t[n, 0]), float(t[n, 1])])
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the single-index entry point of the model, f32: the same pose
    tf = pev.exhaustive_index_to_tfm(torch.tensor(idx, dtype=torch.float64), grid, R)
    assert abs(float(tf.angle) - want[0]) <= 1e-5 and np.abs(tf.t.numpy() - want[1:]).max() <= 1e-5
    fd = np.zeros((3, 3))
    for j in range(3):
      d = np.zeros(3)
      d[j] = h
      fd[:, j] = (ref.index_to_pose(idx + d, extent, cell, R) - ref.index_to_pose(idx - d, extent, cell, R)) / (2 * h)
    # (central differences: h^2 / 6 times a third derivative <= (2 pi / R)^3 * 8 m, plus rounding 1e-16 * 8 m / h)
    assert np.abs(J[n].numpy() - fd).max() <= 1e-9
    assert np.abs(ref.pose_jacobian(idx, extent, cell, R) - fd).max() <= 1e-9
    assert abs(J[n, 1, 0]) > 1e-3 or abs(J[n, 2, 0]) > 1e-3     # the translation does depend on the rotation index


def test_reference_modes_propagation():
  """cov = J Sigma J^T of the reference's wrapper against a Monte-Carlo-free check: a rotation-only covariance moves
  the corner-frame translation along d t / d k."""
  R, extent, cell = 8, (16, 16), 0.25
  stats = np.zeros((2, 16), dtype=np.float32)
  stats[0, :5] = (-1.0, -2.0, 3.25, 12.5, 20.0)
  stats[0, 5] = 0.04
  stats[1, :2] = -np.inf
  stats[1, 2:12] = np.nan
  out = ref.modes(stats, 0.0, extent, cell, R)
  J = ref.pose_jacobian(stats[0, 2:5], extent, cell, R)
  assert np.allclose(out['cov'][0], float(stats[0, 5]) * np.outer(J[:, 0], J[:, 0]), rtol=1e-12)
  assert np.isnan(out['pose'][1]).all() and out['weight'][1] == 0 and abs(out['weight'][0] - math.exp(-1)) < 1e-15
  assert abs(out['unassigned'] - (1 - math.exp(-1))) < 1e-15
