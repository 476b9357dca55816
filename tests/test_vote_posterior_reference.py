"""CPU pins of the pose-distribution contract (snap_vote_posterior_f32, include/snap_hip.h): the float64 numpy
restatement ``vote_posterior_reference`` against ``scipy.special.logsumexp`` and brute-force sums, its identities, the
documented error bound against a float32 restatement of the kernel's two-level summation on every input of the GPU
tests, and the C entry points' argument validation (no launch)."""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import vote_posterior_reference as ref
from snap_amd import _lib


def _brute(v, scale, gt=None):
  """Plain loops over the cells."""
  R, Ho, Wo = v.shape
  cells = [(r, a, b, float(np.float32(scale)) * float(v[r, a, b])) for r in range(R) for a in range(Ho)
           for b in range(Wo) if np.isfinite(v[r, a, b])]
  m = max(c[3] for c in cells)
  z = sum(np.exp(c[3] - m) for c in cells)
  log_z = m + np.log(z)
  p = [np.exp(c[3] - log_z) for c in cells]
  ea = sum(q * c[1] for q, c in zip(p, cells))
  eb = sum(q * c[2] for q, c in zip(p, cells))
  C = sum(q * np.cos(2 * np.pi * c[0] / R) for q, c in zip(p, cells))
  S = sum(q * np.sin(2 * np.pi * c[0] / R) for q, c in zip(p, cells))
  return dict(log_z=log_z, max_x=m, E_a=ea, E_b=eb,
              Var_a=sum(q * (c[1] - ea) ** 2 for q, c in zip(p, cells)),
              Cov_ab=sum(q * (c[1] - ea) * (c[2] - eb) for q, c in zip(p, cells)),
              Var_b=sum(q * (c[2] - eb) ** 2 for q, c in zip(p, cells)), C=C, S=S,
              mean_r=(np.arctan2(S, C) * R / (2 * np.pi)) % R, resultant=np.hypot(C, S),
              entropy=-sum(q * np.log(q) for q in p if q > 0))


@pytest.mark.parametrize('shape', [(4, 7, 7), (1, 5, 5), (3, 1, 1), (6, 4, 9)])
@pytest.mark.parametrize('scale', [1.0, 30.0])
def test_reference_equals_scipy_and_brute_force(shape, scale):
  v = ref.random_votes(shape, seed=3)
  lxy, lr, st, cnt = ref.vote_posterior(v, scale)
  x = np.float64(np.float32(scale)) * v.astype(np.float64)
  with np.errstate(divide='ignore'):
    assert np.isclose(st[0], logsumexp(x), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lxy, logsumexp(x, axis=0) - logsumexp(x), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lr, logsumexp(x, axis=(1, 2)) - logsumexp(x), rtol=0, atol=1e-12)
  want = _brute(v, scale)
  for n, name in enumerate(ref.STAT_NAMES[:12]):
    assert np.isclose(st[n], want[name], rtol=0, atol=1e-9), name
  assert cnt.tolist() == [int(np.isfinite(v).sum()), 0, 0] and np.isnan(st[12]) and (st[13:] == 0).all()


def test_identities():
  v = ref.random_votes((5, 6, 7), seed=1)
  lxy, lr, st, _ = ref.vote_posterior(v, 3.0, (1.5, 2.5, 3.5))
  assert abs(logsumexp(lxy)) < 1e-12 and abs(logsumexp(lr)) < 1e-12
  # votes + c (exactly representable shift): everything but log_z and max x is unchanged
  v2 = (np.where(np.isfinite(v), np.round(v * 64) / 64, v)).astype(np.float32)
  a = ref.vote_posterior(v2, 2.0, (1.5, 2.5, 3.5))
  b = ref.vote_posterior((v2 + np.float32(8)).astype(np.float32), 2.0, (1.5, 2.5, 3.5))
  np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-11)
  np.testing.assert_allclose(a[1], b[1], rtol=0, atol=1e-11)
  np.testing.assert_allclose(a[2][2:], b[2][2:], rtol=0, atol=1e-10)
  assert np.isclose(b[2][0] - a[2][0], 16.0) and np.isclose(b[2][1] - a[2][1], 16.0)
  assert a[3].tolist() == b[3].tolist()


def test_empty_single_cell_and_bad_cells():
  lxy, lr, st, cnt = ref.vote_posterior(np.full((3, 4, 5), -np.inf, np.float32))
  assert (lxy == -np.inf).all() and (lr == -np.inf).all() and st[0] == st[1] == -np.inf
  assert np.isnan(st[2:13]).all() and (st[13:] == 0).all() and cnt.tolist() == [0, 0, 0]
  v, c = ref.single_cell_votes((6, 5, 7), -3.25)
  lxy, lr, st, cnt = ref.vote_posterior(v, 2.0)
  assert st[0] == st[1] == -6.5 and st[2] == c[1] and st[3] == c[2] and (st[4:7] == 0).all() and st[11] == 0
  assert np.isclose(st[9], c[0]) and np.isclose(st[10], 1) and cnt.tolist() == [1, 0, 0]
  assert lxy[c[1], c[2]] == 0 and np.isinf(np.delete(lxy.reshape(-1), c[1] * 7 + c[2])).all()
  bad, masked, n = ref.nan_inf_votes()
  gb, gm = ref.vote_posterior(bad, 30.0), ref.vote_posterior(masked, 30.0)
  assert gb[3].tolist() == [gm[3][0], n, 0] and gm[3][1] == 0
  for x, y in zip(gb[:3], gm[:3]):
    np.testing.assert_array_equal(x, y)


def test_ground_truth_sample():
  v, cases = ref.gt_cases()
  R = v.shape[0]
  for name, idx, valid in cases:
    _, _, st, cnt = ref.vote_posterior(v, 3.0, idx)
    assert cnt[2] == valid, name
    assert np.isnan(st[12]) == (not valid), name
  x = 3.0 * v.astype(np.float64)
  lz = logsumexp(x)
  assert np.isclose(ref.vote_posterior(v, 3.0, (2.0, 4.0, 9.0))[2][12], x[2, 4, 9] - lz)
  assert np.isclose(ref.vote_posterior(v, 3.0, (R - 0.25, 6.0, 6.0))[2][12], 0.25 * x[R - 1, 6, 6] + 0.75 * x[0, 6, 6] - lz)
  want = sum(0.125 * x[k, i, j] for k in (7, 8) for i in (3, 4) for j in (20, 21))
  assert np.isclose(ref.vote_posterior(v, 3.0, (7.5, 3.5, 20.5))[2][12], want - lz)


@pytest.mark.parametrize('case', ref.all_inputs(), ids=lambda c: c[0].replace(' ', ''))
def test_f32_two_level_scheme_stays_inside_the_bound(case):
  """The bound is not too tight (a float32 restatement of the kernel's rounding points stays inside it) and not
  vacuous (it is far below the outputs' own scale where the input is benign)."""
  name, v, scale, gt = case
  want = ref.vote_posterior(v, scale, gt)
  got = ref.two_level_f32(v, scale, gt)
  tol_xy, tol_r, tol_s = ref.bound(v, scale, gt)
  with np.errstate(invalid='ignore'):
    for g, w, tol, what in ((got[0], want[0], tol_xy, 'log_prob_xy'), (got[1], want[1], tol_r, 'log_prob_r')):
      assert ((g == w) | (np.abs(g - w) <= tol)).all(), what
  R = v.shape[0]
  for n, nm in enumerate(ref.STAT_NAMES):
    g, w = float(got[2][n]), float(want[2][n])
    if np.isnan(w) or np.isinf(w):
      assert np.isnan(g) == np.isnan(w) and (np.isnan(w) or g == w), nm
      continue
    err = abs(g - w)
    if n == 9:
      err = min(err, R - err)
    assert err <= tol_s[n], (nm, g, w, tol_s[n])
  assert got[3].tolist() == want[3].tolist()
  if name.startswith('random') and scale == 1.0:
    assert tol_xy.max() < 1e-4 and tol_r.max() < 1e-4 and tol_s[0] < 1e-4 and tol_s[11] < 1e-4


def test_a_single_precision_second_moment_breaks_the_bound():
  """What the bound is for: E[a^2] - E[a]^2 with f32 sums misses it on the sharp far-corner peak."""
  v = ref.peak_votes()
  _, _, st, _ = ref.vote_posterior(v, 1.0)
  tol = ref.bound(v, 1.0)[2]
  p = np.exp(v.astype(np.float64) - st[0]).sum(0).astype(np.float32)
  a = np.arange(v.shape[1], dtype=np.float32)[:, None]
  w = np.float32(p.sum(dtype=np.float32))
  ea = (p * a).sum(dtype=np.float32) / w
  var32 = (p * a * a).sum(dtype=np.float32) / w - ea * ea
  assert abs(float(var32) - st[4]) > 2 * tol[4]


def test_entry_points_validate_before_any_launch():
  """Status codes for bad arguments with dummy non-null pointers: nothing is launched (CPU-safe)."""
  lib = _lib.load()
  one = ctypes.c_void_p(16)
  ws_bytes = lib.snap_vote_posterior_workspace_bytes

  def call(R=36, Ho=31, Wo=33, scale=1.0, votes=one, lxy=one, lr=one, stats=one, count=one, ws=one, nbytes=None):
    nbytes = ws_bytes(R, Ho, Wo) if nbytes is None else nbytes
    return lib.snap_vote_posterior_f32(votes, R, Ho, Wo, scale, None, lxy, lr, stats, count, ws, nbytes, None)

  need = ws_bytes(36, 31, 33)
  assert need > 0 and need % 8 == 0 and ws_bytes(36, 511, 511) > 0 and ws_bytes(64, 1, 1) > 0
  for kw in (dict(R=65), dict(R=0), dict(Ho=0), dict(Wo=-1), dict(R=64, Ho=8192, Wo=8192)):
    full = dict(dict(R=36, Ho=31, Wo=33), **kw)
    assert ws_bytes(full['R'], full['Ho'], full['Wo']) == 0, kw
    assert call(nbytes=1 << 30, **kw) == -1, kw
    assert not ref.supported((full['R'], full['Ho'], full['Wo']))
  for scale in (0.0, -1.0, float('inf'), float('nan')):
    assert call(scale=scale) == -2, scale
  for name in ('votes', 'lxy', 'lr', 'stats', 'count', 'ws'):
    assert call(**{name: None}) == -3, name
  assert call(nbytes=need - 1) == -5 and call(nbytes=0) == -5
  assert call(ws=ctypes.c_void_p(20)) == -5
