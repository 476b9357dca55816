"""`-m gpu`: ``ops.prior_volume`` (vote_prior.hip, through the C ABI) and the host entry points built on it
(``prior_votes``, ``VoteFilter.apply_prior``, ``localize_exhaustive(prior=...)``), against the float64 numpy restatement
``vote_prior_reference`` within twice its documented error bound (a function of the input: the reference module's
docstring).

Launches 1 and 2 tile the pixels p = a * Wo + b into runs of 256, one workgroup each (up to 1024 workgroups, then
several tiles per workgroup), one kernel instance per number of components M.  ``[1, 5, 5]`` and ``[3, 1, 1]``: the
smallest extents (launch 4 then has only its scalar head / tail cells); ``[4, 7, 7]``: one partial tile; ``[36, 31,
33]``: four tiles, a ragged last one, Ho != Wo; ``[64, 5, 300]``: the largest R; ``[2, 520, 520]``: 1057 tiles on 1024
workgroups (the float64 accumulators carry over a second tile); M in {1, 3, 8}.  Every call runs under
``guarded.scope()``: guard regions intact (outputs and workspace), the workspace as large as the query says, no output
element left unwritten.

Observed on an MI355X (each test prints its figures; ``test_the_shares_of_the_bound`` the worst of the module): the
bound is a worst-case sum over the rounding points, and the largest observed share of it is 0.87 on ``out`` (a centred
sensor, M = 1, ``[36, 31, 33]``), 0.20 on log_z, 0.22 on log_z_votes, 0.05 on log_z_prior, 0.10 on log_z_prior_F, 0.07 on
E_post[u] and 0.09 on the responsibilities (2 allowed); the flat prior differs from ``ops.vote_posterior``'s log_z by
1.2e-7 where the bounds sum to 1.1e-5; two priors in turn differ from their product by 7.6e-6 (8.4e-5 allowed)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_posterior_reference as pref
import vote_prior_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
SHARES = {}


def _prior(tab):
  return pev.PosePrior(tab['shape'], tab['weights'], tab['mu'], tab['centres'], tab['planes'], tab['comps'])


def _run(v, tab, scale=1.0, prior=None):
  """One guarded call -> numpy (out, resp, stats, count)."""
  prior = prior or _prior(tab)
  R, Ho, Wo = tab['shape']
  M = tab['comps'].shape[0]
  votes = None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
  with guarded.scope() as sc:
    out = ops.prior_volume(None if votes is None else guarded.place(votes, 'value'), prior, scale, device=DEV)
    assert [tuple(o.shape) for o in out] == [(R, Ho, Wo), (M,), (8,), (4,)]
    assert [o.dtype for o in out] == [torch.float32, torch.float64, torch.float64, torch.int32]
    ws = [a for a in sc.allocations('prior_volume') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_prior_workspace_bytes(R, Ho, Wo, M)
    for o, what in zip(out, ('out', 'resp', 'stats', 'count')):
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  assert (res[2][5:] == 0).all() and res[3][3] == 0
  return res


def _share(err, tol):
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(err == 0, 0.0, np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.inf))


def _assert_within(got, want, tol, factor=2.0, what=''):
  out, resp, stats, count = got
  assert count[:2].tolist() == want['count'], f'{what}: count {count.tolist()} != {want["count"]}'
  assert want['zero_lo'] <= count[2] <= want['zero_hi'], (what, count[2], want['zero_lo'], want['zero_hi'])
  w = want['out']
  assert ((out == -np.inf) == (w == -np.inf)).all() and not np.isnan(out).any(), f'{what}: -inf pattern'
  fin = np.isfinite(w)
  shares = {}
  e = np.abs(out.astype(np.float64)[fin] - w[fin])
  shares['out'] = float(_share(e, tol['out'][fin]).max()) if fin.any() else 0.0
  assert (e <= factor * tol['out'][fin]).all(), f'{what}: out, {int((e > factor * tol["out"][fin]).sum())} cells outside'
  for i, name in enumerate(ref.STATS):
    g, x, b = stats[i], want['stats'][i], tol['stats'][i]
    if not np.isfinite(x) or (b == np.inf):
      assert b == np.inf or (np.isnan(g) and np.isnan(x)) or g == x, f'{what}: {name} {g} vs {x}'
      continue
    shares[name] = float(_share(np.abs(g - x), np.float64(b)))
    assert abs(g - x) <= factor * b, f'{what}: {name} {g!r} vs {x!r}, bound {b:.3e}'
  if np.isnan(want['resp']).any():
    assert np.isnan(resp).all()
  elif resp.size == 1:
    assert resp[0] == 1.0, f'{what}: resp of one component is exactly 1, got {resp[0]!r}'
  else:
    e = np.abs(resp - want['resp'])
    shares['resp'] = float(_share(e, tol['resp']).max())
    assert (e <= factor * tol['resp']).all(), f'{what}: resp {resp} vs {want["resp"]}, bound {tol["resp"]}'
    rb = float(tol['resp'].sum())
    assert abs(resp.sum() - 1) <= factor * rb, f'{what}: resp sums to {resp.sum()!r}'
  SHARES[what] = shares
  print(f'{what}: largest share of the bound', {k: round(v, 4) for k, v in shares.items()})


def _check(v, tab, scale, what):
  got = _run(v, tab, scale)
  _assert_within(got, ref.vote_prior(v, tab, scale), ref.bound(v, tab, scale), what=what)
  return got


@pytest.mark.parametrize('M', ref.COMPONENTS)
@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_random_shapes(shape, M):
  """Random votes with -inf patches; random components (Pxy != 0, kappa from {0, 2, 500}, a sensor off the centre)."""
  seed = sum(shape) + M
  _check(ref.random_votes(shape, seed), ref.random_table(shape, M, seed + 1), 0.7, f'random{shape}_M{M}')


def test_several_tiles_per_workgroup():
  v = ref.fold_votes()
  assert v.shape[1] * v.shape[2] > ref.MAX_GROUPS * ref.TILE
  for M in (1, 8):
    _check(v, ref.random_table(ref.FOLD_SHAPE, M, 5 + M, sigma_cells=40.0), 1.0, f'fold_M{M}')


@pytest.mark.parametrize('M', (1, 3))
def test_centre_outside_tight_and_wide(M):
  shape = (36, 31, 33)
  v = ref.random_votes(shape, 3)
  _check(v, ref.random_table(shape, M, 11, outside=True), 1.0, f'outside_M{M}')
  _check(v, ref.random_table(shape, M, 12, sigma_cells=0.5), 1.0, f'tight_M{M}')
  _check(v, ref.random_table(shape, M, 13, sigma_cells=400.0), 1.0, f'wide_M{M}')
  for kappa in (0.0, 2.0, 500.0):
    _check(v, ref.random_table(shape, M, 14, kappa=kappa), 2.5, f'kappa{kappa:g}_M{M}')
  _check(v, ref.random_table(shape, M, 15, sensor=False, cross=False), 1.0, f'centre_sensor_M{M}')


def test_without_votes_the_prior_is_a_belief():
  """votes=None: logsumexp(out) = 0 within the bound, every cell finite, and ``ops.vote_peaks`` finds the component's
  rounded centre in the plane nearest the heading."""
  shape = (36, 31, 33)
  grid = grids.Grid2D((16, 17), 0.25)
  prior = pev.pose_prior(grid, 36, position=[2.3, 1.9], covariance=[[0.2, 0.05], [0.05, 0.3]], heading=-2 * np.pi * 7 / 36,
                         concentration=20.0)
  tab = dict(shape=prior.shape, weights=prior.weights, mu=prior.mu, centres=prior.centres, planes=prior.planes,
             comps=prior.comps)
  got = _run(None, tab, prior=prior)
  want, tol = ref.vote_prior(None, tab), ref.bound(None, tab)
  _assert_within(got, want, tol, what='no_votes')
  assert got[3].tolist()[:2] == [36 * 31 * 33, 0] and np.isfinite(got[0]).all()
  assert abs(ref._lse(got[0].astype(np.float64))) <= 2 * (tol['stats'][0] + 2.0 ** -24 * np.abs(want['out']).max())
  assert abs(got[2][0] - got[2][2]) <= 2 * (tol['stats'][0] + tol['stats'][2])      # log_z = log_z_prior
  out = pev.prior_votes(None, prior, grid, 36, device=DEV)
  assert guarded.same_bits(out['votes'], torch.from_numpy(got[0]).to(DEV))
  index = ops.vote_peaks(out['votes'], 1)[0].cpu().numpy()[0]
  assert index.tolist() == [7] + prior.centres[0, 7].tolist()


def test_flat_prior_agrees_with_vote_posterior():
  """A flat prior (huge covariance, kappa = 0) has u = c on every cell, so log_z = log_z_votes + c and log_z_prior_F =
  c + log |F|: log_z - log_z_prior_F + log |F| is ``ops.vote_posterior``'s log_z, within the two bounds summed (the
  term log |F|, the number of contributing cells, is exact: the prior's sum over F counts cells, the votes' does not)."""
  shape = (36, 31, 33)
  v = ref.random_votes(shape, 21)
  tab = ref.table(shape, 0.25, [3.0, 3.0], np.eye(2) * 1e12, heading=0.0, concentration=0.0)
  got = _run(v, tab, 0.7)
  tol = ref.bound(v, tab, 0.7)
  post = ops.vote_posterior(torch.from_numpy(v).to(DEV), 0.7)[2].cpu().numpy().astype(np.float64)
  ptol = pref.bound(v, np.float32(0.7), None)[2]
  err = abs((got[2][0] - got[2][3] + np.log(float(got[3][0]))) - post[0])
  allowed = tol['stats'][0] + tol['stats'][3] + ptol[0]
  print(f'flat prior: |difference| {err:.3e}, sum of the bounds {allowed:.3e}')
  assert err <= allowed
  assert abs(got[2][1] - post[0]) <= tol['stats'][1] + ptol[0]


def test_two_priors_in_turn_equal_their_product():
  shape = (4, 15, 13)
  p1, c1 = np.array([1.0, 1.2]), np.array([[0.2, 0.05], [0.05, 0.3]])
  p2, c2 = np.array([1.4, 0.9]), np.array([[0.4, -0.1], [-0.1, 0.25]])
  c12 = np.linalg.inv(np.linalg.inv(c1) + np.linalg.inv(c2))
  p12 = c12 @ (np.linalg.inv(c1) @ p1 + np.linalg.inv(c2) @ p2)
  sq = np.array([0.3, 1.9])
  v = ref.random_votes(shape, 5)
  t1, t2, t12 = (ref.table(shape, 0.25, p, c, sensor_q=sq) for p, c in ((p1, c1), (p2, c2), (p12, c12)))
  first = _run(v, t1, 1.3)
  second = _run(first[0], t2, 1.0)
  both = _run(v, t12, 1.3)
  fin = np.isfinite(both[0])
  assert (fin == np.isfinite(second[0])).all()
  # the three calls' bounds, plus what the f32 rounding of the three tables' precisions and offsets moves the quadratic by
  _, q1 = ref._cells(t1)
  _, q2 = ref._cells(t2)
  _, q12 = ref._cells(t12)
  table_rounding = 2.0 ** -23 * (q1 + q2 + q12)[0] + 1e-5
  allowed = (ref.bound(v, t1, 1.3)['out'] + ref.bound(first[0], t2, 1.0)['out'] + ref.bound(v, t12, 1.3)['out']
             + 2 * table_rounding.max())
  with np.errstate(invalid='ignore'):
    err = np.abs(second[0].astype(np.float64) - both[0])[fin]
  print(f'two priors in turn: largest difference {err.max():.3e}, allowed {allowed[fin].min():.3e} ..')
  assert (err <= allowed[fin]).all()


def test_masked_nan_and_inf_cells():
  shape = (4, 7, 7)
  tab = ref.random_table(shape, 3, 31)
  v = ref.random_votes(shape, 32)
  masked = v.copy()
  bad = v.copy()
  for i, c in enumerate(((0, 3, 3), (1, 6, 6), (3, 2, 5))):
    masked[c] = -np.inf
    bad[c] = np.nan if i % 2 == 0 else np.inf
  g_bad, g_masked = _run(bad, tab), _run(masked, tab)
  assert g_bad[3].tolist() == [g_masked[3][0], 3, g_masked[3][2], 0] and g_masked[3][1] == 0
  for a, b in zip(g_bad[:3], g_masked[:3]):                  # the rest is unchanged, bit for bit
    assert guarded.same_bits(torch.from_numpy(a), torch.from_numpy(b))
  assert (g_bad[0][np.isneginf(masked)] == -np.inf).all()
  _assert_within(g_bad, ref.vote_prior(bad, tab), ref.bound(bad, tab), what='nan_inf')
  for shp in ((36, 31, 33), (3, 1, 1)):
    t = ref.random_table(shp, 3, 33)
    out, resp, stats, count = _run(np.full(shp, -np.inf, np.float32), t)
    want = ref.vote_prior(np.full(shp, -np.inf, np.float32), t)
    assert (out == -np.inf).all() and np.isnan(resp).all() and count.tolist() == [0, 0, 0, 0]
    assert stats[0] == -np.inf and stats[1] == -np.inf and stats[3] == -np.inf and np.isnan(stats[4])
    assert abs(stats[2] - want['stats'][2]) <= 2 * ref.bound(None, t)['stats'][2]


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for shape, M in (((36, 31, 33), 8), ((64, 5, 300), 3), (ref.FOLD_SHAPE, 1)):
    tab = ref.random_table(shape, M, 41)
    prior = _prior(tab)
    votes = torch.from_numpy(ref.random_votes(shape, 42)).to(DEV)
    first = ops.prior_volume(votes, prior, 0.9)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.prior_volume(votes, prior, 0.9)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), shape
    R, Ho, Wo = shape
    dev = [torch.from_numpy(tab[k]).to(DEV) for k in ('centres', 'planes', 'comps')]
    nbytes = lib.snap_vote_prior_workspace_bytes(R, Ho, Wo, M)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    for fill in (0x7ff8000000000001, -1):
      ws.fill_(fill)
      o = (torch.empty(shape, dtype=torch.float32, device=DEV), torch.empty((M,), dtype=torch.float64, device=DEV),
           torch.empty((8,), dtype=torch.float64, device=DEV), torch.empty((4,), dtype=torch.int32, device=DEV))
      st = lib.snap_vote_prior_f32(
          ctypes.c_void_p(votes.data_ptr()), R, Ho, Wo, 0.9, M, *(ctypes.c_void_p(t.data_ptr()) for t in dev),
          *(ctypes.c_void_p(t.data_ptr()) for t in o), ctypes.c_void_p(ws.data_ptr()), nbytes,
          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      torch.cuda.synchronize()
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), shape


def test_a_repeated_prior_uploads_nothing():
  tab = ref.random_table((4, 7, 7), 3, 51)
  prior = _prior(tab)
  votes = torch.from_numpy(ref.random_votes((4, 7, 7), 52)).to(DEV)
  ops.prior_volume(votes, prior)
  blobs = dict(prior._device_consts)
  ops.prior_volume(votes, prior)
  assert len(blobs) == 1 and all(prior._device_consts[k] is t for k, t in blobs.items())


# ---- the host entry points -----------------------------------------------------------------------------------------------
GRID = grids.Grid2D((5, 6), 0.25)                             # votes [8, 9, 11]
R8 = 8


def _gps():
  return pev.pose_prior(GRID, R8, position=[[0.7, 0.9], [0.4, 0.3]], covariance=[np.eye(2) * 0.1, np.eye(2) * 0.2],
                        heading=[0.4, 0.1], concentration=[4.0, 1.0], sensor_q=[0.2, 1.0])


def test_prior_votes_names_and_ground_truth():
  v = ref.random_votes((R8, 9, 11), 61)
  votes = torch.from_numpy(v).to(DEV)
  prior = _gps()
  gt = geometry.Transform2D(torch.tensor(-2 * np.pi * 3 / R8), torch.tensor([0.66, 0.8]))
  out = pev.prior_votes(votes, prior, GRID, R8, temperature=0.8, m_t_q_gt=gt)
  s = out['stats'].cpu().numpy()
  assert float(out['log_evidence']) == s[0] - s[2] and float(out['log_overlap']) == (s[0] - s[2]) - s[1]
  assert float(out['information_gain']) == (s[4] - s[0]) + s[1]
  assert float(out['log_overlap']) <= 0 <= float(out['information_gain'])
  assert out['responsibility'].dtype == torch.float64 and tuple(out['responsibility'].shape) == (2,)
  idx = pev.exhaustive_tfm_to_index(gt, GRID, R8).numpy()
  k, a, b = (int(np.rint(x)) for x in idx)
  want = float(prior.log_prior(k % R8, a, b)) - s[2]
  assert abs(float(out['log_prior_gt']) - want) < 1e-12


def test_filter_apply_prior():
  v = ref.random_votes((R8, 9, 11), 71)
  votes = torch.from_numpy(v).to(DEV)
  prior = _gps()
  flt = pev.VoteFilter(GRID, R8, 0.1, 0.05, temperature=0.8, keep_history=True)
  with pytest.raises(ValueError, match=r'VoteFilter.apply_prior: no belief \(at least one step\)'):
    flt.apply_prior(prior)
  step = flt.step(votes)
  belief = step['belief'].cpu().numpy()
  got = flt.apply_prior(prior)
  assert flt.belief is got['votes'] and flt.history[-1][0] is got['votes'] and flt.history[-1][1] is None
  direct = pev.prior_votes(votes, prior, GRID, R8, temperature=0.8)
  tab = dict(shape=prior.shape, weights=prior.weights, mu=prior.mu, centres=prior.centres, planes=prior.planes,
             comps=prior.comps)
  # the first step's belief is softmax(0.8 votes) rounded to f32: its own rounding enters beside the two bounds
  allowed = (ref.bound(belief, tab, 1.0)['out'] + ref.bound(v, tab, 0.8)['out']
             + 2.0 ** -23 * (np.abs(np.where(np.isfinite(belief), belief, 0)) + 1) + 1e-5)
  a, b = got['votes'].cpu().numpy().astype(np.float64), direct['votes'].cpu().numpy().astype(np.float64)
  fin = np.isfinite(b)
  with np.errstate(invalid='ignore'):
    assert (np.isfinite(a) == fin).all() and (np.abs(a - b)[fin] <= allowed[fin]).all()
  flt.step(votes, geometry.Transform2D(torch.zeros(()), torch.tensor([0.1, 0.0])))
  inc = flt.history[-1][1]
  new = flt.apply_prior(prior)
  assert flt.history[-1][0] is new['votes'] and flt.history[-1][1] is inc and len(flt.history) == 2
  frames = flt.smooth()
  assert len(frames) == 2 and frames[-1]['votes'] is new['votes']


def test_localize_exhaustive_with_and_without_a_prior():
  H, D = 8, 8
  rng = np.random.default_rng(9)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  plane_q = types.FeaturePlane(features=torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV), valid=valid)
  plane_map = types.FeaturePlane(features=torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV),
                                 valid=valid)
  prior = pev.pose_prior(grid, R8, position=[1.1, 0.8], covariance=np.eye(2) * 0.1, heading=0.4, concentration=4.0)
  plain = pev.localize_exhaustive(plane_q, plane_map, R8, grid)
  none = pev.localize_exhaustive(plane_q, plane_map, R8, grid, prior=None)
  assert sorted(plain) == sorted(none) and 'votes_frame' not in none and 'prior' not in none
  for key in ('votes', 'index', 'score', 'count'):
    assert guarded.same_bits(plain[key], none[key]), key
  with_prior = pev.localize_exhaustive(plane_q, plane_map, R8, grid, prior=prior)
  assert tuple(with_prior['votes'].shape) == (R8, 15, 15)
  assert guarded.same_bits(with_prior['votes_frame'], plain['votes'])
  assert with_prior['votes'] is with_prior['prior']['votes']
  lse = torch.logsumexp(with_prior['votes'].double().reshape(-1), 0)
  assert abs(float(lse)) < 1e-4


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_status_codes_without_a_launch():
  lib = _lib.load()
  R, Ho, Wo, M = 4, 7, 7, 3
  tab = ref.random_table((R, Ho, Wo), M, 81)
  dev = [torch.from_numpy(tab[k]).to(DEV) for k in ('centres', 'planes', 'comps')]
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  nbytes = lib.snap_vote_prior_workspace_bytes(R, Ho, Wo, M)
  assert nbytes > 0
  assert [lib.snap_vote_prior_workspace_bytes(*a) for a in ((R, Ho, Wo, 0), (R, Ho, Wo, 9), (65, Ho, Wo, M),
                                                            (R, 0, Wo, M), (64, 8192, 8192, 1))] == [0] * 5
  ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
  o = (torch.full((R, Ho, Wo), 7.0, device=DEV), torch.full((M,), 7.0, dtype=torch.float64, device=DEV),
       torch.full((8,), 7.0, dtype=torch.float64, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV))
  p = lambda t: ctypes.c_void_p(t.data_ptr())

  def call(votes_p=p(votes), shape=(R, Ho, Wo), scale=1.0, m=M, out_p=p(o[0]), ws_p=p(ws), ws_bytes=nbytes):
    return lib.snap_vote_prior_f32(votes_p, *shape, scale, m, *(p(t) for t in dev), out_p, p(o[1]), p(o[2]), p(o[3]),
                                   ws_p, ws_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert call(out_p=None) == _lib.SNAP_ERR_NULL
  assert call(m=0) == _lib.SNAP_ERR_BAD_SHAPE and call(m=9) == _lib.SNAP_ERR_BAD_SHAPE
  assert call(shape=(65, Ho, Wo)) == _lib.SNAP_ERR_BAD_SHAPE
  assert call(ws_bytes=nbytes - 8) == _lib.SNAP_ERR_WORKSPACE
  assert call(ws_p=ctypes.c_void_p(ws.data_ptr() + 4)) == _lib.SNAP_ERR_WORKSPACE
  for scale in (float('inf'), float('nan'), 0.0, -1.0):
    assert call(scale=scale) == _lib.SNAP_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in o), 'a refused call wrote nothing'
  assert call() == 0 and call(votes_p=None, scale=float('nan')) == 0      # (without votes the scale is ignored)
  torch.cuda.synchronize()


def _good():
  tab = ref.random_table((3, 4, 5), 2, 91)
  return dict(votes=torch.zeros((3, 4, 5), dtype=torch.float32, device=DEV), table=_prior(tab), scale=1.0)


class _Table:
  def __init__(self, **kw):
    self.__dict__.update(kw)


def _broken(**change):
  t = _good()['table']
  kw = dict(shape=t.shape, centres=t.centres, planes=t.planes, comps=t.comps)
  kw.update(change)
  return _Table(**kw)


BAD_CALLS = [
    ('votes-f64', 'votes', lambda: torch.zeros((3, 4, 5), dtype=torch.float64, device=DEV)),
    ('votes-nontensor', 'votes', lambda: np.zeros((3, 4, 5), np.float32)),
    ('votes-cpu', 'votes', lambda: torch.zeros((3, 4, 5), dtype=torch.float32)),
    ('votes-2d', 'votes', lambda: torch.zeros((4, 5), dtype=torch.float32, device=DEV)),
    ('votes-other-shape', 'votes', lambda: torch.zeros((3, 4, 6), dtype=torch.float32, device=DEV)),
    ('votes-noncontig', 'votes', lambda: torch.zeros((3, 4, 10), dtype=torch.float32, device=DEV)[..., ::2]),
    ('scale-0', 'scale', lambda: 0.0),
    ('scale-negative', 'scale', lambda: -1.0),
    ('scale-inf', 'scale', lambda: float('inf')),
    ('scale-nan', 'scale', lambda: float('nan')),
    ('scale-inf-as-f32', 'scale', lambda: 1e39),
    ('table-none', 'table', lambda: None),
    ('table-tuple', 'table', lambda: (1, 2, 3)),
    ('table-centres-f32', 'table', lambda: _broken(centres=_good()['table'].centres.astype(np.float32))),
    ('table-planes-f64', 'table', lambda: _broken(planes=_good()['table'].planes.astype(np.float64))),
    ('table-comps-short', 'table', lambda: _broken(comps=_good()['table'].comps[:, :3])),
    ('table-other-R', 'table', lambda: _broken(shape=(4, 4, 5))),
    ('table-9-components', 'table', lambda: _prior(ref.random_table((3, 4, 5), 9, 92))),
]


@pytest.mark.parametrize('arg,value', [row[1:] for row in BAD_CALLS], ids=[row[0] for row in BAD_CALLS])
def test_bad_call_is_refused(arg, value):
  """A call that is good but for ONE argument: ValueError (``_vote_volume_arg``'s rule), the operator's name in front,
  and nothing allocated before the refusal."""
  a = _good()
  a[arg] = value()
  with guarded.scope() as sc:
    with pytest.raises(ValueError) as info:
      ops.prior_volume(a['votes'], a['table'], a['scale'])
    print(f'{type(info.value).__name__}: {info.value}')
    assert type(info.value) is ValueError
    assert str(info.value).startswith('vote_prior:'), str(info.value)
    assert not sc.allocations(), 'a refused call allocated nothing'
  g = _good()
  assert ops.prior_volume(g['votes'], g['table'], g['scale']) is not None


def test_the_shares_of_the_bound():
  """Prints the worst share over the cases that ran before it in this module (a record; alone it has nothing to
  print)."""
  worst = {}
  for what, shares in SHARES.items():
    for k, v in shares.items():
      if v > worst.get(k, (0, ''))[0]:
        worst[k] = (v, what)
  print('largest observed share of the bound:', {k: (round(v, 4), w) for k, (v, w) in worst.items()})
  assert all(v <= 2.0 for v, _ in worst.values())
