"""`-m gpu`: ``ops.raster_volume`` (vote_raster.hip, through the C ABI) and the host entry points built on it
(``raster_votes``, ``VoteFilter.apply_raster_prior``, ``localize_exhaustive(raster=...)``, ``RasterStrengthFit``),
against the float64 numpy restatement ``vote_raster_reference`` within twice its documented error bound (a function of
the input: the reference module's docstring); the -inf pattern and the counts exactly.

Launches 1 and 2 tile the pixels p = a * Wo + b into runs of 256, one workgroup each (up to 1024 workgroups, then
several tiles per workgroup), one kernel instance per ladder length S.  ``[1, 5, 5]`` and ``[3, 1, 1]``: the smallest
extents; ``[4, 7, 7]``: one partial tile; ``[36, 31, 33]``: four tiles, a ragged last one, Ho != Wo; ``[64, 5, 300]``:
the largest R; ``[2, 520, 520]``: 1057 tiles on 1024 workgroups (the float64 accumulators carry over a second tile); S in
{1, 3, 8} with the written level first and last; h in {1, 2}; one, two and four taps; rasters that cover the lattice and
that it leaves on every side, with invalid patches; ``outside`` finite and -inf.  Every call runs under
``guarded.scope()``: guard regions intact (outputs and workspace), the workspace as large as the query says, no output
element left unwritten.

Observed on an MI355X (each test prints its figures; ``test_the_shares_of_the_bound`` the worst of the module): the
bound is a worst-case sum over the rounding points, and the largest observed share of it is 0.41 on ``out`` (one tap,
``[36, 31, 33]``), 0.27 on log_z, 0.14 on log_z_prior, 0.22 on E[g], 0.33 on Var[g], 0.22 on log_z_votes, 0.61 on the
ground-truth cell's fl32(scale v) and 0.15 on its g (2 allowed); the flat raster differs from ``ops.vote_posterior``'s
log_z by 1.2e-7 where the bounds sum to 8.2e-6; two rasters in turn differ from their sum by 1.5e-5 (4.8e-5 allowed)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_posterior_reference as pref
import vote_raster_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
SHARES = {}


def _prior(tab):
  return pev.RasterPrior(tab['shape'], tab['raster'], tab['offset'], tab['offsets'], tab['planes'], tab['outside'],
                         tab['strengths'], tab['harmonic'])


def _run(v, tab, scale=1.0, write=0, gt=-1, prior=None):
  """One guarded call -> numpy (out, table, stats, count)."""
  prior = prior or _prior(tab)
  R, Ho, Wo = tab['shape']
  X, Y = tab['raster'].shape[:2]
  S = tab['strengths'].size
  votes = None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
  with guarded.scope() as sc:
    out = ops.raster_volume(None if votes is None else guarded.place(votes, 'value'), prior, scale, write=write,
                            gt_index=gt, device=DEV)
    assert [tuple(o.shape) for o in out] == [(R, Ho, Wo), (S, 4), (4,), (4,)]
    assert [o.dtype for o in out] == [torch.float32, torch.float64, torch.float64, torch.int32]
    ws = [a for a in sc.allocations('raster_volume') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_raster_workspace_bytes(R, Ho, Wo, X, Y, S)
    for o, what in zip(out, ('out', 'table', 'stats', 'count')):
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  assert res[2][3] == 0
  return res


def _share(err, tol):
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(err == 0, 0.0, np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.inf))


def _close(g, x, b, factor, what, shares, name):
  """One float64 figure: NaN with NaN, an infinity exactly, else within ``factor`` times the bound."""
  if not np.isfinite(x) or b == np.inf:
    assert b == np.inf or (np.isnan(g) and np.isnan(x)) or g == x, f'{what}: {name} {g} vs {x}'
    return
  shares[name] = max(shares.get(name, 0.0), float(_share(np.abs(g - x), np.float64(b))))
  assert abs(g - x) <= factor * b, f'{what}: {name} {g!r} vs {x!r}, bound {b:.3e}'


def _assert_within(got, want, tol, factor=2.0, what=''):
  out, table, stats, count = got
  assert count[:3].tolist() == want['count'], f'{what}: count {count.tolist()} != {want["count"]}'
  assert want['zero_lo'] <= count[3] <= want['zero_hi'], (what, count[3], want['zero_lo'], want['zero_hi'])
  w = want['out']
  assert ((out == -np.inf) == (w == -np.inf)).all() and not np.isnan(out).any(), f'{what}: -inf pattern'
  fin = np.isfinite(w)
  shares = {}
  e = np.abs(out.astype(np.float64)[fin] - w[fin])
  shares['out'] = float(_share(e, tol['out'][fin]).max()) if fin.any() else 0.0
  assert (e <= factor * tol['out'][fin]).all(), f'{what}: out, {int((e > factor * tol["out"][fin]).sum())} cells outside'
  for s in range(table.shape[0]):
    for i, name in enumerate(ref.COLUMNS):
      _close(table[s, i], want['table'][s, i], tol['table'][s, i], factor, f'{what}[{s}]', shares, name)
  for i, name in enumerate(('log_z_votes', 'x_gt', 'g_gt')):
    _close(stats[i], want['stats'][i], tol['stats'][i], factor, what, shares, name)
  SHARES[what] = shares
  print(f'{what}: largest share of the bound', {k: round(v, 4) for k, v in shares.items()})


def _check(v, tab, scale, what, write=0, gt=-1):
  got = _run(v, tab, scale, write, gt)
  _assert_within(got, ref.vote_raster(v, tab, scale, write, gt), ref.bound(v, tab, scale, write, gt), what=what)
  return got


def _gt_cases(v, tab):
  """A ground-truth index inside F, one on a cell the raster excludes (where there is one), and -1."""
  g = ref.log_prior(tab)[0].reshape(-1)
  fin = np.isfinite(v.reshape(-1)) if v is not None else np.ones(g.size, bool)
  inside = np.flatnonzero(fin & (g > -np.inf) & (g != tab['outside']))
  cut = np.flatnonzero(fin & (g == tab['outside']))
  return [int(c[c.size // 2]) for c in (inside, cut) if c.size] + [-1]


OPTIONS = list(itertools.product((1, 2), (1, 2, 4), ('covers', 'cut'), (-np.inf, -2.5)))   # h, taps, cover, outside


@pytest.mark.parametrize('S', (1, 3, 8))
@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_random_shapes(shape, S):
  """Random votes with -inf patches on every lattice and ladder length; the options (harmonic, taps, cover, outside)
  cycle with the case, two of them per case, the written level first and last, every kind of ground-truth index."""
  seed = sum(shape) + S
  v = ref.random_votes(shape, seed)
  for i, write in enumerate((0, S - 1)):
    h, taps, cover, outside = OPTIONS[(5 * seed + 7 * i) % len(OPTIONS)]
    tab = ref.synthetic(shape, seed + i, S, h, taps, cover, outside)
    for gt in _gt_cases(v, tab)[i::2] or [-1]:
      _check(v, tab, 0.7, f'random{shape}_S{S}_h{h}_t{taps}_{cover}_{outside}_w{write}_gt{gt}', write, gt)


@pytest.mark.parametrize('h,taps,cover,outside', OPTIONS,
                         ids=['h%d-taps%d-%s-%s' % (o[0], o[1], o[2], 'inf' if o[3] == -np.inf else 'finite')
                              for o in OPTIONS])
def test_every_option(h, taps, cover, outside):
  """Every combination of harmonic, taps, cover and outside on [36, 31, 33] (several tiles) with S = 3, and without
  votes on [4, 7, 7]."""
  shape = (36, 31, 33)
  v = ref.random_votes(shape, 3)
  tab = ref.synthetic(shape, 11 + taps, 3, h, taps, cover, outside)
  for write, gt in zip((0, 2, 1), _gt_cases(v, tab)):
    _check(v, tab, 1.3, f'option_h{h}_t{taps}_{cover}_{outside}_w{write}_gt{gt}', write, gt)
  small = ref.synthetic((4, 7, 7), 17 + taps, 8, h, taps, cover, outside)
  got = _check(None, small, 1.0, f'no_votes_h{h}_t{taps}_{cover}_{outside}', 7, _gt_cases(None, small)[0])
  assert got[3][0] == 4 * 7 * 7 and got[3][1] == 0


def test_several_tiles_per_workgroup():
  v = ref.fold_votes()
  assert v.shape[1] * v.shape[2] > ref.MAX_GROUPS * ref.TILE
  for S, taps, cover in ((1, 1, 'covers'), (8, 4, 'cut')):
    tab = ref.synthetic(ref.FOLD_SHAPE, 5 + S, S, 1, taps, cover, -np.inf, kappa=2.0)
    _check(v, tab, 1.0, f'fold_S{S}', S - 1, _gt_cases(v, tab)[0])


def test_without_votes_the_raster_prior_is_a_belief():
  """votes=None through ``raster_prior`` / ``raster_votes``: logsumexp(out) = 0 within the bound, log_z = log_z_prior,
  and the information gain against flat votes is log(cells) - the entropy >= 0."""
  grid = grids.Grid2D((16, 17), 0.25)
  A, ok, phi, kap = ref.random_raster(16, 17, 21)
  prior = pev.raster_prior(grid, 36, log_area=A, valid=ok, heading=phi, concentration=kap, sensor_q=(2.3, 1.7),
                           strengths=ref.LADDERS[3])
  tab = dict(shape=prior.shape, raster=prior.raster, offset=prior.offset, offsets=prior.offsets, planes=prior.planes,
             outside=prior.outside, strengths=prior.strengths, harmonic=1)
  got = _run(None, tab, write=1, prior=prior)
  want, tol = ref.vote_raster(None, tab, write=1), ref.bound(None, tab, write=1)
  _assert_within(got, want, tol, what='no_votes')
  assert 0 < got[3][2] < 36 * 31 * 33 and got[3][0] == 36 * 31 * 33
  fin = np.isfinite(got[0])
  assert abs(ref._lse(got[0][fin].astype(np.float64))) <= 2 * (tol['table'][1, 0] + ref.EPS * np.abs(want['out'][fin]).max())
  for s in range(3):
    assert abs(got[1][s, 0] - got[1][s, 1]) <= 2 * (tol['table'][s, 0] + tol['table'][s, 1])
  out = pev.raster_votes(None, prior, grid, 36, strength=1, device=DEV)
  assert guarded.same_bits(out['votes'], torch.from_numpy(got[0]).to(DEV))
  assert tuple(out['information_gain'].shape) == (3,) and bool((out['information_gain'] >= 0).all())


def test_flat_raster_agrees_with_vote_posterior():
  """A = 0, kappa = 0 on a raster that covers the lattice: log_z_s and log_z_votes are ``ops.vote_posterior``'s log_z,
  within the two bounds summed; E[g] = 0 and Var[g] = 0 exactly."""
  shape = (36, 31, 33)
  v = ref.random_votes(shape, 21)
  tab = ref.synthetic(shape, 22, 3, 1, 4, 'covers', -np.inf, invalid=False, kappa=0.0)
  tab['raster'][..., 0] = 0
  got = _run(v, tab, 0.7)
  tol = ref.bound(v, tab, 0.7)
  post = ops.vote_posterior(torch.from_numpy(v).to(DEV), 0.7)[2].cpu().numpy().astype(np.float64)
  ptol = pref.bound(v, np.float32(0.7), None)[2]
  for s in range(3):
    err = abs(got[1][s, 0] - post[0])
    print(f'flat raster[{s}]: |difference| {err:.3e}, sum of the bounds {tol["table"][s, 0] + ptol[0]:.3e}')
    assert err <= tol['table'][s, 0] + ptol[0]
    assert got[1][s, 2] == 0 and got[1][s, 3] == 0
  assert abs(got[2][0] - post[0]) <= tol['stats'][0] + ptol[0]


def test_two_rasters_in_turn_equal_their_sum():
  """Same offsets and weights, so the interpolation is linear in the planes: two calls equal one with the summed
  raster, within the three calls' bounds plus the f32 rounding of the summed planes."""
  shape = (4, 15, 13)
  v = ref.random_votes(shape, 5)
  t1 = ref.synthetic(shape, 31, 1, 1, 4, 'cut', -np.inf)
  A2, _, phi2, kap2 = ref.random_raster(*t1['raster'].shape[:2], 33, invalid=False)
  t2 = dict(t1, raster=ref.table(shape, 0.25, A2, t1['raster'][..., 3] != 0, phi2, kap2)['raster'])
  t12 = dict(t1, raster=t1['raster'].copy())
  t12['raster'][..., :3] = t1['raster'][..., :3] + t2['raster'][..., :3]
  first = _run(v, t1, 1.3)
  second = _run(first[0], t2, 1.0)
  both = _run(v, t12, 1.3)
  fin = np.isfinite(both[0])
  assert (fin == np.isfinite(second[0])).all() and fin.any()
  rounding = 2.0 ** -23 * ref.log_prior(t12)[1] + 1e-6
  allowed = (ref.bound(v, t1, 1.3)['out'] + ref.bound(first[0], t2, 1.0)['out'] + ref.bound(v, t12, 1.3)['out']
             + rounding + 2.0 ** -23 * np.abs(np.where(np.isfinite(first[0]), first[0], 0)))
  with np.errstate(invalid='ignore'):
    err = np.abs(second[0].astype(np.float64) - both[0])
  print(f'two rasters in turn: largest difference {err[fin].max():.3e}, allowed {allowed[fin].min():.3e} ..')
  assert (err[fin] <= allowed[fin]).all()


def test_masked_nan_and_inf_cells():
  shape = (4, 7, 7)
  tab = ref.synthetic(shape, 41, 3, 2, 4, 'covers', -1.0)
  v = ref.random_votes(shape, 32)
  masked, bad = v.copy(), v.copy()
  for i, c in enumerate(((0, 3, 3), (1, 6, 6), (3, 2, 5))):
    masked[c] = -np.inf
    bad[c] = np.nan if i % 2 == 0 else np.inf
  g_bad, g_masked = _run(bad, tab, write=2), _run(masked, tab, write=2)
  assert g_bad[3].tolist() == [g_masked[3][0], 3, g_masked[3][2], g_masked[3][3]] and g_masked[3][1] == 0
  for a, b in zip(g_bad[:3], g_masked[:3]):                  # the rest is unchanged, bit for bit
    assert guarded.same_bits(torch.from_numpy(a), torch.from_numpy(b))
  _assert_within(g_bad, ref.vote_raster(bad, tab, write=2), ref.bound(bad, tab, write=2), what='nan_inf')
  gt = 5
  bad.reshape(-1)[gt] = np.nan
  assert np.isnan(_run(bad, tab, gt=gt)[2][1])
  for shp in ((36, 31, 33), (3, 1, 1)):
    t = ref.synthetic(shp, 43, 3, 1, 4, 'covers', -np.inf)
    out, table, stats, count = _run(np.full(shp, -np.inf, np.float32), t)
    want = ref.vote_raster(None, t)
    assert (out == -np.inf).all() and count.tolist() == [0, 0, 0, 0] and stats[0] == -np.inf
    assert (table[:, 0] == -np.inf).all() and np.isnan(table[:, 2:]).all()
    assert (np.abs(table[:, 1] - want['table'][:, 1]) <= 2 * ref.bound(None, t)['table'][:, 1]).all()


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for shape, S in (((36, 31, 33), 8), ((64, 5, 300), 3), (ref.FOLD_SHAPE, 1)):
    tab = ref.synthetic(shape, 51, S, 1, 4, 'cut', -np.inf)
    prior = _prior(tab)
    votes = torch.from_numpy(ref.random_votes(shape, 42)).to(DEV)
    first = ops.raster_volume(votes, prior, 0.9, write=S - 1, gt_index=7)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.raster_volume(votes, prior, 0.9, write=S - 1, gt_index=7)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), shape
    R, Ho, Wo = shape
    X, Y = tab['raster'].shape[:2]
    dev = [torch.from_numpy(tab[k]).to(DEV) for k in ('raster', 'offsets', 'planes')]
    lam = (ctypes.c_float * S)(*tab['strengths'].tolist())
    nbytes = lib.snap_vote_raster_workspace_bytes(R, Ho, Wo, X, Y, S)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    for fill in (0x7ff8000000000001, -1):
      ws.fill_(fill)
      o = (torch.empty(shape, dtype=torch.float32, device=DEV), torch.empty((S, 4), dtype=torch.float64, device=DEV),
           torch.empty((4,), dtype=torch.float64, device=DEV), torch.empty((4,), dtype=torch.int32, device=DEV))
      p = lambda t: ctypes.c_void_p(t.data_ptr())
      st = lib.snap_vote_raster_f32(p(votes), R, Ho, Wo, 0.9, p(dev[0]), X, Y, p(dev[1]), p(dev[2]), tab['outside'],
                                    lam, S, S - 1, 7, *(p(t) for t in o), p(ws), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      torch.cuda.synchronize()
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), shape


def test_a_repeated_raster_uploads_nothing():
  tab = ref.synthetic((4, 7, 7), 61, 3, 1, 4, 'cut')
  prior = _prior(tab)
  votes = torch.from_numpy(ref.random_votes((4, 7, 7), 52)).to(DEV)
  ops.raster_volume(votes, prior)
  blobs = dict(prior._device_consts)
  ops.raster_volume(votes, prior)
  assert len(blobs) == 1 and all(prior._device_consts[k] is t for k, t in blobs.items())


# ---- the host entry points -----------------------------------------------------------------------------------------------
R8 = 8
H, D = 8, 8
GRID = grids.Grid2D((H, H), 0.25)                             # votes [8, 15, 15]


def _real_votes(seed):
  rng = np.random.default_rng(seed)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  planes = [types.FeaturePlane(features=torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV),
                               valid=valid) for _ in range(2)]
  return planes[0], planes[1]


def _pose_of(k, a, b):
  """The pose of a lattice index as one Transform2D (host)."""
  tfm = pev.exhaustive_indices_to_tfm(torch.tensor([[k, a, b]]), GRID, R8)
  return geometry.Transform2D(tfm.angle[0], tfm.t[0])


def _lanes(strengths=(1.0,), **kw):
  A, ok, phi, kap = ref.random_raster(H, H, 71)
  return pev.raster_prior(GRID, R8, log_area=A, valid=ok, heading=phi, concentration=kap, outside=-6.0,
                          strengths=strengths, **kw)


def test_raster_votes_names_and_ground_truth():
  plane_q, plane_map = _real_votes(9)
  votes = pev.exhaustive_pose_voting(plane_q, plane_map, R8, GRID)
  prior = _lanes(ref.LADDERS[3], sensor_q=(0.7, 1.2))
  gt = _pose_of(3, 9, 4)
  out = pev.raster_votes(votes, prior, GRID, R8, temperature=0.8, strength=2, m_t_q_gt=gt)
  t, s, lam = out['table'].cpu().numpy(), out['stats'].cpu().numpy(), prior.strengths
  for name in ('log_z', 'log_z_prior', 'expected_log_prior', 'variance_log_prior', 'log_evidence', 'log_overlap',
               'information_gain', 'log_prob_gt', 'log_prob_gt_slope'):
    assert out[name].dtype == torch.float64 and tuple(out[name].shape) == (3,), name
  assert out['log_z_votes'].dtype == torch.float64 and out['log_z_votes'].dim() == 0
  assert np.array_equal(out['log_evidence'].cpu().numpy(), t[:, 0] - t[:, 1])
  assert np.array_equal(out['information_gain'].cpu().numpy(), (lam * t[:, 2] - t[:, 0]) + s[0])
  assert bool((out['log_overlap'] <= 0).all()) and bool((out['information_gain'] >= 0).all())
  idx = pev.exhaustive_tfm_to_index(gt, GRID, R8).numpy()
  k, a, b = (int(np.rint(x)) for x in idx)
  v = votes.cpu().numpy()
  assert (k % R8, a, b) == (3, 9, 4) and abs(s[2] - float(prior.log_prior(k % R8, a, b))) < 1e-4
  assert s[1] == float(np.float32(0.8) * v[k % R8, a, b])
  assert np.array_equal(out['log_prob_gt'].cpu().numpy(), (s[1] + lam * s[2]) - t[:, 0])
  # the written level is the normalised product, cell for cell
  tab = dict(shape=prior.shape, raster=prior.raster, offsets=prior.offsets, planes=prior.planes, outside=prior.outside,
             strengths=prior.strengths)
  want, tol = ref.vote_raster(v, tab, 0.8, 2), ref.bound(v, tab, 0.8, 2)
  got = out['votes'].cpu().numpy().astype(np.float64)
  fin = np.isfinite(want['out'])
  assert (np.isfinite(got) == fin).all() and (np.abs(got[fin] - want['out'][fin]) <= 2 * tol['out'][fin]).all()
  away = pev.raster_votes(votes, prior, GRID, R8, m_t_q_gt=geometry.Transform2D(torch.tensor(0.0), torch.tensor([9.0, 9.0])))
  assert bool(torch.isnan(away['log_prob_gt']).all())


def test_filter_apply_raster_prior():
  plane_q, plane_map = _real_votes(10)
  votes = pev.exhaustive_pose_voting(plane_q, plane_map, R8, GRID)
  prior = _lanes((0.5, 1.0))
  flt = pev.VoteFilter(GRID, R8, 0.1, 0.05, temperature=0.8, keep_history=True)
  with pytest.raises(ValueError, match=r'VoteFilter.apply_raster_prior: no belief \(at least one step\)'):
    flt.apply_raster_prior(prior)
  belief = flt.step(votes)['belief']
  got = flt.apply_raster_prior(prior, strength=1)
  assert flt.belief is got['votes'] and flt.history[-1][0] is got['votes'] and flt.history[-1][1] is None
  direct = pev.raster_votes(belief, prior, GRID, R8, strength=1)
  assert guarded.same_bits(got['votes'], direct['votes'])
  assert abs(float(torch.logsumexp(got['votes'].double().reshape(-1), 0))) < 1e-4


def test_localize_exhaustive_with_and_without_a_raster():
  plane_q, plane_map = _real_votes(11)
  prior = _lanes()
  plain = pev.localize_exhaustive(plane_q, plane_map, R8, GRID)
  none = pev.localize_exhaustive(plane_q, plane_map, R8, GRID, raster=None)
  assert sorted(plain) == sorted(none) and 'votes_frame' not in none and 'raster' not in none
  for key in ('votes', 'index', 'score', 'count'):
    assert guarded.same_bits(plain[key], none[key]), key
  with_raster = pev.localize_exhaustive(plane_q, plane_map, R8, GRID, raster=dict(raster=prior, temperature=0.5))
  assert guarded.same_bits(with_raster['votes_frame'], plain['votes'])
  assert with_raster['votes'] is with_raster['raster']['votes'] and 'prior' not in with_raster
  assert abs(float(torch.logsumexp(with_raster['votes'].double().reshape(-1), 0))) < 1e-4
  gps = pev.pose_prior(GRID, R8, position=[1.1, 0.8], covariance=np.eye(2) * 0.1)
  both = pev.localize_exhaustive(plane_q, plane_map, R8, GRID, prior=gps, raster=prior)
  assert guarded.same_bits(both['votes_frame'], plain['votes']) and both['votes'] is both['raster']['votes']
  chained = pev.raster_votes(both['prior']['votes'], prior, GRID, R8)
  assert guarded.same_bits(both['votes'], chained['votes'])


def test_strength_fit_on_the_device():
  plane_q, plane_map = _real_votes(12)
  lad = (0.125, 0.5, 2.0, 8.0)
  prior = _lanes(lad)
  fit = pev.RasterStrengthFit(GRID, R8, prior, temperature=0.8)
  nll = np.zeros(4)
  frames = 0
  for seed in range(3):
    votes = pev.exhaustive_pose_voting(*_real_votes(20 + seed), R8, GRID)
    gt = _pose_of(seed, 5 + seed, 7)
    fit.add(votes, gt)
    out = pev.raster_votes(votes, prior, GRID, R8, temperature=0.8, m_t_q_gt=gt)
    lp = out['log_prob_gt'].cpu().numpy()
    if np.isfinite(lp).all():
      nll -= lp
      frames += 1
  res = fit.solve()
  assert res['frames'] == frames and frames > 0
  assert np.allclose(res['nll'], nll, rtol=0, atol=1e-9) and res['argmin'] == int(np.argmin(nll))
  assert res['bracket'][0] <= res['strength'] <= res['bracket'][1]


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_status_codes_without_a_launch():
  lib = _lib.load()
  R, Ho, Wo, S = 4, 7, 7, 3
  tab = ref.synthetic((R, Ho, Wo), 81, S)
  X, Y = tab['raster'].shape[:2]
  dev = [torch.from_numpy(tab[k]).to(DEV) for k in ('raster', 'offsets', 'planes')]
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  q = lib.snap_vote_raster_workspace_bytes
  nbytes = q(R, Ho, Wo, X, Y, S)
  assert nbytes > 0
  assert [q(*a) for a in ((R, Ho, Wo, X, Y, 0), (R, Ho, Wo, X, Y, 9), (65, Ho, Wo, X, Y, S), (0, Ho, Wo, X, Y, S),
                          (R, 0, Wo, X, Y, S), (R, Ho, Wo, 0, Y, S), (R, Ho, Wo, X, -1, S), (R, Ho, Wo, 1 << 15, 1 << 14, S),
                          (64, 8192, 8192, X, Y, 1))] == [0] * 9
  ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
  o = (torch.full((R, Ho, Wo), 7.0, device=DEV), torch.full((S, 4), 7.0, dtype=torch.float64, device=DEV),
       torch.full((4,), 7.0, dtype=torch.float64, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV))
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  good = (ctypes.c_float * S)(*tab['strengths'].tolist())

  def call(votes_p=p(votes), shape=(R, Ho, Wo), scale=1.0, raster_p=p(dev[0]), xy=(X, Y), outside=-np.inf, lam=good,
           s=S, write=0, gt=-1, out_p=p(o[0]), ws_p=p(ws), ws_bytes=nbytes):
    return lib.snap_vote_raster_f32(votes_p, *shape, scale, raster_p, *xy, p(dev[1]), p(dev[2]), outside, lam, s, write,
                                    gt, out_p, p(o[1]), p(o[2]), p(o[3]), ws_p, ws_bytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert call(out_p=None) == _lib.SNAP_ERR_NULL and call(raster_p=None) == _lib.SNAP_ERR_NULL
  assert call(lam=None) == _lib.SNAP_ERR_NULL
  assert call(s=0) == _lib.SNAP_ERR_BAD_SHAPE and call(s=9) == _lib.SNAP_ERR_BAD_SHAPE
  assert call(shape=(65, Ho, Wo)) == _lib.SNAP_ERR_BAD_SHAPE and call(xy=(0, Y)) == _lib.SNAP_ERR_BAD_SHAPE
  assert call(write=-1) == _lib.SNAP_ERR_BAD_SHAPE and call(write=S) == _lib.SNAP_ERR_BAD_SHAPE
  assert call(gt=-2) == _lib.SNAP_ERR_BAD_SHAPE and call(gt=R * Ho * Wo) == _lib.SNAP_ERR_BAD_SHAPE
  assert call(ws_bytes=nbytes - 8) == _lib.SNAP_ERR_WORKSPACE
  assert call(ws_p=ctypes.c_void_p(ws.data_ptr() + 4)) == _lib.SNAP_ERR_WORKSPACE
  assert call(raster_p=ctypes.c_void_p(dev[0].data_ptr() + 4)) == _lib.SNAP_ERR_UNSUPPORTED
  for scale in (float('inf'), float('nan'), 0.0, -1.0):
    assert call(scale=scale) == _lib.SNAP_ERR_UNSUPPORTED
  for outside in (float('inf'), float('nan')):
    assert call(outside=outside) == _lib.SNAP_ERR_UNSUPPORTED
  for lam in ((1.0, 0.0, 2.0), (1.0, -1.0, 2.0), (1.0, float('inf'), 2.0), (float('nan'), 1.0, 2.0)):
    assert call(lam=(ctypes.c_float * S)(*lam)) == _lib.SNAP_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in o), 'a refused call wrote nothing'
  assert call() == 0 and call(votes_p=None, scale=float('nan')) == 0      # (without votes the scale is ignored)
  assert call(gt=R * Ho * Wo - 1, write=S - 1, outside=-1.0) == 0
  torch.cuda.synchronize()


def _good():
  tab = ref.synthetic((3, 4, 5), 91, 3)
  return dict(votes=torch.zeros((3, 4, 5), dtype=torch.float32, device=DEV), table=_prior(tab), scale=1.0, write=0,
              gt_index=None)


class _Table:
  def __init__(self, **kw):
    self.__dict__.update(kw)


def _broken(**change):
  t = _good()['table']
  kw = dict(shape=t.shape, raster=t.raster, offsets=t.offsets, planes=t.planes, outside=t.outside, strengths=t.strengths)
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
    ('scale-nan', 'scale', lambda: float('nan')),
    ('scale-inf-as-f32', 'scale', lambda: 1e39),
    ('write-negative', 'write', lambda: -1),
    ('write-past-the-ladder', 'write', lambda: 3),
    ('gt-below', 'gt_index', lambda: -2),
    ('gt-past-the-volume', 'gt_index', lambda: 60),
    ('table-none', 'table', lambda: None),
    ('table-tuple', 'table', lambda: (1, 2, 3)),
    ('table-raster-f64', 'table', lambda: _broken(raster=_good()['table'].raster.astype(np.float64))),
    ('table-raster-3-planes', 'table', lambda: _broken(raster=_good()['table'].raster[..., :3])),
    ('table-offsets-f32', 'table', lambda: _broken(offsets=_good()['table'].offsets.astype(np.float32))),
    ('table-planes-short', 'table', lambda: _broken(planes=_good()['table'].planes[:, :3])),
    ('table-other-R', 'table', lambda: _broken(shape=(4, 4, 5))),
    ('table-outside-nan', 'table', lambda: _broken(outside=float('nan'))),
    ('table-outside-inf', 'table', lambda: _broken(outside=float('inf'))),
    ('table-strength-0', 'table', lambda: _broken(strengths=np.array([1.0, 0.0, 2.0]))),
    ('table-9-strengths', 'table', lambda: _broken(strengths=np.arange(1.0, 10.0))),
]


@pytest.mark.parametrize('arg,value', [row[1:] for row in BAD_CALLS], ids=[row[0] for row in BAD_CALLS])
def test_bad_call_is_refused(arg, value):
  """A call that is good but for ONE argument: ValueError, the operator's name in front, and nothing allocated before
  the refusal."""
  a = _good()
  a[arg] = value()
  with guarded.scope() as sc:
    with pytest.raises(ValueError) as info:
      ops.raster_volume(a['votes'], a['table'], a['scale'], a['write'], a['gt_index'])
    print(f'{type(info.value).__name__}: {info.value}')
    assert type(info.value) is ValueError
    assert str(info.value).startswith('vote_raster:'), str(info.value)
    assert not sc.allocations(), 'a refused call allocated nothing'
  g = _good()
  assert ops.raster_volume(g['votes'], g['table'], g['scale']) is not None


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
