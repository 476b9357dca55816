"""`-m gpu`: ``ops.vote_posterior`` (vote_posterior.hip, through the C ABI) and the host entry points built on it,
against the float64 numpy restatement ``vote_posterior_reference`` within twice its documented error bound (a
function of the input: the reference module's docstring).

Launch A tiles the pixels p = a * Wo + b into runs of 256, one workgroup each (up to 1024 workgroups, then several
tiles per workgroup); launch B folds the per-workgroup partial rows.  ``[4, 7, 7]``: one partial tile; ``[36, 31,
33]``: four tiles, a ragged last one, Ho != Wo; ``[1, 5, 5]`` and ``[3, 1, 1]``: the smallest extents; ``[64, 5,
300]``: the largest R, rows that span workgroups; ``[8, 200, 210]`` (the sharp peak): 165 workgroups, every chunk of
launch B's column sums in use; ``[2, 520, 520]``: 1057 tiles on 1024 workgroups, the fold of several tiles into one
workgroup's running sums.  Every call runs under ``guarded.scope()``: guard regions intact (outputs and
workspace), no output element left unwritten.

Observed on an MI355X (each test prints its figures): the exact case within 0.5 f32 ulp of the value itself on every
output (4 allowed); elsewhere the largest error is 0.51 of the bound on the marginals and 0.75 of it on a statistic (2 allowed),
e.g. ``[2, 520, 520]``: log_prob_xy 2.0e-6 against a bound of 3.9e-6, log_z 1.7e-7 against 3.5e-6."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_posterior_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c[0]: c for c in ref.all_inputs()}


@functools.lru_cache(maxsize=None)
def _want(name):
  _, v, scale, gt = _inputs()[name]
  return ref.vote_posterior(v, scale, gt), ref.bound(v, scale, gt)


def _run(v, scale, gt=None, poison_check=True):
  """One guarded call -> numpy (log_prob_xy, log_prob_r, stats, count)."""
  votes = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
  gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
  with guarded.scope() as sc:
    gtp = None if gt_dev is None else guarded.place(gt_dev, 'address')
    out = ops.vote_posterior(guarded.place(votes, 'value'), scale, gtp)
    R, Ho, Wo = v.shape
    assert [tuple(o.shape) for o in out] == [(Ho, Wo), (R,), (16,), (3,)]
    assert [o.dtype for o in out] == [torch.float32] * 3 + [torch.int32]
    ws = [a for a in sc.allocations('vote_posterior') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_posterior_workspace_bytes(R, Ho, Wo)
    if poison_check:     # (a NaN result has the poison's bits only if it is the all-ones NaN; the kernel writes 0x7fc00000)
      for o, what in zip(out, ('log_prob_xy', 'log_prob_r', 'stats', 'count')):
        assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  return res


def _assert_within(got, want, tols, factor=2.0, what=''):
  (gxy, gr, gs, gc), (wxy, wr, ws, wc), (txy, tr, ts) = got, want, tols
  assert gc.tolist() == wc.tolist(), f'{what}: count {gc.tolist()} != {wc.tolist()}'
  with np.errstate(invalid='ignore'):
    for g, w, t, nm in ((gxy, wxy, txy, 'log_prob_xy'), (gr, wr, tr, 'log_prob_r')):
      err = np.where(g == w, 0.0, np.abs(g.astype(np.float64) - w))
      bad = ~(err <= factor * t)
      print(f'{what} {nm}: max err {np.nanmax(np.where(np.isfinite(err), err, 0)):.3e}, max bound {t.max():.3e}')
      assert not bad.any(), f'{what} {nm}: {int(bad.sum())} outside, first {np.argwhere(bad)[0].tolist()}'
  R = len(wr)
  for n, nm in enumerate(ref.STAT_NAMES):
    g, w = float(gs[n]), float(ws[n])
    if np.isnan(w) or np.isinf(w):
      assert (np.isnan(g) and np.isnan(w)) or g == w, f'{what} {nm}: {g} != {w}'
      continue
    err = abs(g - w)
    if n == 9:
      err = min(err, R - err)
    print(f'{what} {nm}: got {g!r} want {w!r} err {err:.3e} bound {ts[n]:.3e}')
    assert err <= factor * ts[n], f'{what} {nm}: {g!r} vs {w!r}, err {err:.3e} > {factor} x {ts[n]:.3e}'


def _ulps(got, want, scale_floor=0.0):
  """|got - want| in f32 ulps of max(|want|, scale_floor)."""
  want = np.asarray(want, np.float64)
  unit = np.spacing(np.maximum(np.abs(want), scale_floor).astype(np.float32)).astype(np.float64)
  with np.errstate(invalid='ignore'):
    return np.where(np.asarray(got, np.float64) == want, 0.0, np.abs(np.asarray(got, np.float64) - want) / unit)


@pytest.mark.parametrize('shape', [(36, 31, 33), (4, 7, 7), (64, 5, 300)], ids=lambda s: '%dx%dx%d' % s)
def test_exact_case(shape):
  """Votes in {0, -inf}, scale 1: every exponential is 1 or 0, every sum an integer.  log_z = log n,
  log_prob_xy = log(n_ab / n), the moments ratios of integer sums: one log or division and one rounding, compared
  within 4 f32 ulp of the value itself, for every output: the kernel forms each in float64 and rounds once."""
  v = ref.exact_votes(shape)
  wxy, wr, ws, wc = ref.vote_posterior(v, 1.0)
  gxy, gr, gs, gc = _run(v, 1.0)
  n = int(np.isfinite(v).sum())
  assert gc.tolist() == wc.tolist() == [n, 0, 0]
  assert _ulps(gs[0], np.log(n)) <= 4 and gs[1] == 0 and _ulps(gs[11], np.log(n)) <= 4
  with np.errstate(divide='ignore'):
    want_xy = np.log(np.isfinite(v).sum(0) / n)
    want_r = np.log(np.isfinite(v).sum((1, 2)) / n)
  assert _ulps(gxy, want_xy).max() <= 4 and _ulps(gr, want_r).max() <= 4
  assert ((gxy == -np.inf) == (want_xy == -np.inf)).all()
  R = shape[0]
  for i in (2, 3, 4, 5, 6, 7, 8, 10):
    print(f'exact {shape} {ref.STAT_NAMES[i]}: got {float(gs[i])!r} want {ws[i]!r}: {float(_ulps(gs[i], ws[i])):.2f} ulp')
    assert _ulps(gs[i], ws[i]) <= 4, (ref.STAT_NAMES[i], gs[i], ws[i])
  d9 = abs(float(gs[9]) - ws[9])
  print(f'exact {shape} mean_r: got {float(gs[9])!r} want {ws[9]!r}')
  assert min(d9, R - d9) <= 4 * np.spacing(np.float32(ws[9]))
  assert np.isnan(gs[12]) and (gs[13:] == 0).all()


@pytest.mark.parametrize('scale', [1.0, 30.0])
@pytest.mark.parametrize('shape', ref.RANDOM_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_random_shapes(shape, scale):
  name = 'random%s_s%g' % (shape, scale)
  _, v, s, gt = _inputs()[name]
  want, tols = _want(name)
  _assert_within(_run(v, s, gt), want, tols, what=name)


def test_single_contributing_cell():
  v, c = ref.single_cell_votes()
  scale = 2.5
  gxy, gr, gs, gc = _run(v, scale)
  x = float(np.float32(scale) * np.float32(v[c]))
  assert gc.tolist() == [1, 0, 0]
  assert gs[0] == np.float32(x) and gs[1] == np.float32(x)
  assert gs[2] == c[1] and gs[3] == c[2] and (gs[4:7] == 0).all() and gs[11] == 0
  assert abs(float(gs[9]) - c[0]) <= 1e-5 and abs(float(gs[10]) - 1) <= 2.0 ** -23
  assert not np.isnan(gxy).any() and not np.isnan(gr).any() and not np.isnan(gs[:12]).any()
  one_xy = np.full(v.shape[1:], -np.inf, np.float32)
  one_xy[c[1], c[2]] = 0
  one_r = np.full(v.shape[0], -np.inf, np.float32)
  one_r[c[0]] = 0
  assert (gxy == one_xy).all() and (gr == one_r).all()
  _assert_within((gxy, gr, gs, gc), *_want('single'), what='single')


@pytest.mark.parametrize('shape', [(36, 31, 33), (3, 1, 1)], ids=lambda s: '%dx%dx%d' % s)
def test_empty_volume(shape):
  gxy, gr, gs, gc = _run(np.full(shape, -np.inf, np.float32), 1.0, (0.5, 0.0, 0.0))
  assert (gxy == -np.inf).all() and (gr == -np.inf).all()
  assert gs[0] == -np.inf and gs[1] == -np.inf and np.isnan(gs[2:13]).all() and (gs[13:] == 0).all()
  assert gc.tolist() == [0, 0, 0]


def test_nan_and_plus_inf_are_excluded_and_counted():
  bad, masked, n = ref.nan_inf_votes()
  got_bad, got_masked = _run(bad, 30.0), _run(masked, 30.0)
  assert got_bad[3].tolist() == [got_masked[3][0], n, 0] and got_masked[3][1] == 0
  for a, b in zip(got_bad[:3], got_masked[:3]):              # the rest is unchanged, bit for bit
    assert guarded.same_bits(torch.from_numpy(a), torch.from_numpy(b))
  _assert_within(got_bad, *_want('nan_inf'), what='nan_inf')


def test_sharp_far_corner_peak():
  """sigma = 0.7 cells around (Ho - 1.3, Wo - 1.6) at [8, 200, 210]: E[a^2] ~ 4e4 against Var a ~ 0.5.  An f32
  E[a^2] - E[a]^2 is outside the bound here (test_vote_posterior_reference pins that)."""
  want, tols = _want('peak')
  assert tols[2][4] < 1e-5 and tols[2][2] < 1e-4
  got = _run(ref.peak_votes(), 1.0)
  _assert_within(got, want, tols, what='peak')


def test_several_tiles_per_workgroup():
  """[2, 520, 520]: 1057 tiles on 1024 workgroups, so workgroups 0 .. 32 fold two tiles each into their running
  sums: a fully masked tile before a live one (0 .. 9), a live one before a masked one (16 .. 25), a low maximum
  before a maximum 20 higher and one 35 higher before a lower (``ref.fold_votes``).  The ground-truth index lies in
  a second tile."""
  _, v, scale, gt = _inputs()['fold']
  assert v.shape[1] * v.shape[2] > 1024 * ref.TILE
  tile_live = np.isfinite(np.pad(v.reshape(2, -1), ((0, 0), (0, 1057 * 256 - 520 * 520)), constant_values=-np.inf)
                          ).reshape(2, 1057, 256).any((0, 2))
  assert not tile_live[:10].any() and tile_live[1024:1034].all() and tile_live[16:26].all() and not tile_live[1040:1050].any()
  want, tols = _want('fold')
  assert want[3][2] == 1 and tols[2][0] < 1e-4 and tols[2][11] < 1e-4
  _assert_within(_run(v, scale, gt), want, tols, what='fold')


def test_axis_order_of_the_expected_pose_and_covariance():
  """A Gaussian on rotation 0, sigma 3 cells along a and 1 along b, centred at (a, b) = (15, 9) of a 31 x 31 volume
  (a 16 x 16 grid of 0.25 m cells): index a is the map's x.  With rotation 0 the conjugation is the identity, so the
  expected translation is ((E a, E b) - extent + 1.5) * cell_size = (0.125, -1.375) m, written out here."""
  v = ref.aniso_votes()
  grid = grids.Grid2D((16, 16), 0.25)
  post = pev.posterior_from_votes(torch.from_numpy(v).to(DEV), grid, 8)
  want = ref.vote_posterior(v, 1.0)[2]
  assert abs(want[2] - 15) < 1e-4 and abs(want[3] - 9) < 1e-6 and abs(want[6] - 1) < 1e-3 and 8.9 < want[4] < 9.1
  tf = post['map_t_query_expected']
  assert abs(float(tf.angle)) < 1e-6
  t = tf.t.cpu().numpy()
  assert abs(t[0] - (want[2] - 16 + 1.5) * 0.25) < 1e-5 and abs(t[1] - (want[3] - 16 + 1.5) * 0.25) < 1e-5
  assert abs(t[0] - 0.125) < 1e-4 and abs(t[1] + 1.375) < 1e-5
  cov = post['cov_xy'].cpu().numpy()
  assert cov[0, 0] > 4 * cov[1, 1]                              # x = a is the wide axis
  assert abs(cov[0, 0] - want[4] * 0.0625) < 1e-5 and abs(cov[1, 1] - want[6] * 0.0625) < 1e-6
  assert abs(cov[0, 1] - want[5] * 0.0625) < 1e-6 and cov[0, 1] == cov[1, 0]
  assert abs(float(post['yaw_resultant']) - 1) < 1e-6
  _assert_within(tuple(post[k].cpu().numpy() for k in ('log_prob_xy', 'log_prob_r', 'stats', 'count')),
                 *_want('aniso'), what='aniso')


def test_ground_truth_sample():
  v, cases = ref.gt_cases()
  for name, idx, valid in cases:
    want, tols = _want('gt_' + name)
    assert want[3][2] == valid
    got = _run(v, 3.0, idx)
    assert got[3][2] == valid and bool(np.isnan(got[2][12])) == (not valid), name
    _assert_within(got, want, tols, what='gt_' + name)
  none = _run(v, 3.0, None)
  assert none[3][2] == 0 and np.isnan(none[2][12])
  for a, b in zip(none[:2], got[:2]):                          # the sample changes nothing else
    assert (a.view(np.int32) == b.view(np.int32)).all()
  assert (none[2][:12].view(np.int32) == got[2][:12].view(np.int32)).all()


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('random(36, 31, 33)_s30', 'random(64, 5, 300)_s1', 'peak', 'gt_interior', 'fold'):
    _, v, scale, gt = _inputs()[name]
    votes = torch.from_numpy(v.copy()).to(DEV)
    gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
    first = ops.vote_posterior(votes, scale, gt_dev)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_posterior(votes, scale, gt_dev)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    # the C entry point on one workspace, left full of garbage between the calls
    R, Ho, Wo = v.shape
    nbytes = lib.snap_vote_posterior_workspace_bytes(R, Ho, Wo)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    outs = []
    for fill in (0x7ff8000000000001, -1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = (torch.empty((Ho, Wo), device=DEV), torch.empty((R,), device=DEV), torch.empty((16,), device=DEV),
           torch.empty((3,), dtype=torch.int32, device=DEV))
      st = lib.snap_vote_posterior_f32(
          ctypes.c_void_p(votes.data_ptr()), R, Ho, Wo, scale, None if gt_dev is None else ctypes.c_void_p(gt_dev.data_ptr()),
          *(ctypes.c_void_p(t.data_ptr()) for t in o), ctypes.c_void_p(ws.data_ptr()), nbytes,
          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_raise_without_launching():
  votes = torch.zeros((4, 5, 6), device=DEV)
  with pytest.raises(ValueError):
    ops.vote_posterior(torch.zeros((65, 5, 5), device=DEV))
  for scale in (0.0, -2.0, float('inf'), float('nan')):
    with pytest.raises(ValueError):
      ops.vote_posterior(votes, scale)
  with pytest.raises(ValueError):
    ops.vote_posterior(votes[0])
  with pytest.raises(ValueError):
    ops.vote_posterior(votes, 1.0, torch.zeros(2, device=DEV))
  lib = _lib.load()
  need = lib.snap_vote_posterior_workspace_bytes(4, 5, 6)
  ws = torch.empty(need // 8, dtype=torch.int64, device=DEV)
  o = [torch.full((n,), 7.0, device=DEV) for n in (30, 4, 16)] + [torch.full((3,), 7, dtype=torch.int32, device=DEV)]
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  call = lambda R, scale, nbytes: lib.snap_vote_posterior_f32(p(votes), R, 5, 6, scale, None, *(p(t) for t in o),
                                                             p(ws), nbytes, None)
  assert call(65, 1.0, 1 << 20) == -1 and call(4, 0.0, need) == -2 and call(4, float('nan'), need) == -2
  assert call(4, 1.0, need - 1) == -5
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in o)                  # nothing ran


@pytest.mark.parametrize('method,D', [('fft', 6), ('direct', 8)])
def test_posterior_from_votes_and_localize_exhaustive(method, D):
  """A planted pose at 16^2, R = 8: the map is the query rotated by one rotation step and shifted by whole cells, on
  both voting formulations.  The expected pose and the nll are the numpy reference's on the returned votes; without
  the argument ``localize_exhaustive`` returns the same keys and bits as before."""
  H, R = 16, 8
  rng = np.random.default_rng(77 + H)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  fq = torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV)
  fm = torch.roll(torch.rot90(fq, 2, (0, 1)), (2, -1), (0, 1)).contiguous()      # rotation index R / 2, shifted
  pq, pm = types.FeaturePlane(features=fq, valid=valid), types.FeaturePlane(features=fm, valid=valid)
  base = pev.localize_exhaustive(pq, pm, R, grid, method=method)
  assert set(base) == {'map_t_query', 'index', 'score', 'count', 'votes'}
  gt_tf = pev.exhaustive_index_to_tfm(base['index'][0].to(torch.float32), grid, R)
  temperature = 4.0
  with guarded.scope():
    out = pev.localize_exhaustive(pq, pm, R, grid, method=method,
                                  posterior=dict(temperature=temperature, m_t_q_gt=gt_tf))
  assert set(out) == set(base) | {'posterior'}
  for k in base:
    a, b = (base[k], out[k]) if k != 'map_t_query' else (base[k].t, out[k].t)
    assert guarded.same_bits(a, b), k
  assert guarded.same_bits(base['map_t_query'].angle, out['map_t_query'].angle)
  post = out['posterior']
  assert set(post) == {'log_prob_xy', 'log_prob_r', 'log_z', 'entropy', 'map_t_query_expected', 'cov_xy',
                       'yaw_resultant', 'count', 'stats', 'nll', 'nll_valid'}
  votes = out['votes'].cpu().numpy()
  gt_idx = pev.exhaustive_tfm_to_index(gt_tf, grid, R).to(torch.float32).cpu().numpy()
  dgt = np.abs(gt_idx - base['index'][0].cpu().numpy())
  assert min(dgt[0], R - dgt[0]) < 1e-3 and dgt[1:].max() < 1e-3                # the planted index, to f32 rounding
  want = ref.vote_posterior(votes, temperature, gt_idx)
  tols = ref.bound(votes, temperature, gt_idx)
  got = (post['log_prob_xy'].cpu().numpy(), post['log_prob_r'].cpu().numpy(), post['stats'].cpu().numpy(),
         post['count'].cpu().numpy())
  _assert_within(got, want, tols, what=method)
  assert bool(post['nll_valid']) and want[3][2] == 1
  assert abs(float(post['nll']) + want[2][12]) <= 2 * tols[2][12]
  exp_tf = post['map_t_query_expected']
  ref_tf = pev.exhaustive_index_to_tfm(torch.tensor([want[2][9], want[2][2], want[2][3]], dtype=torch.float32), grid, R)
  dang = abs(float(exp_tf.angle) - float(ref_tf.angle))
  assert min(dang, 2 * np.pi - dang) <= 2 * tols[2][9] * 2 * np.pi / R + 1e-6
  assert float((exp_tf.t.cpu() - ref_tf.t).abs().max()) <= (2 * max(tols[2][2], tols[2][3]) * 0.25
                                                             + 4 * 2 * tols[2][9] * 2 * np.pi / R + 1e-5)
  cov = post['cov_xy'].cpu().numpy()
  assert cov.shape == (2, 2) and cov[0, 1] == cov[1, 0]
  assert np.allclose(cov, 0.0625 * np.array([[want[2][4], want[2][5]], [want[2][5], want[2][6]]]), rtol=1e-5,
                     atol=0.0625 * 2 * max(tols[2][4:7]))
  assert float(post['log_z']) == float(post['stats'][0]) and float(post['entropy']) == float(post['stats'][11])
  # posterior=True: the defaults (temperature 1, no ground truth)
  plain = pev.localize_exhaustive(pq, pm, R, grid, method=method, posterior=True)['posterior']
  assert 'nll' not in plain and plain['count'][2] == 0
  w1 = ref.vote_posterior(votes, 1.0)
  assert abs(float(plain['log_z']) - w1[2][0]) <= 2 * ref.bound(votes, 1.0)[2][0]
