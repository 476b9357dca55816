"""`-m gpu`: ``ops.vote_modes`` (vote_modes.hip, through the C ABI) and the host entry points built on it, against the
float64 restatement ``vote_modes_reference``.

Both sides round a float64 value to f32 once, and the two float64 values differ only by libm and the order of the sums
(<= ~1e-12 relative), so: counts and the -inf / NaN / 0 patterns are EQUAL; log_mass, m_k and the means are within 2
f32 ulps; the covariances within 2 f32 ulps + 1e-10 win_xy^2 (the cancellation of E[d d'] - E[d] E[d'], offsets up to
win_xy, in float64); nees_gt within 1e-6 relative (cond(Sigma + I / 12) <= 1e4 is asserted on the reference).  Every
call runs under ``guarded.scope()``: guard regions intact (outputs and workspace), no output element left unwritten.

Observed on an MI355X (each test prints its figures): every mass, mean and covariance within 0.01 of its tolerance
(most rows equal the rounded reference bit for bit); nees_gt within 5.8e-8 relative, i.e. inside its f32 rounding."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_modes_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


@functools.lru_cache(maxsize=None)
def _cases():
  return {c['name']: c for c in ref.cases()}


def _run(votes, peaks, win_r, win_xy, scale, gt):
  """One guarded call; ``peaks`` a numpy table or a device tensor -> (stats, count) as numpy arrays."""
  v = torch.from_numpy(np.ascontiguousarray(votes)).to(DEV)
  pk = peaks if isinstance(peaks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(peaks, dtype=np.int32)).to(DEV)
  gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
  R, Ho, Wo = votes.shape
  K = pk.shape[0]
  with guarded.scope() as sc:
    gtp = None if gt_dev is None else guarded.place(gt_dev, 'address')
    stats, count = ops.vote_modes(guarded.place(v, 'value'), guarded.place(pk, 'address'), win_r, win_xy, scale, gtp)
    assert tuple(stats.shape) == (K, 16) and stats.dtype == torch.float32
    assert tuple(count.shape) == (K, 2) and count.dtype == torch.int32
    ws = [a for a in sc.allocations('vote_modes') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_modes_workspace_bytes(R, Ho, Wo, K, win_r, win_xy)
    # (the poison is all-ones: a NaN other than the kernel's 0x7fc00000, and -1, which no count is)
    assert not bool(guarded.unwritten(stats).any()) and not bool(guarded.unwritten(count).any())
    res = stats.cpu().numpy(), count.cpu().numpy()
  return res


def _ulps(x32, n=2):
  return n * np.spacing(np.abs(x32).astype(np.float32)).astype(np.float64)


def _assert_close(got, want, R, win_xy, what):
  (gs, gc), (ws64, wc) = got, want
  assert (gc == wc).all(), f'{what}: count\n{gc}\n!=\n{wc}'
  ws = ref.round_stats(ws64, R)
  assert (np.isnan(gs) == np.isnan(ws)).all() and (np.isneginf(gs) == np.isneginf(ws)).all(), f'{what}: patterns'
  assert (gs[:, 12:] == 0).all() and not np.isposinf(gs).any()
  live = np.isfinite(ws[:, 0])
  if not live.any():
    return
  g, w = gs[live].astype(np.float64), ws[live]
  err = np.abs(g[:, :11] - w[:, :11].astype(np.float64))
  tol = _ulps(w[:, :11])
  tol[:, 5:11] += 1e-10 * win_xy ** 2
  print(f'{what}: worst error / tolerance: masses {np.max(err[:, :2] / tol[:, :2]):.2f}, means '
        f'{np.max(err[:, 2:5] / tol[:, 2:5]):.2f}, covariances {np.max(err[:, 5:] / tol[:, 5:]):.2f}')
  assert (err <= tol).all(), f'{what}: stats\n{g[:, :11]}\nvs\n{w[:, :11]}'
  gn, wn = g[:, 11], ws64[live][:, 11]
  assert (np.isnan(gn) == np.isnan(wn)).all(), f'{what}: nees patterns'
  ok = ~np.isnan(wn)
  if ok.any():
    assert ref.nees_condition(ws64) <= 1e4
    rel = np.abs(gn[ok] - wn[ok]) / np.maximum(np.abs(wn[ok]), 1e-300)
    print(f'{what}: nees worst relative error {rel.max():.2e}')
    assert (rel <= 1e-6).all(), f'{what}: nees {gn} vs {wn}'


@pytest.mark.parametrize('name', [c['name'] for c in ref.cases()])
def test_against_the_float64_reference(name):
  c = _cases()[name]
  want = ref.vote_modes(c['votes'], c['peaks'], c['win_r'], c['win_xy'], c['scale'], c['gt'])[:2]
  got = _run(c['votes'], c['peaks'], c['win_r'], c['win_xy'], c['scale'], c['gt'])
  _assert_close(got, want, c['votes'].shape[0], c['win_xy'], name)
  if name.startswith('all_masked') or name.startswith('masked_window'):
    assert got[1][0].tolist() == [0, 0] and got[0][0, 0] == -np.inf and np.isnan(got[0][0, 2:12]).all()
  if name.startswith('duplicate'):
    assert got[1][2].tolist() == [0, 0] and got[1][4].tolist() == [0, 0] and got[1][1, 0] > 0
  if name.startswith('nan_inf'):
    assert got[1][0, 1] == 3
  if name.startswith('gt_not_finite'):
    assert np.isnan(got[0][0, 11]) and np.isfinite(got[0][0, :11]).all()
  if name.startswith('one_cell'):
    # Sigma = 0: the I / 12 term alone, e = (-0.1, 0.25, 0.25) with the rotation wrapped
    assert got[1][0].tolist() == [1, 0] and (got[0][0, 5:11] == 0).all()
    assert abs(got[0][0, 11] - 12 * (0.1 ** 2 + 2 * 0.25 ** 2)) <= 1e-5


@pytest.mark.parametrize('shape', ref.SHAPES)
@pytest.mark.parametrize('setting', ref.SETTINGS)
def test_peak_tables_of_vote_peaks(shape, setting):
  """The table ``ops.vote_peaks`` writes (its -1 rows past the found count included) goes in as it is, on the device."""
  K, win_r, win_xy = setting
  if not ref.supported(*shape, K, win_r, win_xy):
    with pytest.raises(ValueError):
      ops.vote_modes(torch.zeros(shape, device=DEV), torch.zeros((K, 3), dtype=torch.int32, device=DEV), win_r, win_xy)
    return
  v = ref.smooth_votes(shape, seed=31 + K)
  index = ops.vote_peaks(torch.from_numpy(v).to(DEV), K, min(win_r, 2), min(win_xy, 4))[0]
  peaks = index.cpu().numpy()
  gt = (0.5, 1.25, 2.0)
  got = _run(v, index, win_r, win_xy, 2.0, gt)
  want = ref.vote_modes(v, peaks, win_r, win_xy, 2.0, gt)[:2]
  _assert_close(got, want, shape[0], win_xy, f'vote_peaks{shape}{setting}')
  found = (peaks[:, 0] >= 0).sum()
  assert found >= 1 and (got[1][found:] == 0).all() and (got[0][found:, 0] == -np.inf).all()


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('normal(36, 63, 63)_K64_w2_16', 'normal(8, 31, 33)_K5_w3_32', 'nan_inf_w1_4', 'empty_rows_w1_4'):
    c = _cases()[name]
    votes = torch.from_numpy(c['votes'].copy()).to(DEV)
    peaks = torch.from_numpy(c['peaks']).to(DEV)
    gt = torch.tensor(c['gt'], dtype=torch.float32, device=DEV)
    first = ops.vote_modes(votes, peaks, c['win_r'], c['win_xy'], c['scale'], gt)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_modes(votes, peaks, c['win_r'], c['win_xy'], c['scale'], gt)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = c['votes'].shape
    K = peaks.shape[0]
    nbytes = lib.snap_vote_modes_workspace_bytes(R, Ho, Wo, K, c['win_r'], c['win_xy'])
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for fill in (0x7ff8000000000001, -1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = [torch.empty_like(t) for t in first]
      st = lib.snap_vote_modes_f32(p(votes), R, Ho, Wo, c['scale'], p(peaks), K, c['win_r'], c['win_xy'], p(gt), p(o[0]),
                                   p(o[1]), p(ws), nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      torch.cuda.synchronize()
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_return_their_codes_without_launching():
  lib = _lib.load()
  R, Ho, Wo = 8, 5, 6
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  peaks = torch.zeros((64, 3), dtype=torch.int32, device=DEV)
  stats = torch.full((64, 16), 7.0, device=DEV)
  count = torch.full((64, 2), 7, dtype=torch.int32, device=DEV)
  need = lib.snap_vote_modes_workspace_bytes(R, Ho, Wo, 64, 3, 32)
  assert need > 0 and need % 8 == 0
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  p = lambda t: ctypes.c_void_p(t.data_ptr())

  def call(R=R, Ho=Ho, Wo=Wo, K=4, win_r=1, win_xy=4, scale=1.0, vp=p(votes), pp=p(peaks), sp=p(stats), cp=p(count),
           wsp=p(ws), nbytes=need):
    return lib.snap_vote_modes_f32(vp, R, Ho, Wo, scale, pp, K, win_r, win_xy, None, sp, cp, wsp, nbytes, None)

  bad_shapes = [dict(K=0), dict(K=65), dict(K=-1), dict(win_r=-1), dict(win_r=5), dict(K=1, win_r=4), dict(win_xy=0),
                dict(win_xy=33), dict(R=0), dict(Ho=0), dict(Wo=0), dict(R=2, win_r=1), dict(R=2048, Ho=1024, Wo=1024)]
  for kw in bad_shapes:
    assert call(**kw) == -1, kw
    q = dict(R=R, Ho=Ho, Wo=Wo, K=4, win_r=1, win_xy=4)
    q.update(kw)
    assert lib.snap_vote_modes_workspace_bytes(q['R'], q['Ho'], q['Wo'], q['K'], q['win_r'], q['win_xy']) == 0, kw
  assert lib.snap_vote_modes_workspace_bytes(9, Ho, Wo, 1, 4, 4) > 0          # (win_r = 4 needs R >= 9)
  for scale in (0.0, -2.0, float('inf'), float('nan')):
    assert call(scale=scale) == -2, scale
  for kw in (dict(vp=None), dict(pp=None), dict(sp=None), dict(cp=None), dict(wsp=None)):
    assert call(**kw) == -3, kw
  assert call(nbytes=lib.snap_vote_modes_workspace_bytes(R, Ho, Wo, 4, 1, 4) - 1) == -5          # short
  assert call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5                                       # misaligned
  torch.cuda.synchronize()
  assert bool((stats == 7).all()) and bool((count == 7).all())                                   # nothing ran
  # the wrapper refuses on the host
  pk = peaks[:4].contiguous()
  for kw in (dict(win_r=5), dict(win_r=4), dict(win_xy=0), dict(win_xy=33), dict(scale=0.0), dict(scale=float('nan'))):
    with pytest.raises(ValueError):
      ops.vote_modes(votes, pk, **kw)
  for bad in (pk.to(torch.int64), pk[:, :2].contiguous(), pk.cpu(), peaks[:0]):
    with pytest.raises(ValueError):
      ops.vote_modes(votes, bad)
  with pytest.raises(ValueError):
    ops.vote_modes(votes[0], pk)
  with pytest.raises(ValueError):
    ops.vote_modes(votes, pk, gt_index=torch.zeros(2, device=DEV))


# ------------------------------- the wrapper level ------------------------------------------------
def _assert_modes(out, votes, peaks, grid, R, win_r, win_xy, temperature, lz_arg, gt_idx, what):
  """``modes_from_votes``' dict against the reference's propagation of the reference's rows.  The op's rows are within
  the tolerances above of the reference's; those bounds are carried through exp (weight), through the pose map and
  through J Sigma J^T, each with the final f32 rounding of the wrapper's output added."""
  extent, cell = tuple(grid.extent), float(grid.cell_size)
  stats64, count = ref.vote_modes(votes, peaks, win_r, win_xy, temperature, gt_idx)[:2]
  s32 = ref.round_stats(stats64, R)
  lz64 = ref.log_z(votes, temperature) if lz_arg is None else lz_arg
  want = ref.modes(s32, lz64, extent, cell, R)
  live = np.isfinite(s32[:, 0])
  assert live.any() and (out['count'].cpu().numpy() == count).all()
  eps = 2.0 ** -24
  # weight = exp(log_mass - log_z): 2 ulps of the f32 log_mass, 2 ulps of an f32 log_z (vote_posterior's own output)
  d_log = _ulps(s32[:, 0]) + (0.0 if lz_arg is not None else _ulps(np.float32(lz64)))
  w_got = out['weight'].cpu().numpy().astype(np.float64)
  w_tol = want['weight'] * (np.where(live, d_log, 0.0) * 1.01 + eps)
  assert (np.abs(w_got - want['weight']) <= w_tol).all(), f'{what}: weight {w_got} vs {want["weight"]}'
  assert (w_got[~live] == 0).all()
  exact = 1.0 - np.exp(stats64[live, 0] - lz64).sum()
  print(f'{what}: unassigned {float(out["unassigned"]):.6f}, float64 {exact:.6f}')
  assert abs(float(out['unassigned']) - exact) <= 1e-6
  # pose and covariance
  pose = np.concatenate([out['map_t_query'].angle.cpu().numpy()[:, None], out['map_t_query'].t.cpu().numpy()], -1)
  cov = out['cov'].cpu().numpy().astype(np.float64)
  cov_index = out['cov_index'].cpu().numpy()
  assert np.isnan(pose[~live]).all() and np.isnan(cov[~live]).all()
  tol_s = _ulps(s32[:, :11])
  tol_s[:, 5:11] += 1e-10 * win_xy ** 2
  tri = [(0, 0, 5), (0, 1, 6), (0, 2, 7), (1, 1, 8), (1, 2, 9), (2, 2, 10)]
  for k in np.nonzero(live)[0]:
    J = np.abs(ref.pose_jacobian(s32[k, 2:5], extent, cell, R))
    p_tol = J @ tol_s[k, 2:5] + eps * np.abs(want['pose'][k]) + 1e-12
    assert (np.abs(pose[k] - want['pose'][k]) <= p_tol).all(), f'{what}: pose {k}: {pose[k]} vs {want["pose"][k]}'
    T = np.zeros((3, 3))
    for i, j, col in tri:
      T[i, j] = T[j, i] = tol_s[k, col]
      assert abs(float(cov_index[k, i, j]) - float(s32[k, col])) <= tol_s[k, col] and cov_index[k, i, j] == cov_index[k, j, i]
    # (J itself moves with the mean rotation by 2 ulps of it: second order, covered by 4 eps of the term sizes)
    size = J @ np.abs(want['cov_index'][k]) @ J.T
    c_tol = J @ T @ J.T + 5 * eps * size + 1e-15
    assert (np.abs(cov[k] - want['cov'][k]) <= c_tol).all(), f'{what}: cov {k}:\n{cov[k]}\nvs\n{want["cov"][k]}'
  if gt_idx is not None:
    gn, wn = out['nees'].cpu().numpy().astype(np.float64), stats64[:, 11]
    assert (np.isnan(gn) == np.isnan(wn)).all() and ref.nees_condition(stats64) <= 1e4
    ok = ~np.isnan(wn)
    assert (np.abs(gn[ok] - wn[ok]) <= 1e-6 * np.abs(wn[ok])).all(), f'{what}: nees {gn} vs {wn}'
  else:
    assert 'nees' not in out


def _planted_scene(H, R, D, seed):
  rng = np.random.default_rng(seed)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  fq = torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV)
  fm = torch.roll(torch.rot90(fq, 2, (0, 1)), (2, -1), (0, 1)).contiguous()
  return grid, types.FeaturePlane(features=fq, valid=valid), types.FeaturePlane(features=fm, valid=valid)


def test_localize_exhaustive_modes():
  """[36, 63, 63] from a planted pose at 32^2: ``modes=True`` reuses the peaks and the posterior's log_z; without the
  argument ``localize_exhaustive`` returns the keys and bits it returned before."""
  H, R = 32, 36
  grid, pq, pm = _planted_scene(H, R, 8, seed=5)
  base = pev.localize_exhaustive(pq, pm, R, grid)
  assert set(base) == {'map_t_query', 'index', 'score', 'count', 'votes'}
  assert tuple(base['votes'].shape) == (36, 63, 63)
  gt_tf = pev.exhaustive_index_to_tfm(base['index'][0].to(torch.float32) + torch.tensor([0.2, -0.3, 0.4], device=DEV),
                                      grid, R)
  temperature = 0.05
  with guarded.scope():
    out = pev.localize_exhaustive(pq, pm, R, grid, posterior=dict(temperature=temperature),
                                  modes=dict(temperature=temperature, m_t_q_gt=gt_tf, win_xy=3), radius_xy=2)
    plain = pev.localize_exhaustive(pq, pm, R, grid, posterior=True, modes=True)
  assert set(out) == set(base) | {'posterior', 'modes'}
  for k in ('votes', 'score'):
    assert guarded.same_bits(base[k], plain[k]), k
  m = out['modes']
  assert set(m) == {'weight', 'unassigned', 'index_mean', 'map_t_query', 'cov_index', 'cov', 'count', 'stats', 'index',
                    'nees'}
  assert m['index'] is out['index']
  votes, peaks = out['votes'].cpu().numpy(), out['index'].cpu().numpy()
  gt_idx = pev.exhaustive_tfm_to_index(gt_tf, grid, R).to(torch.float32).cpu().numpy()
  _assert_modes(m, votes, peaks, grid, R, 1, 3, temperature, None, gt_idx, 'localize')
  # the best mode belongs to the planted pose: its mean stays inside its window
  st = m['stats'].cpu().numpy()
  assert np.abs(st[0, 3:5] - peaks[0, 1:]).max() <= 3 and np.isfinite(float(m['nees'][0]))
  assert 0 < float(m['weight'][0]) <= 1 and -1e-6 <= float(m['unassigned']) < 1
  _assert_modes(plain['modes'], plain['votes'].cpu().numpy(), plain['index'].cpu().numpy(), grid, R, 1, 1, 1.0, None,
                None, 'localize plain')


def test_vote_filter_modes():
  """``VoteFilter.modes`` works on the belief (log space, normalised: scale 1, log_z 0)."""
  H, R = 32, 36
  grid = grids.Grid2D((H, H), 0.25)
  v = ref.smooth_votes((R, 2 * H - 1, 2 * H - 1), seed=4)
  f = pev.VoteFilter(grid, R, sigma_xy=0.3, sigma_yaw=0.1, temperature=2.0)
  with pytest.raises(ValueError):
    f.modes()
  f.step(torch.from_numpy(v).to(DEV))
  gt_tf = pev.exhaustive_index_to_tfm(torch.tensor([3.0, 12.0, 20.0]), grid, R)
  with guarded.scope():
    out = f.modes(num_peaks=8, radius_r=2, radius_xy=4, win_xy=6, m_t_q_gt=gt_tf)
  belief = f.belief.cpu().numpy()
  gt_idx = pev.exhaustive_tfm_to_index(gt_tf, grid, R).to(torch.float32).cpu().numpy()
  assert tuple(out['index'].shape) == (8, 3)
  _assert_modes(out, belief, out['index'].cpu().numpy(), grid, R, 2, 6, 1.0, 0.0, gt_idx, 'filter')
  # the belief is normalised: the exact log_z is 0 to f32 accuracy, so the weights are probabilities
  assert abs(ref.log_z(belief, 1.0)) <= 1e-5
