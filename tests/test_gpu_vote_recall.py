"""`-m gpu`: ``ops.vote_recall`` (vote_recall.hip, through the C ABI) and the host entry points built on it, against the
float64 restatement ``vote_recall_reference``.

Both sides round a float64 log mass to f32 once, and the two float64 values differ only by libm and the order of sums
of non-negative terms, so: counts and the -inf / NaN patterns are EQUAL and every log mass (maps, centres, ground
truth, best) is within 2 f32 ulps of the rounded reference, plus ``ref.float64_slack``: log(ball) - log S cancels for a
ball that holds nearly all of the mass (the issue's own [3, 5, 6] case with a ball larger than the volume has the exact
answer 0, where an f32 ulp is 1.4e-45 and two float64 sums of the same terms in two orders differ by ~1e-16), so the
float64 error of the operands, <= 2^-52 (2 R Ho Wo + 8 log S) < 7e-11 at these shapes, is added.  It exceeds one f32
ulp only where |log mass| < ~1e-4.  Every call runs under ``guarded.scope()``: guard regions intact (outputs and
workspace), no output element left unwritten, one workspace allocation of exactly ``workspace_bytes``."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_recall_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
NAMES = [c['name'] for c in ref.cases()]


def _run(votes, rho2, half_r, centres, scale, gt, maps=True):
  """One guarded call; ``centres`` None, a numpy table or a device tensor -> the op's outputs as numpy arrays."""
  v = torch.from_numpy(np.ascontiguousarray(votes)).to(DEV)
  ct = centres
  if centres is not None and not isinstance(centres, torch.Tensor):
    ct = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.int32)).to(DEV)
  gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
  R, Ho, Wo = votes.shape
  K, L = 0 if ct is None else ct.shape[0], len(rho2)
  with guarded.scope() as sc:
    gtp = None if gt_dev is None else guarded.place(gt_dev, 'address')
    ctp = None if ct is None else guarded.place(ct, 'address')
    out = ops.vote_recall(guarded.place(v, 'value'), rho2, half_r, ctp, scale, gtp, maps)
    shapes = [(L, 3), (L,), (K, L), (L,), (4,), (4,)] + ([(L, R, Ho, Wo)] if maps else [])
    # (the poison is all-ones: a NaN other than the kernel's 0x7fc00000, and -1, which no count is; -1 IS best_index's
    # value without a finite cell, so that table is checked against the kernel's own maps instead, exactly)
    for t, shape in zip(out, shapes):
      assert tuple(t.shape) == shape and (t is out[0] or not bool(guarded.unwritten(t).any()))
    assert (out[6] is None) == (not maps)
    ws = [a for a in sc.allocations('vote_recall') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_recall_workspace_bytes(R, Ho, Wo, K, L)
    res = [None if t is None else t.cpu().numpy() for t in out]
  return res


def _ulps(x32, n=2):
  x = np.where(np.isfinite(x32), np.abs(x32), 0).astype(np.float32)
  return n * np.spacing(x).astype(np.float64)


def _assert_log_mass(got, want64, slack, what):
  """f32 ``got`` against float64 ``want64``: equal -inf / NaN patterns, 2 f32 ulps + the float64 slack elsewhere."""
  want = ref.round_log_mass(want64)
  assert got.dtype == np.float32 and got.shape == want.shape, what
  assert (np.isnan(got) == np.isnan(want)).all() and (np.isneginf(got) == np.isneginf(want)).all(), f'{what}: patterns'
  assert not np.isposinf(got).any() and not (got > 0).any(), what
  live = np.isfinite(want)
  if not live.any():
    return 0.0
  err = np.abs(got[live].astype(np.float64) - want[live].astype(np.float64))
  tol = _ulps(want[live]) + slack
  worst = float(np.max(err / tol))
  print(f'{what}: worst error / tolerance {worst:.3f}; {int((err > _ulps(want[live])).sum())} of {err.size} elements '
        f'beyond 2 ulps alone (all with |log mass| < {float(np.abs(want[live][err > _ulps(want[live])]).max(initial=0)):.1e})')
  assert (err <= tol).all(), f'{what}: {got[live][err > tol][:8]} vs {want[live][err > tol][:8]}'
  return worst


def _assert_case(got, c, want, what):
  best_index, best_lm, centre_lm, gt_lm, stats, count, maps = got
  shape = c['votes'].shape
  slack = ref.float64_slack(shape, want['log_z'], want['m'])
  assert (count == want['count']).all(), f'{what}: count {count} != {want["count"]}'
  ws = ref.round_stats(want['log_z'], want['m'])
  assert (stats[2:] == 0).all() and (np.isneginf(stats[:2]) == np.isneginf(ws[:2])).all()
  fin = np.isfinite(ws[:2])
  assert (np.abs(stats[:2][fin].astype(np.float64) - ws[:2][fin]) <= _ulps(ws[:2][fin])).all(), f'{what}: stats {stats}'
  _assert_log_mass(maps, want['maps'], slack, f'{what} maps')
  _assert_log_mass(centre_lm, want['centre'], slack, f'{what} centres')
  _assert_log_mass(gt_lm, want['gt'], slack, f'{what} gt')
  # the best cell: exactly the first flat arg-max of the kernel's OWN maps ...
  own_index, own_value = ref.best_of(maps)
  assert (best_index == own_index).all(), f'{what}: best_index\n{best_index}\nvs own maps\n{own_index}'
  assert (best_lm.view(np.int32) == own_value.view(np.int32)).all(), f'{what}: best_log_mass'
  # ... and as good as the reference's maximum, to 2 ulps a side
  want32 = ref.round_log_mass(want['maps'])
  ref_index, ref_value = ref.best_of(want32)
  assert ((best_index[:, 0] < 0) == (ref_index[:, 0] < 0)).all()
  _assert_log_mass(best_lm, ref_value.astype(np.float64), slack, f'{what} best')
  for l in range(len(c['rho2'])):
    if ref_index[l, 0] < 0:
      continue
    at = float(want32[l][tuple(best_index[l])])
    assert at >= float(ref_value[l]) - (_ulps(ref_value[l:l + 1], 4)[0] + 2 * slack), f'{what}: level {l}'
    if c['planted'] is not None:
      ball = ref.ball_mask(shape, ref_index[l], c['rho2'][l], c['half_r'][l])
      outside = float(want32[l][~ball].max())
      assert float(ref_value[l]) - outside > _ulps(ref_value[l:l + 1], 8)[0] + 4 * slack     # decided on the reference
      assert ball[tuple(best_index[l])] and ball[c['planted']], f'{what}: level {l}: {best_index[l]}'


@pytest.mark.parametrize('name', NAMES)
def test_against_the_float64_reference(name):
  c, want = ref.shared()[name]
  got = _run(c['votes'], c['rho2'], c['half_r'], c['centres'], c['scale'], c['gt'])
  _assert_case(got, c, want, name)
  if name == 'all_masked':
    assert (got[0] == -1).all() and np.isneginf(got[1]).all() and np.isneginf(got[6]).all()
    assert np.isneginf(got[4][:2]).all() and got[5].tolist() == [0, 0, 1, 0]
  if name == 'ball_covers_volume':
    assert np.abs(got[6]).max() <= 1e-6
  if name == 'nan_inf':
    assert got[5][1] == 3 and np.isneginf(got[2][0, 0])
  if name in ('empty_rows_gt_out_of_range', 'gt_not_finite'):
    assert np.isnan(got[3]).all() and got[5][2] == 0
  if name == 'odd_L1':
    assert got[2].shape == (0, 1) and np.isnan(got[3]).all()
  # maps=False: every other output holds the same bytes
  lean = _run(c['votes'], c['rho2'], c['half_r'], c['centres'], c['scale'], c['gt'], maps=False)
  for a, b in zip(got[:6], lean[:6]):
    assert a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize('shape,border,rho2,half_r', [((8, 31, 33), 11, (3, 15, 63), (0, 1, 2)),
                                                      ((36, 63, 63), 4, (25,), (4,))])
def test_peak_tables_of_vote_peaks(shape, border, rho2, half_r):
  """The table ``ops.vote_peaks`` writes goes in as it is, on the device, with its -1 rows past the found count: the
  8 x 9 x 11 cells inside the first border hold at most 3 * 2 * 3 = 18 peaks of radii (2, 4)."""
  v = ref.mask_border(ref.smooth_votes(shape, seed=31), border)
  index = ops.vote_peaks(torch.from_numpy(v).to(DEV), 64, 2, 4)[0]
  peaks = index.cpu().numpy()
  found = int((peaks[:, 0] >= 0).sum())
  assert 1 <= found and (found < 64 or border != 11)
  gt = (0.5, 6.5, 20.0)
  got = _run(v, rho2, half_r, index, 2.0, gt)
  want = ref.vote_recall(v, rho2, half_r, peaks, 2.0, gt)
  _assert_case(got, dict(votes=v, rho2=rho2, half_r=half_r, planted=None), want, f'vote_peaks{shape}')
  assert np.isneginf(got[2][found:]).all() and np.isfinite(got[2][:found]).all()


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
  for name in ('c4_small_L8', 'odd_L8', 'nan_inf', 'single_row'):
    c, _ = ref.shared()[name]
    votes = torch.from_numpy(c['votes'].copy()).to(DEV)
    centres = torch.from_numpy(c['centres']).to(DEV)
    gt = torch.tensor(c['gt'], dtype=torch.float32, device=DEV)
    first = ops.vote_recall(votes, c['rho2'], c['half_r'], centres, c['scale'], gt, True)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_recall(votes, c['rho2'], c['half_r'], centres, c['scale'], gt, True)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = c['votes'].shape
    K, L = centres.shape[0], len(c['rho2'])
    nbytes = lib.snap_vote_recall_workspace_bytes(R, Ho, Wo, K, L)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    rho2, half_r = (ctypes.c_int32 * L)(*c['rho2']), (ctypes.c_int32 * L)(*c['half_r'])
    for fill in (0x7ff8000000000001, -1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = [torch.empty_like(t) for t in first]
      st = lib.snap_vote_recall_f32(p(votes), R, Ho, Wo, c['scale'], rho2, half_r, L, p(centres), K, p(gt), p(o[0]),
                                    p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[5]), p(o[6]), p(ws), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      torch.cuda.synchronize()
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_workspace_is_one_float64_volume_at_the_c4_shape():
  lib = _lib.load()
  nbytes = lib.snap_vote_recall_workspace_bytes(36, 511, 511, 64, 8)
  assert 8 * 36 * 511 * 511 <= nbytes < 256 * 10 ** 6 and nbytes < 1.01 * 8 * 36 * 511 * 511


def test_bad_arguments_return_their_codes_without_launching():
  lib = _lib.load()
  R, Ho, Wo = 9, 5, 6
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  centres = torch.zeros((64, 3), dtype=torch.int32, device=DEV)
  outs = [torch.full((8, 3), 7, dtype=torch.int32, device=DEV), torch.full((8,), 7.0, device=DEV),
          torch.full((64, 8), 7.0, device=DEV), torch.full((8,), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV),
          torch.full((4,), 7, dtype=torch.int32, device=DEV), torch.full((8, R, Ho, Wo), 7.0, device=DEV)]
  need = lib.snap_vote_recall_workspace_bytes(R, Ho, Wo, 64, 8)
  assert need > 0 and need % 8 == 0
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  arr = lambda v: (ctypes.c_int32 * len(v))(*v)

  def call(R=R, Ho=Ho, Wo=Wo, K=4, rho2=(1, 25), half_r=(0, 1), L=None, scale=1.0, vp=p(votes), cp=p(centres),
           rp=0, hp=0, wsp=p(ws), nbytes=need, null_out=None):
    op = [p(t) for t in outs]
    if null_out is not None:
      op[null_out] = None
    L = len(rho2) if L is None else L
    return lib.snap_vote_recall_f32(vp, R, Ho, Wo, scale, arr(rho2) if rp == 0 else rp, arr(half_r) if hp == 0 else hp,
                                    L, cp, K, None, *op, wsp, nbytes, None)

  assert call() == 0
  torch.cuda.synchronize()
  for t in outs[:2] + outs[3:6]:
    t.fill_(7)
  outs[2].fill_(7.0)
  outs[6].fill_(7.0)
  torch.cuda.synchronize()
  bad_shapes = [dict(K=65), dict(K=-1), dict(L=0), dict(L=9, rho2=(1,) * 9, half_r=(0,) * 9), dict(rho2=(1, -1)),
                dict(rho2=(1025, 1)), dict(half_r=(0, 5)), dict(half_r=(-1, 0)), dict(R=8, half_r=(0, 4)), dict(R=0),
                dict(R=65), dict(Ho=0), dict(Wo=0), dict(R=64, Ho=8192, Wo=8192)]
  for kw in bad_shapes:
    assert call(**kw) == -1, kw
  for kw in (dict(K=65), dict(K=-1), dict(L=0), dict(L=9), dict(R=0), dict(R=65), dict(Ho=0), dict(Wo=0),
             dict(R=64, Ho=8192, Wo=8192)):
    q = dict(R=R, Ho=Ho, Wo=Wo, K=4, L=2)
    q.update(kw)
    assert lib.snap_vote_recall_workspace_bytes(q['R'], q['Ho'], q['Wo'], q['K'], q['L']) == 0, kw
  assert lib.snap_vote_recall_workspace_bytes(1, 1, 1, 0, 1) > 0
  for scale in (0.0, -2.0, float('inf'), float('nan')):
    assert call(scale=scale) == -2, scale
  for kw in (dict(vp=None), dict(cp=None), dict(rp=None), dict(hp=None), dict(wsp=None), dict(null_out=0),
             dict(null_out=1), dict(null_out=2), dict(null_out=3), dict(null_out=4), dict(null_out=5)):
    assert call(**kw) == -3, kw
  assert call(nbytes=lib.snap_vote_recall_workspace_bytes(R, Ho, Wo, 4, 2) - 1) == -5          # short
  assert call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5                                     # misaligned
  torch.cuda.synchronize()
  for t in outs:
    assert bool((t == 7).all())                                                                 # nothing ran
  # K = 0 needs neither the table nor its output; maps may be NULL
  assert call(K=0, cp=None, null_out=2) == 0 and call(null_out=6) == 0
  torch.cuda.synchronize()
  # the wrapper refuses on the host
  ct = centres[:4].contiguous()
  for kw in (dict(rho2=(1025,)), dict(rho2=(-1,)), dict(half_r=(5,)), dict(half_r=(-1,)), dict(rho2=(), half_r=()),
             dict(rho2=(1,) * 9, half_r=(0,) * 9), dict(rho2=(1, 2)), dict(rho2=(1.5,)), dict(scale=0.0),
             dict(scale=float('nan')), dict(gt_index=torch.zeros(2, device=DEV))):
    q = dict(rho2=(1,), half_r=(0,))
    q.update(kw)
    with pytest.raises(ValueError):
      ops.vote_recall(votes, q.pop('rho2'), q.pop('half_r'), ct, **q)
  with pytest.raises(ValueError):
    ops.vote_recall(votes[:8].contiguous(), (1,), (4,))                                         # 2 half_r + 1 > R
  for bad in (ct.to(torch.int64), ct[:, :2].contiguous(), ct.cpu(), torch.zeros((65, 3), dtype=torch.int32, device=DEV)):
    with pytest.raises(ValueError):
      ops.vote_recall(votes, (1,), (0,), bad)
  with pytest.raises(ValueError):
    ops.vote_recall(votes[0], (1,), (0,))
  with pytest.raises(ValueError):
    ops.vote_recall(torch.zeros((65, 2, 2), device=DEV), (1,), (0,))


# ------------------------------- the wrapper level ------------------------------------------------
def _assert_poses(out, grid, R, what):
  """``map_t_query`` against the reference's propagation of ``best_index`` (the f32 tolerance of the modes test's
  pose check at an exact lattice index: the rounding of the output alone)."""
  index = out['best_index'].cpu().numpy()
  pose = np.concatenate([out['map_t_query'].angle.cpu().numpy()[:, None], out['map_t_query'].t.cpu().numpy()], -1)
  for l, row in enumerate(index):
    if row[0] < 0:
      assert np.isnan(pose[l]).all()
      continue
    want = ref.index_to_pose(row, tuple(grid.extent), float(grid.cell_size), R)
    tol = 4 * 2.0 ** -24 * (np.abs(want) + float(np.max(grid.extent)) * float(grid.cell_size)) + 1e-12
    assert (np.abs(pose[l] - want) <= tol).all(), f'{what}: pose {l}: {pose[l]} vs {want}'


def _planted_scene(H, R, D, seed):
  rng = np.random.default_rng(seed)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  fq = torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV)
  fm = torch.roll(torch.rot90(fq, 2, (0, 1)), (2, -1), (0, 1)).contiguous()
  return grid, types.FeaturePlane(features=fq, valid=valid), types.FeaturePlane(features=fm, valid=valid)


def test_localize_exhaustive_recall():
  """[36, 63, 63] from a planted pose at 32^2 (the scene of the modes test): ``recall=`` reuses the peaks; the planted
  pose's ball holds the best mass; without the argument the keys and bits are what they were.  The votes are
  correlations per query cell: ~8 (the D = 8 channels' mean square) at the planted pose, ~N(0, 0.1^2) elsewhere, so at
  temperature 2 the planted cell weighs e^16 against at most 197 cells of e^1 in a ball that misses it: every best ball
  must hold it.  (At the modes test's temperature 0.05 the posterior is nearly flat and 197 background cells outweigh
  the peak: there the arg-max of the votes is NOT the pose of maximum expected recall.)"""
  H, R = 32, 36
  grid, pq, pm = _planted_scene(H, R, 8, seed=5)
  base = pev.localize_exhaustive(pq, pm, R, grid)
  assert set(base) == {'map_t_query', 'index', 'score', 'count', 'votes'}
  planted = base['index'][0].cpu().numpy()
  gt_tf = pev.exhaustive_index_to_tfm(base['index'][0].to(torch.float32) + torch.tensor([0.2, -0.3, 0.4], device=DEV),
                                      grid, R)
  temperature = 2.0
  with guarded.scope():
    out = pev.localize_exhaustive(pq, pm, R, grid, recall=dict(temperature=temperature, m_t_q_gt=gt_tf, maps=True))
    plain = pev.localize_exhaustive(pq, pm, R, grid, recall=True)
  assert set(out) == set(base) | {'recall'} and set(plain) == set(out)
  for k in ('votes', 'score', 'index', 'count'):
    assert guarded.same_bits(base[k], plain[k]) and guarded.same_bits(base[k], out[k]), k
  rec = out['recall']
  assert set(rec) == {'best_index', 'map_t_query', 'best_recall', 'thresholds_cells', 'log_z', 'count', 'peak_recall',
                      'gt_recall', 'maps'}
  assert set(plain['recall']) == set(rec) - {'gt_recall', 'maps'}
  assert rec['thresholds_cells'].tolist() == [[3, 0], [15, 0], [63, 0]]
  votes, peaks = out['votes'].cpu().numpy(), out['index'].cpu().numpy()
  gt_idx = pev.exhaustive_tfm_to_index(gt_tf, grid, R).to(torch.float32).cpu().numpy()
  want = ref.vote_recall(votes, (3, 15, 63), (0, 0, 0), peaks, temperature, gt_idx)
  slack = ref.float64_slack(votes.shape, want['log_z'], want['m'])
  _assert_log_mass(rec['maps'].cpu().numpy(), want['maps'], slack, 'localize maps')
  eps = 2.0 ** -24
  for key, w64 in (('peak_recall', want['centre']), ('gt_recall', want['gt'])):
    g, w = rec[key].cpu().numpy().astype(np.float64), np.exp(w64)
    # exp of an f32 log mass within 2 ulps (+ slack) of the reference's, rounded to f32 once more
    tol = w * (1.01 * (_ulps(ref.round_log_mass(w64)) + slack) + 2 * eps)
    assert (np.abs(g - w) <= tol).all(), f'{key}: {g} vs {w}'
  assert want['gt_cell'] == tuple(int(x) for x in planted) and int(rec['count'][2]) == 1
  best = rec['best_index'].cpu().numpy()
  for l, (q, h) in enumerate(rec['thresholds_cells'].tolist()):
    assert ref.ball_mask(votes.shape, planted, q, h)[tuple(best[l])], f'level {l}: {best[l]} vs planted {planted}'
  br = rec['best_recall'].cpu().numpy()
  assert (br > 0).all() and (br <= 1).all() and (np.diff(br) >= 0).all()
  assert (br + 1e-6 >= rec['peak_recall'].cpu().numpy().max(0)).all()
  _assert_poses(rec, grid, R, 'localize')
  _assert_poses(plain['recall'], grid, R, 'localize plain')


def test_vote_filter_recall():
  """``VoteFilter.recall`` works on the belief (log space, normalised: scale 1, log_z ~ 0)."""
  H, R = 32, 36
  grid = grids.Grid2D((H, H), 0.25)
  v = ref.smooth_votes((R, 2 * H - 1, 2 * H - 1), seed=4)
  f = pev.VoteFilter(grid, R, sigma_xy=0.3, sigma_yaw=0.1, temperature=2.0)
  with pytest.raises(ValueError):
    f.recall()
  f.step(torch.from_numpy(v).to(DEV))
  peaks = pev.poses_from_votes(f.belief, grid, R, num_peaks=8, radius_r=2, radius_xy=4)['index']
  with guarded.scope():
    out = f.recall(thresholds=((0.5, 1), (1.3, 25)), peaks=peaks)
  assert out['thresholds_cells'].tolist() == [[3, 0], [27, 2]] and abs(float(out['log_z'])) <= 1e-5
  belief = f.belief.cpu().numpy()
  want = ref.vote_recall(belief, (3, 27), (0, 2), peaks.cpu().numpy(), 1.0)
  slack = ref.float64_slack(belief.shape, want['log_z'], want['m'])
  g, w = out['peak_recall'].cpu().numpy().astype(np.float64), np.exp(want['centre'])
  tol = w * (1.01 * (_ulps(ref.round_log_mass(want['centre'])) + slack) + 2 * 2.0 ** -24)
  assert (np.abs(g - w) <= tol).all(), f'{g} vs {w}'
  assert 'gt_recall' not in out and 'maps' not in out
  _assert_poses(out, grid, R, 'filter')
  with pytest.raises(ValueError):
    pev.recall_from_votes(f.belief[:8], grid, R)
