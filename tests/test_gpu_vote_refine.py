"""`-m gpu`: ``ops.plane_align_score`` (vote_refine.hip, through the C ABI) and the host entry points built on it
(``pose_exhaustive_voting.refine_lattice`` / ``refine_poses`` / ``localize_exhaustive(refine=...)``), against the
float64 numpy restatement ``vote_refine_reference`` within twice its derived rounding bound; ``overlap`` and the -inf
set exactly.

The partial launch cuts the query plane into 16 x 16 cell tiles, 16 tiles per workgroup, one workgroup row per pose:
``tiny`` 1 x 1 in 3 x 3; ``ragged`` 5 x 7 in 9 x 6 with D = 12; ``tiles`` 33 x 17 (3 x 2 tiles, ragged last ones) with 70
poses; ``small_map`` 20 x 20 in 6 x 6; ``masks`` invalid cells on both sides, a zero-weight invalid tap, overlap equal to
/ one above the threshold; ``outside``; ``nonfinite_pose``; ``wide`` D = 128.  The host-level case (24 x 24, 4 peaks x
891 poses) and the voting comparison (16 x 16, D = 32) add planes of more than one tile per axis with whole tiles.
Every call runs under ``guarded.scope()``: guard regions intact (outputs and workspace), no output element left
unwritten, the workspace the size ``snap_plane_align_score_workspace_bytes`` states.

Observed on an MI355X (each case prints its figures), largest error / bound per case: ``tiny`` 0.034 (6.5e-8 against
2.4e-6), ``ragged`` 0.009, ``tiles`` 0.004, ``small_map`` 0.009, ``masks`` 0.004, ``nonfinite_pose`` 0.015, ``wide``
0.001 (8.2e-8 against 1.3e-4), the planted-pose lattices 0.055 (1.3e-7 against 2.8e-6); against the direct voting at
the convention poses the scores differ by at most 2.1e-7; 2 x the bound is allowed."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_refine_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c[0]: c[1:] for c in ref.all_inputs()}


@functools.lru_cache(maxsize=None)
def _want(name):
  case = _inputs()[name]
  return ref.plane_align_score(*case), ref.bound(*case)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(fq, vq, fm, vm, poses, thr):
  """One guarded call -> numpy (score, overlap)."""
  Hq, Wq, D = fq.shape
  Hm, Wm = fm.shape[:2]
  P = poses.shape[0]
  with guarded.scope() as sc:
    out = ops.plane_align_score(guarded.place(_dev(fq), 'value'), guarded.place(_dev(vq), 'address'),
                                guarded.place(_dev(fm), 'value'), guarded.place(_dev(vm), 'address'),
                                guarded.place(_dev(poses), 'address'), thr)
    assert [tuple(o.shape) for o in out] == [(P,), (P,)]
    assert [o.dtype for o in out] == [torch.float32, torch.int32]
    ws = [a for a in sc.allocations('plane_align_score') if a.dtype == torch.int64]
    assert len(ws) == 1
    assert ws[0].numel() * 8 == _lib.load().snap_plane_align_score_workspace_bytes(Hq, Wq, Hm, Wm, D, P)
    for o, what in zip(out, ('score', 'overlap')):
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  return res


def _assert_within(got, want, tol, what, factor=2.0):
  (g, go), (w, wo) = got, want
  assert go.tolist() == wo.tolist(), f'{what}: overlap {go.tolist()} != {wo.tolist()}'
  assert (np.isnan(g) == np.isnan(w)).all(), f'{what}: NaN poses differ'
  assert ((g == -np.inf) == (w == -np.inf)).all(), f'{what}: -inf poses differ'
  fin = np.isfinite(w)
  err = np.abs(g[fin].astype(np.float64) - w[fin])
  if fin.any():
    print(f'{what}: max err {err.max():.3e}, max bound {tol[fin].max():.3e}, '
          f'max err / bound {np.max(err / np.maximum(tol[fin], 1e-300)):.3f}')
  bad = ~(err <= factor * tol[fin])
  assert not bad.any(), f'{what}: {int(bad.sum())} poses outside {factor} x bound'


@pytest.mark.parametrize('name', ['tiny', 'ragged', 'tiles', 'small_map', 'masks', 'outside', 'nonfinite_pose', 'wide'])
def test_against_the_reference(name):
  want, tol = _want(name)
  _assert_within(_run(*_inputs()[name]), want, tol, name)
  w, wo = want
  if name == 'outside':
    assert (w == -np.inf).all() and (wo == 0).all()
  if name == 'nonfinite_pose':
    assert (w[[1, 3]] == -np.inf).all() and np.isfinite(w[[0, 2, 4]]).all()
  if name == 'masks':
    thr = _inputs()[name][5]
    assert wo[1] == thr and w[1] == -np.inf and wo[2] == thr + 1 and np.isfinite(w[2])
  if name not in ('outside',):
    assert np.isfinite(w).any()


def test_integer_poses_on_integer_features_are_exact():
  case = ref.exact_case()
  want, wo = ref.plane_align_score(*case)
  g, go = _run(*case)
  assert go.tolist() == wo.tolist() and np.isfinite(want).all() and (wo > 0).all()
  assert (g.view(np.int32) == (want.astype(F32) + F32(0)).view(np.int32)).all()


def test_a_nan_map_feature_reaches_exactly_the_poses_that_tap_it():
  fq, vq, fm, vm, poses, thr = _inputs()['tiles']
  taps = ref.counted_taps(fq, vq, fm, vm, poses)
  Wm = fm.shape[1]
  hits = {}
  for cell in range(fm.shape[0] * Wm):
    n = sum(cell in t for t in taps)
    if 0 < n < len(taps) // 2 and vm.reshape(-1)[cell]:
      hits = {p for p, t in enumerate(taps) if cell in t}
      break
  assert hits
  clean, _ = _run(fq, vq, fm, vm, poses, thr)
  fm2 = fm.copy()
  fm2[cell // Wm, cell % Wm, 5] = np.nan
  want, _ = ref.plane_align_score(fq, vq, fm2, vm, poses, thr)
  g, _ = _run(fq, vq, fm2, vm, poses, thr)
  expect_nan = np.array([p in hits for p in range(len(poses))]) & (want != -np.inf)
  assert expect_nan.any() and (np.isnan(want) == expect_nan).all()
  assert (np.isnan(g) == expect_nan).all()
  assert (g.view(np.int32)[~expect_nan] == clean.view(np.int32)[~expect_nan]).all()


def test_two_calls_and_any_grouping_of_the_poses_give_identical_bits():
  fq, vq, fm, vm, poses, thr = _inputs()['tiles']
  args = [_dev(a) for a in (fq, vq, fm, vm)]
  first = ops.plane_align_score(*args, _dev(poses), thr)
  torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
  second = ops.plane_align_score(*args, _dev(poses), thr)
  for a, b in zip(first, second):
    assert guarded.same_bits(a, b)
  perm = np.random.default_rng(3).permutation(len(poses))
  moved = ops.plane_align_score(*args, _dev(poses[perm]), thr)
  for a, b in zip(first, moved):
    assert guarded.same_bits(a[torch.from_numpy(perm).to(DEV)], b)
  for lo, hi in ((0, 1), (5, 18), (37, 70)):                  # other pose counts, other neighbours
    part = ops.plane_align_score(*args, _dev(poses[lo:hi]), thr)
    for a, b in zip(first, part):
      assert guarded.same_bits(a[lo:hi], b)
  # garbage in the workspace changes nothing
  lib = _lib.load()
  Hq, Wq, D = fq.shape
  Hm, Wm = fm.shape[:2]
  P = len(poses)
  nbytes = lib.snap_plane_align_score_workspace_bytes(Hq, Wq, Hm, Wm, D, P)
  ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  pd = _dev(poses)
  for fill in (-1, 0x3ff0000000000000):
    ws.fill_(fill)
    o = (torch.empty((P,), device=DEV), torch.empty((P,), dtype=torch.int32, device=DEV))
    st = lib.snap_plane_align_score_f32(p(args[0]), p(args[1]), p(args[2]), p(args[3]), p(pd), Hq, Wq, Hm, Wm, D, P,
                                        thr, p(o[0]), p(o[1]), p(ws), nbytes,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    for a, b in zip(first, o):
      assert guarded.same_bits(a, b)


def test_against_the_exhaustive_voting_at_the_convention_poses():
  """votes[k, H - 1, W - 1] of the direct form is the score of the continuous index (k, H - 1.5, W - 1.5) at whole
  quarter turns (the templates are exact permutations there).  The vote's bound: one product, at most H W D additions
  in whatever order the f32 engine takes them, one division: gamma_(H W D + 2) * sum |q| |m| / tcount."""
  H, D, R = 16, 32, 8
  rng = np.random.default_rng(21)
  fq = rng.standard_normal((H, H, D)).astype(F32)
  fm = rng.standard_normal((H, H, D)).astype(F32)
  ones = np.ones((H, H), bool)
  grid = grids.Grid2D((H, H), 0.25)
  with ops.engine_scope('f32'):
    votes = pev.exhaustive_pose_voting(types.FeaturePlane(features=_dev(fq), valid=_dev(ones)),
                                       types.FeaturePlane(features=_dev(fm), valid=_dev(ones)), R, grid,
                                       method='direct').cpu().numpy()
  ks = [0, R // 4, R // 2, 3 * R // 4]
  index = torch.tensor([[k, H - 1, H - 1] for k in ks], dtype=torch.int32)
  cont, poses = pev.refine_lattice(index, grid, R, (H, H), steps_r=1, range_r=0.0, steps_xy=1, range_xy=0.0)
  # the one-point lattice sits on the integer index; the convention pose is half a cell below it
  poses = poses.numpy().copy()
  poses[:, 2:] -= F32(0.5)
  want = ref.index_to_pose(np.array([[k, H - 1.5, H - 1.5] for k in ks]), (H, H), R)
  assert np.array_equal(poses[:, :2], np.round(want[:, :2]).astype(F32)) and np.allclose(poses[:, 2:], want[:, 2:])
  g, go = _run(fq, ones, fm, ones, poses, 0.0)
  w, wo = ref.plane_align_score(fq, ones, fm, ones, poses, 0.0)
  tol = ref.bound(fq, ones, fm, ones, poses, 0.0)
  assert go.tolist() == [H * H] * 4 == wo.tolist()
  n = H * H * D + 2
  s_abs = ref._walk(fq, ones, fm, ones, poses, 'bound')[0]
  tol_vote = n * ref.U / (1 - n * ref.U) * s_abs
  for i, k in enumerate(ks):
    v = float(votes[k, H - 1, H - 1])
    print(f'k={k}: score {g[i]!r} vote {v!r} reference {w[i]!r}; bounds {tol[i]:.2e} + {tol_vote[i]:.2e}')
    assert abs(float(g[i]) - w[i]) <= 2 * tol[i]
    assert abs(float(g[i]) - v) <= tol[i] + tol_vote[i]


def _planted():
  case = ref.planted_case()
  grid = grids.Grid2D(case['extent'], case['cell_size'])
  pq = types.FeaturePlane(features=_dev(case['fq']), valid=_dev(case['vq']))
  pm = types.FeaturePlane(features=_dev(case['fm']), valid=_dev(case['vm']))
  return case, grid, pq, pm


def test_localize_exhaustive_refines_its_peaks_on_the_planted_pose():
  case, grid, pq, pm = _planted()
  R, H, K = case['R'], case['extent'][0], 4
  with guarded.scope():
    out = pev.localize_exhaustive(pq, pm, R, grid, refine=True, num_peaks=K)
  assert set(out) == {'map_t_query', 'index', 'score', 'count', 'votes', 'refined'}
  fine = out['refined']
  assert set(fine) == {'index', 'score', 'overlap', 'map_t_query', 'lattice_scores'}
  assert tuple(fine['lattice_scores'].shape) == (K, 11, 9, 9) and fine['overlap'].dtype == torch.int32
  assert int(out['count'][0]) >= K
  cont, poses = pev.refine_lattice(out['index'], grid, R, (H, H))
  assert cont.device == out['index'].device
  L = cont.shape[1]
  cont, poses = cont.cpu().numpy(), poses.cpu().numpy().reshape(K, L, 4)
  thr = 0.05 * H * H
  for k in range(K):
    args = (case['fq'], case['vq'], case['fm'], case['vm'], poses[k], thr)
    w, wo = ref.plane_align_score(*args)
    tol = ref.bound(*args)
    lat = fine['lattice_scores'][k].reshape(-1).cpu().numpy()
    _assert_within((lat, np.zeros(0)), (w, np.zeros(0)), tol, f'planted peak {k}')
    best = int(np.argmax(lat))                       # the first maximum
    top = int(np.argmax(w))
    print(f'peak {k}: lattice argmax {best} (reference {top}), reference score there {w[best]:.9f} against its '
          f'maximum {w[top]:.9f}, bound {max(tol[best], tol[top]):.2e}')
    assert w[top] - w[best] <= 2 * max(tol[best], tol[top])
    assert float(fine['score'][k]) == float(lat[best]) and int(fine['overlap'][k]) == int(wo[best])
    assert np.array_equal(fine['index'][k].cpu().numpy(), cont[k, best])
    want = ref.index_to_pose(cont[k, best].astype(np.float64), (H, H), R)
    mtq = fine['map_t_query'][k]
    assert abs(float(mtq.angle) + 2 * math.pi * float(cont[k, best, 0]) / R) < 1e-6
    assert np.abs(mtq.t.cpu().numpy() - want[2:] * case['cell_size']).max() < 1e-5
  # the best peak, refined, is closer to the planted pose than the peak itself
  e0 = abs(float(out['map_t_query'][0].angle) - case['angle_true'])
  e1 = abs(float(fine['map_t_query'][0].angle) - case['angle_true'])
  print(f'yaw error {math.degrees(e0):.3f} deg -> {math.degrees(e1):.3f} deg')
  assert e1 < e0
  # lattice keywords pass through
  small = pev.localize_exhaustive(pq, pm, R, grid, num_peaks=2, refine=dict(steps_r=3, range_r=0.25, steps_xy=5,
                                                                             min_overlap=0.1))
  assert tuple(small['refined']['lattice_scores'].shape) == (2, 3, 5, 5)
  with pytest.raises(TypeError):
    pev.localize_exhaustive(pq, pm, R, grid, num_peaks=2, refine=dict(steps=3))


def test_without_refine_the_result_is_the_parents_key_for_key():
  case, grid, pq, pm = _planted()
  R = case['R']
  votes = pev.exhaustive_pose_voting(pq, pm, R, grid)
  peaks = pev.poses_from_votes(votes, grid, R, num_peaks=4)
  for refine in (None, False):
    out = pev.localize_exhaustive(pq, pm, R, grid, num_peaks=4, refine=refine)
    assert set(out) == {'map_t_query', 'index', 'score', 'count', 'votes'}
    assert guarded.same_bits(out['votes'], votes)
    for key in ('index', 'score', 'count'):
      assert guarded.same_bits(out[key], peaks[key]), key
    assert guarded.same_bits(out['map_t_query'].angle, peaks['map_t_query'].angle)
    assert guarded.same_bits(out['map_t_query'].t, peaks['map_t_query'].t)


def test_fewer_peaks_than_asked_for_give_empty_rows():
  H, D, R, K = 8, 4, 4, 64
  rng = np.random.default_rng(8)
  grid = grids.Grid2D((H, H), 0.5)
  ones = _dev(np.ones((H, H), bool))
  pq = types.FeaturePlane(features=_dev(rng.standard_normal((H, H, D)).astype(F32)), valid=ones)
  pm = types.FeaturePlane(features=_dev(rng.standard_normal((H, H, D)).astype(F32)), valid=ones)
  with guarded.scope():
    out = pev.localize_exhaustive(pq, pm, R, grid, num_peaks=K, radius_xy=4, refine=dict(steps_r=3, steps_xy=3))
  found = int(out['count'][0])
  assert 1 <= found < K
  fine = out['refined']
  assert bool(torch.isfinite(fine['score'][:found]).all()) and bool((fine['score'][found:] == -math.inf).all())
  assert bool((fine['overlap'][found:] == 0).all()) and bool(torch.isnan(fine['index'][found:]).all())
  assert bool(torch.isnan(fine['map_t_query'].angle[found:]).all())
  assert bool(torch.isnan(fine['map_t_query'].t[found:]).all())
  assert not bool(torch.isnan(fine['map_t_query'].t[:found]).any())
  assert bool((fine['lattice_scores'][found:] == -math.inf).all())


def test_bad_arguments_raise_without_launching():
  fq = torch.zeros((5, 6, 8), device=DEV)
  fm = torch.zeros((7, 4, 8), device=DEV)
  vq = torch.ones((5, 6), dtype=torch.bool, device=DEV)
  vm = torch.ones((7, 4), dtype=torch.bool, device=DEV)
  poses = torch.zeros((3, 4), device=DEV)
  bad = [
      (fq[..., :6].contiguous(), vq, fm[..., :6].contiguous(), vm, poses),     # D % 4
      (fq, vq, fm[..., :4].contiguous(), vm, poses),                           # D differs
      (fq, vq[:4], fm, vm, poses), (fq, vq, fm, vm.float(), poses), (fq, vq, fm, vm, poses[:, :3]),
      (fq, vq, fm, vm, poses.double()), (fq, vq, fm, vm, poses.cpu()), (fq, vq, fm, vm, poses[:0]),
      (fq[0], vq, fm, vm, poses), (torch.zeros((5, 6, 132), device=DEV), vq, torch.zeros((7, 4, 132), device=DEV), vm, poses),
  ]
  for args in bad:
    with pytest.raises(ValueError):
      ops.plane_align_score(*args, 0.0)
  with pytest.raises(ValueError):
    ops.plane_align_score(fq, vq, fm, vm, poses, float('nan'))
  lib = _lib.load()
  wsb = lib.snap_plane_align_score_workspace_bytes
  assert wsb(5, 6, 7, 4, 6, 3) == 0 and wsb(5, 6, 7, 4, 132, 3) == 0 and wsb(5, 6, 7, 4, 0, 3) == 0
  assert wsb(0, 6, 7, 4, 8, 3) == 0 and wsb(5, 1025, 7, 4, 8, 3) == 0 and wsb(5, 6, 7, 1025, 8, 3) == 0
  assert wsb(5, 6, 7, 4, 8, 0) == 0 and wsb(5, 6, 7, 4, 8, 1 << 20) == 0
  assert wsb(1024, 1024, 1024, 1024, 128, (1 << 20) - 1) == ((1 << 20) - 1) * 256 * 16 + 8
  need = wsb(5, 6, 7, 4, 8, 3)
  assert need == 3 * 1 * 16 + 8                                                   # one workgroup per pose, and tcount
  ws = torch.empty(need // 8, dtype=torch.int64, device=DEV)
  score = torch.full((3,), 7.0, device=DEV)
  overlap = torch.full((3,), 7, dtype=torch.int32, device=DEV)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  call = lambda D, P, nbytes, pp=p(poses): lib.snap_plane_align_score_f32(
      p(fq), p(vq), p(fm), p(vm), pp, 5, 6, 7, 4, D, P, 0.0, p(score), p(overlap), p(ws), nbytes, None)
  assert call(6, 3, need) == -2 and call(8, 0, need) == -2 and call(8, 1 << 20, 1 << 40) == -2
  assert call(8, 3, need - 1) == -5 and call(8, 3, need, None) == -3
  torch.cuda.synchronize()
  assert bool((score == 7).all()) and bool((overlap == 7).all())                  # nothing ran
