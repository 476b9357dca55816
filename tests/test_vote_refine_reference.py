"""CPU pins of ``vote_refine_reference`` (the float64 restatement the GPU tests compare ``ops.plane_align_score``
with) to things that are not the reference: ``scipy.ndimage.map_coordinates`` and the oracle's ``interpolate_nd`` for
the sample, the oracle's exhaustive voting for the pose convention, the host lattice of ``pose_exhaustive_voting``, and
a planted off-lattice pose for the refinement as a whole."""
import math

import numpy as np
import pytest
import scipy.ndimage
import torch

import vote_refine_reference as ref
from oracle import grids as o_grids
from oracle import voting as o_voting
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids

F32 = np.float32


def test_the_sample_is_map_coordinates_and_the_oracle_validity_rule():
  rng = np.random.default_rng(3)
  Hq, Wq, Hm, Wm, D = 6, 5, 7, 9, 3 * 4
  fq = np.zeros((Hq, Wq, D), F32)
  fm = rng.standard_normal((Hm, Wm, D)).astype(F32)
  vm = rng.random((Hm, Wm)) > 0.2
  vq = np.ones((Hq, Wq), bool)
  for pose in (ref.pose_row(0, 1, 2, True), ref.pose_row(25.0, 2.3, 1.1), ref.pose_row(-100.0, 0.4, 7.9),
               ref.pose_row(1, 6, 0, True)):
    g = ref._geometry(pose, Hq, Wq, Hm, Wm)
    c, s, tx, ty = (F32(x) for x in pose)
    gi = (np.arange(Hq, dtype=F32) + F32(0.5))[:, None]
    gj = (np.arange(Wq, dtype=F32) + F32(0.5))[None, :]
    u = ((c * gi - s * gj) + tx).astype(F32)
    v = ((s * gi + c * gj) + ty).astype(F32)
    points = np.stack([u, v], -1).reshape(-1, 2).astype(np.float64)
    values, valid = o_grids.interpolate_nd(fm.astype(np.float64), points, vm)
    counted = vq & g['inside'] & vm[g['i0'], g['j0']] & vm[g['i0'], g['j1']] & vm[g['i1'], g['j0']] & \
        vm[g['i1'], g['j1']]
    assert np.array_equal(counted.reshape(-1), valid)
    assert counted.any()
    wu1, wv1 = g['wu1'][..., None], g['wv1'][..., None]
    f = fm.astype(np.float64)
    mix = ((1 - wu1) * (1 - wv1)) * f[g['i0'], g['j0']] + ((1 - wu1) * wv1) * f[g['i0'], g['j1']] + \
        (wu1 * (1 - wv1)) * f[g['i1'], g['j0']] + (wu1 * wv1) * f[g['i1'], g['j1']]
    coords = np.stack([u.astype(np.float64) - 0.5, v.astype(np.float64) - 0.5]).reshape(2, -1)
    for d in range(D):
      want = scipy.ndimage.map_coordinates(f[..., d], coords, order=1, mode='nearest').reshape(Hq, Wq)
      # (fl32(u - 0.5) against the float64 u - 0.5: 2^-25 of a cell at most, times the feature's slope)
      assert np.abs(mix[..., d] - want)[g['inside']].max() < 1e-6
    # and the score is the sum of it
    fq[:] = rng.standard_normal(fq.shape)
    score, overlap = ref.plane_align_score(fq, vq, fm, vm, pose[None], 0.0)
    assert overlap[0] == counted.sum()
    np.testing.assert_allclose(score[0], (fq.astype(np.float64) * mix).sum(-1)[counted].sum() / vq.sum(), rtol=1e-13)


def test_convention_against_the_oracle_voting():
  """The pose of the continuous index (k, H - 1.5, W - 1.5) is the placement the oracle's votes[k, H - 1, W - 1]
  scores: the zero shift of the correlation sits HALF A CELL below the integer index of ``exhaustive_index_to_tfm``."""
  H, D, R = 8, 4, 8
  rng = np.random.default_rng(11)
  fq = rng.standard_normal((H, H, D))
  fm = rng.standard_normal((H, H, D))
  ones = np.ones((H, H), bool)
  grid = o_grids.Grid2D((H, H), 0.5)
  votes = o_voting.exhaustive_pose_voting(dict(features=fq, valid=ones), dict(features=fm, valid=ones), R, grid)
  assert votes.dtype == np.float64 and votes.shape == (R, 2 * H - 1, 2 * H - 1)
  for k in (0, R // 4, R // 2, 3 * R // 4):
    pose = ref.index_to_pose(np.array([k, H - 1.5, H - 1.5]), (H, H), R)
    pose[:2] = np.round(pose[:2])                     # whole quarter turns: exact (+-1, 0) pairs
    # the features are rounded to f32 for the reference (its input type) and for the oracle alike
    f32q, f32m = fq.astype(F32), fm.astype(F32)
    v32 = o_voting.exhaustive_pose_voting(dict(features=f32q.astype(np.float64), valid=ones),
                                          dict(features=f32m.astype(np.float64), valid=ones), R, grid)
    score, overlap = ref.plane_align_score(f32q, ones, f32m, ones, pose.astype(F32)[None], 0.0)
    assert overlap[0] == H * H
    want = v32[k, H - 1, H - 1]
    print(f'k={k}: reference {score[0]!r} oracle {want!r}')
    assert abs(score[0] - want) <= 1e-12 * abs(want)


def _ulp_diff(a, b):
  a, b = np.asarray(a, F32), np.asarray(b, F32)
  ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
  ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
  return np.abs(ia - ib)


@pytest.mark.parametrize('R,H,lattice', [(36, 24, {}), (8, 16, dict(steps_r=5, range_r=0.25, steps_xy=3, range_xy=0.5))])
def test_the_host_lattice_is_the_float64_lattice(R, H, lattice):
  grid = grids.Grid2D((H, H), 0.2)
  index = np.array([[0, H - 1, H - 1], [R // 4, 3, 2 * H - 2], [-1, -1, -1], [R - 1, 2 * H - 2, 0], [5, 17, 9]],
                   np.int32)
  cont, poses = pev.refine_lattice(torch.tensor(index), grid, R, (H, H), **lattice)
  want_c, want_p = ref.refine_lattice(index, (H, H), R, **lattice)
  L = want_c.shape[1]
  assert cont.dtype == torch.float32 and poses.dtype == torch.float32
  assert tuple(cont.shape) == (5, L, 3) and tuple(poses.shape) == (5 * L, 4)
  cont, poses = cont.numpy(), poses.numpy().reshape(5, L, 4)
  want_p = want_p.reshape(5, L, 4)
  assert np.isnan(cont[2]).all() and np.isnan(poses[2]).all()
  keep = [0, 1, 3, 4]
  assert np.array_equal(cont[keep], want_c[keep].astype(F32))          # sums of small exact numbers
  # cos / sin: within 1 ulp of the f32 rounding, or (near a zero of cos / sin) within the float64 noise of the two routes
  d = _ulp_diff(poses[keep], want_p[keep].astype(F32))
  near = np.abs(poses[keep].astype(np.float64) - want_p[keep]) < 1e-14
  assert ((d <= 1) | near).all(), int(d.max())
  # the lattice order: rotation slowest, then a, then b
  sr, sxy = lattice.get('steps_r', 11), lattice.get('steps_xy', 9)
  c4 = cont[0].reshape(sr, sxy, sxy, 3)
  assert (np.diff(c4[:, 0, 0, 0]) > 0).all() and (np.diff(c4[0, :, 0, 1]) > 0).all() and (np.diff(c4[0, 0, :, 2]) > 0).all()
  # whole quarter turns are exact
  mid = (sr // 2) * sxy * sxy
  assert poses[0, mid, :2].tolist() == [1.0, 0.0] and poses[1, mid, :2].tolist() == [0.0, -1.0]
  with pytest.raises(ValueError):
    pev.refine_lattice(torch.tensor(index), grid, R, (H, H + 1))
  with pytest.raises(ValueError):
    pev.refine_lattice(torch.tensor(index[:, :2]), grid, R, (H, H))


def test_refinement_beats_the_lattice_peak_on_a_planted_pose():
  case = ref.planted_case()
  H, R, cell = case['extent'][0], case['R'], case['cell_size']
  grid = o_grids.Grid2D(case['extent'], cell)
  votes = o_voting.exhaustive_pose_voting(
      dict(features=case['fq'].astype(np.float64), valid=case['vq']),
      dict(features=case['fm'].astype(np.float64), valid=case['vm']), R, grid)
  peak = np.array(np.unravel_index(int(np.argmax(votes)), votes.shape))
  coarse = ref.index_to_pose(peak.astype(np.float64), case['extent'], R)
  fine = ref.refine_poses(case['fq'], case['vq'], case['fm'], case['vm'], peak[None].astype(np.int32), case['extent'],
                          R, cell)

  def yaw_err(angle):
    return abs((angle - case['angle_true'] + math.pi) % (2 * math.pi) - math.pi)

  e_yaw0 = math.degrees(yaw_err(-2 * math.pi * peak[0] / R))
  e_yaw1 = math.degrees(yaw_err(fine['angle'][0]))
  # a translation depends on the frame it is read in; the error that matters is where the query plane's centre lands
  centre = np.array(case['extent']) / 2

  def centre_of(pose):
    c, s, tx, ty = pose
    return np.array([c * centre[0] - s * centre[1] + tx, s * centre[0] + c * centre[1] + ty]) * cell

  best_pose = ref.index_to_pose(fine['index'][0], case['extent'], R)
  e_t0 = float(np.linalg.norm(centre_of(coarse) - centre_of(case['pose_true'])))
  e_t1 = float(np.linalg.norm(centre_of(best_pose) - centre_of(case['pose_true'])))
  print(f'peak {peak.tolist()} true index {case["index_true"].tolist()} refined index {fine["index"][0].tolist()}')
  print(f'yaw error: peak {e_yaw0:.3f} deg -> refined {e_yaw1:.3f} deg; '
        f'translation error: peak {e_t0:.4f} m -> refined {e_t1:.4f} m; score {fine["score"][0]:.6f} '
        f'against the vote {votes.max():.6f}')
  assert e_yaw1 < e_yaw0 and e_t1 < e_t0


def test_masks_thresholds_and_non_finite_inputs_by_hand():
  cases = {c[0]: c[1:] for c in ref.all_inputs()}
  fq, vq, fm, vm, poses, thr = cases['masks']
  score, overlap = ref.plane_align_score(fq, vq, fm, vm, poses, thr)
  assert overlap[1] == thr and score[1] == -np.inf and overlap[2] == thr + 1 and np.isfinite(score[2])
  # the zero-weight tap: validating map cell (7, 6) gives pose 0 exactly its three neighbours back, and their value
  # does not involve the cell's features
  vm2 = vm.copy()
  vm2[7, 6] = True
  s2, o2 = ref.plane_align_score(fq, vq, fm, vm2, poses[:1], -1.0)
  assert o2[0] == overlap[0] + 3
  fm2 = fm.copy()
  fm2[7, 6] = 1e3
  assert ref.plane_align_score(fq, vq, fm2, vm2, poses[:1], -1.0)[0][0] == s2[0]
  fq, vq, fm, vm, poses, thr = cases['outside']
  score, overlap = ref.plane_align_score(fq, vq, fm, vm, poses, thr)
  assert (score == -np.inf).all() and (overlap == 0).all()
  fq, vq, fm, vm, poses, thr = cases['nonfinite_pose']
  score, overlap = ref.plane_align_score(fq, vq, fm, vm, poses, thr)
  assert (score[[1, 3]] == -np.inf).all() and (overlap[[1, 3]] == 0).all() and np.isfinite(score[[0, 2, 4]]).all()
  # exact case: the scores are multiples of 1 / 64
  fq, vq, fm, vm, poses, thr = ref.exact_case()
  score, overlap = ref.plane_align_score(fq, vq, fm, vm, poses, thr)
  assert (overlap > 0).all() and np.array_equal(score * 64, np.round(score * 64))
  assert (ref.bound(fq, vq, fm, vm, poses, thr) > 0).all()
