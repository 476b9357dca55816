"""CPU pins of ``vote_fuse_reference`` (the float64 restatement the GPU tests compare ``ops.vote_fuse`` with) to
things that are not the reference: the identity, ``np.roll`` / slices for integer shifts, the long way round through
the host index <-> transform helpers for the shift table, a localisation property, hand-written masking cases."""
import math

import numpy as np
import pytest
import torch

import vote_fuse_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids


def test_one_frame_with_zero_shifts_is_the_input():
  rng = np.random.default_rng(0)
  v = rng.standard_normal((1, 4, 7, 9)).astype(np.float32)
  v[0, 1, 2, 3] = -np.inf
  out, count = ref.vote_fuse(v, np.zeros((1, 4, 3), np.float32))
  assert np.array_equal(out, v[0].astype(np.float64))
  assert count.tolist() == [4 * 7 * 9 - 1, 0]
  assert (ref.bound(v, np.zeros((1, 4, 3), np.float32)) <= 14 * 2.0 ** -24 * np.abs(np.where(np.isfinite(v[0]), v[0], 0)) * 1.001).all()


def test_integer_shifts_are_roll_and_slices():
  rng = np.random.default_rng(1)
  N, R, Ho, Wo = 3, 6, 8, 10
  v = rng.standard_normal((N, R, Ho, Wo)).astype(np.float32)
  w = np.array([1.0, -0.5, 2.0], np.float32)
  s = np.zeros((N, R, 3), np.float32)
  s[1, :, 0], s[2, :, 0] = 2, -7
  s[1, :, 1:] = rng.integers(-3, 4, (R, 2))
  s[2, :, 1:] = rng.integers(-3, 4, (R, 2))
  want = np.zeros((R, Ho, Wo))
  outside = np.zeros((R, Ho, Wo), bool)
  for n in range(N):
    for r in range(R):
      dk, da, db = (int(x) for x in s[n, r])
      plane = np.roll(v[n].astype(np.float64), -dk, axis=0)[r]         # plane[r] = v[n, (r + dk) mod R]
      moved = np.full((Ho, Wo), -np.inf)
      a0, a1 = max(0, -da), min(Ho, Ho - da)
      b0, b1 = max(0, -db), min(Wo, Wo - db)
      moved[a0:a1, b0:b1] = plane[a0 + da:a1 + da, b0 + db:b1 + db]    # moved[a, b] = plane[a + da, b + db]
      outside[r] |= moved == -np.inf
      want[r] += float(w[n]) * np.where(moved == -np.inf, 0.0, moved)
  want[outside] = -np.inf
  out, count = ref.vote_fuse(v, s, w)
  assert np.array_equal(out, want)
  assert count.tolist() == [int(np.isfinite(want).sum()), 0]
  assert (want == -np.inf).any()


GEOMETRIES = [
    # extent, cell size, R, relative poses (angle, tx, ty); extent * cell / 2 is exact in f32 everywhere
    ((8, 8), 0.25, 4, [(0.0, 0.0, 0.0), (0.3, 0.4, -0.7), (math.pi / 2, -0.5, 0.25)]),
    ((6, 10), 0.5, 36, [(0.0, 0.0, 0.0), (0.0873, 1.0, 0.1), (-1.234, -0.8, 2.2), (2 * math.pi / 36, 0.0, 0.0)]),
    ((12, 12), 0.5, 36, [(-0.05, 0.3, 0.3), (3.0, 2.5, -1.5)]),
]


@pytest.mark.parametrize('extent,cell,R,rel', GEOMETRIES, ids=['R4', 'R36_nonsquare', 'R36'])
def test_shift_table_is_the_long_way_round(extent, cell, R, rel):
  grid = grids.Grid2D(extent, cell)
  rel = np.array(rel)
  closed = ref.shift_table(rel[:, 0], rel[:, 1:], extent, cell, R)            # [N, R, 3]
  cells, general = ref.shift_table_general(rel[:, 0], rel[:, 1:], grid, R)    # every cell of the volume
  assert len(cells) == R * (2 * extent[0] - 1) * (2 * extent[1] - 1)
  want = closed[:, cells[:, 0].astype(int), :]                                # [N, M, 3]
  d = np.abs(general - want)
  d[..., 0] = np.minimum(d[..., 0], R - d[..., 0])
  print(f'{extent} R={R}: max |closed - general| = {d.max():.3e} cells')
  assert d.max() < 1e-9
  # the host entry point: the same table, rounded to f32 once, dk in [0, R), identity -> zeros
  q0_t_q = geometry.Transform2D(torch.tensor(rel[:, 0]), torch.tensor(rel[:, 1:]))
  tab = pev.sequence_shift_table(q0_t_q, grid, R)
  assert tab.dtype == torch.float32 and tuple(tab.shape) == (len(rel), R, 3)
  got = tab.numpy()
  assert (got[..., 0] >= 0).all() and (got[..., 0] < R).all()
  want32 = ref.shift_table_f32(rel[:, 0], rel[:, 1:], extent, cell, R)
  dk = np.abs(got[..., 0].astype(np.float64) - want32[..., 0])
  assert np.minimum(dk, R - dk).max() <= 4 * np.spacing(np.float32(R))
  assert np.abs(got[..., 1:] - want32[..., 1:]).max() <= 4 * np.spacing(np.float32(np.abs(want32[..., 1:]).max()))
  for n in np.flatnonzero((rel == 0).all(1)):
    assert not got[n].any() and not np.signbit(got[n]).any()


def test_index_to_tfm_f64_is_the_helper_without_its_casts():
  grid = grids.Grid2D((6, 10), 0.5)
  for idx in ((0.0, 0.0, 0.0), (7.0, 3.0, 18.0), (35.0, 10.0, 0.0), (12.5, 4.25, 9.75)):
    a = ref.index_to_tfm_f64(np.array(idx), grid, 36)
    b = pev.exhaustive_index_to_tfm(torch.tensor(idx, dtype=torch.float64), grid, 36)
    assert abs(float(a.angle) - float(b.angle)) < 1e-6 and float((a.t - b.t).abs().max()) < 1e-5


def test_a_yaw_just_above_zero_wraps_to_zero():
  grid = grids.Grid2D((8, 8), 0.25)
  tab = pev.sequence_shift_table(geometry.Transform2D(torch.tensor([1e-12]), torch.zeros(1, 2)), grid, 8)
  assert float(tab[0, 0, 0]) == 0.0 and (tab[..., 0] < 8).all()


def test_fusion_localises_where_single_frames_cannot():
  """Every frame holds the true bump and an equally high decoy; the decoys sit on whole cells (sampled height
  exactly 0) and move inconsistently with the motion.  Each frame's own argmax is tied or wrong; the fused argmax
  is the anchor's true index."""
  vols, angle, t, extent, cell, index0 = ref.bump_sequence()
  R = vols.shape[1]
  tab = ref.shift_table_f32(angle, t, extent, cell, R)
  for n in range(len(vols)):
    true_n = np.round(np.array(index0) + tab[n, index0[0]]).astype(int)
    true_n[0] %= R
    best = np.argwhere(vols[n] == vols[n].max())
    ambiguous = len(best) > 1
    wrong = not (best[0] == true_n).all()
    print(f'frame {n}: argmax {best.tolist()}, true {true_n.tolist()}')
    assert ambiguous or wrong
  fused, count = ref.vote_fuse(vols, tab)
  assert count[1] == 0 and count[0] > 0
  peak = np.unravel_index(np.argmax(np.where(np.isfinite(fused), fused, -np.inf)), fused.shape)
  assert tuple(int(i) for i in peak) == tuple(index0)
  runner = np.sort(fused[np.isfinite(fused)])[-2]
  assert fused[peak] > -0.5 and fused[peak] - runner > 0.05


def test_masking_and_nan_precedence():
  v = np.zeros((2, 2, 3, 3), np.float32)
  v[0] = 1.0
  v[1] = 10.0
  s = np.zeros((2, 2, 3), np.float32)
  s[1, :, 1] = 1.0                     # frame 1 reads row a + 1: the last output row is out of range
  # plain
  out, count = ref.vote_fuse(v, s)
  assert (out[:, :2] == 11).all() and (out[:, 2] == -np.inf).all() and count.tolist() == [12, 0]
  # a -inf tap of one frame masks the cell; a zero frame weight does not lift it
  v1 = v.copy()
  v1[1, 0, 1, 1] = -np.inf
  for w in (None, np.array([1.0, 0.0], np.float32)):
    out, count = ref.vote_fuse(v1, s, w)
    assert out[0, 0, 1] == -np.inf and count.tolist() == [11, 0]
    assert out[0, 1, 1] == (11 if w is None else 1)
  # NaN and +inf taps give NaN, also where another frame is out of range (row 2) or masked
  v2 = v.copy()
  v2[0, 1, 2, 0] = np.nan              # read by frame 0 at (1, 2, 0), where frame 1 is out of range
  v2[0, 0, 0, 2] = np.inf
  v2[1, 0, 1, 2] = -np.inf             # frame 1's tap at output (0, 0, 2)
  out, count = ref.vote_fuse(v2, s)
  assert np.isnan(out[1, 2, 0]) and np.isnan(out[0, 0, 2]) and count.tolist() == [11, 2]
  # a tap of weight zero is not read: the NaN in the upper k plane is invisible to an integer shift ...
  v3 = v.copy()
  v3[1, 1] = np.nan
  s3 = np.zeros((2, 2, 3), np.float32)
  out, count = ref.vote_fuse(v3, s3)
  assert (out[0] == 11).all() and np.isnan(out[1]).all() and count.tolist() == [9, 9]
  # ... and visible to a fractional one, from both rotations (circular)
  s3[1, :, 0] = 0.5
  out, count = ref.vote_fuse(v3, s3)
  assert np.isnan(out).all() and count.tolist() == [0, 18]
  # a' = Ho - 1 exactly is inside; any fraction above it is not
  s4 = np.zeros((1, 1, 3), np.float32)
  v4 = np.arange(9, dtype=np.float32).reshape(1, 1, 3, 3)
  s4[0, 0, 1] = 2.0
  out, _ = ref.vote_fuse(v4, s4)
  assert out[0, 0].tolist() == [6, 7, 8] and (out[0, 1:] == -np.inf).all()
  s4[0, 0, 1] = 1.5
  out, _ = ref.vote_fuse(v4, s4)
  assert out[0, 0].tolist() == [4.5, 5.5, 6.5] and (out[0, 1:] == -np.inf).all()
  # a tiny negative shift whose f32 fraction rounds to 1 is the integer position
  s4[0, 0, 1] = -1e-12
  out, count = ref.vote_fuse(v4, s4)
  assert np.array_equal(out[0], v4[0, 0]) and count.tolist() == [9, 0]


def test_count_and_the_named_cases():
  cases = {c[0]: c for c in ref.all_inputs()}
  out, count = ref.vote_fuse(*cases['beyond'][1:])
  assert (out == -np.inf).all() and count.tolist() == [0, 0]
  out, count = ref.vote_fuse(*cases['nonfinite_row'][1:])
  assert (out[[1, 2]] == -np.inf).all() and np.isfinite(out[[0, 3]]).all() and count.tolist() == [2 * 49, 0]
  _, v, s, w = cases['wrap']
  out, count = ref.vote_fuse(v, s, w)
  assert count[1] >= 2 and count[0] + count[1] + (out == -np.inf).sum() == out.size
  assert 0.05 < np.mean(v == -np.inf) < 0.15
  b = ref.bound(v, s, w)
  assert b[np.isfinite(out)].max() < 1e-5 and (b[np.isfinite(out)] > 0).all()
  _, v, s, w = cases['fractional']
  out, _ = ref.vote_fuse(v, s, w)
  for edge in (out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1]):
    assert (edge == -np.inf).all()
  assert np.isfinite(out).any()
