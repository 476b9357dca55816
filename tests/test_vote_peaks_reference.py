"""CPU pins of the top-K peak contract (snap_vote_peaks_f32, include/snap_hip.h): the numpy restatement
``vote_peaks_reference`` against written-out answers, ``np.argmax`` and a plain-loop reading of the rule; the batched
index -> transform helper against the oracle, bit for bit; the C entry points' argument validation (no launch)."""
import ctypes

import numpy as np
import pytest
import torch

import vote_peaks_reference as ref
from oracle import grids as o_grids
from oracle import voting as o_voting
from snap_amd import _lib
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids

NINF = np.float32(-np.inf)


def _loops(v, k, rr, rx):
  """The rule of the header comment, cell by cell."""
  R, Ho, Wo = v.shape
  peaks = []
  for r in range(R):
    for a in range(Ho):
      for b in range(Wo):
        c = v[r, a, b]
        if np.isnan(c) or c == NINF:
          continue
        fc = (r * Ho + a) * Wo + b
        ok = True
        for dr in range(-rr, rr + 1):
          for da in range(-rx, rx + 1):
            for db in range(-rx, rx + 1):
              na, nb_ = a + da, b + db
              if (dr, da, db) == (0, 0, 0) or not (0 <= na < Ho and 0 <= nb_ < Wo):
                continue
              nr = (r + dr) % R
              n = v[nr, na, nb_]
              n = NINF if np.isnan(n) else n
              ok &= bool(c > n or (c == n and fc < (nr * Ho + na) * Wo + nb_))
        if ok:
          peaks.append((-float(c), fc, (r, a, b)))
  peaks.sort(key=lambda p: p[:2])
  return [p[2] for p in peaks[:k]], [np.float32(-p[0]) for p in peaks[:k]]


def test_k1_is_the_argmax():
  rng = np.random.default_rng(0)
  for shape in ((4, 5, 7), (8, 31, 33), (3, 1, 1)):
    for quant in (False, True):
      v = rng.standard_normal(shape).astype(np.float32)
      if quant:
        v = np.clip(np.round(v), -2, 2).astype(np.float32)
      for rr, rx in ((1, 1), (0, 2), (1, 4)):
        index, score, count = ref.vote_peaks(v, 1, rr, rx)
        want = np.unravel_index(np.argmax(v), shape)
        assert tuple(index[0]) == want and count.tolist() == [1, 0]
        assert score.view(np.int32)[0] == v[want].view(np.int32)


def test_constant_volume_has_one_peak_at_flat_zero():
  for value in (0.0, -3.5, np.inf):
    v = np.full((5, 6, 7), value, np.float32)
    index, score, count = ref.vote_peaks(v, 8, 1, 1)
    assert count.tolist() == [1, 0]
    assert index[0].tolist() == [0, 0, 0] and score[0] == np.float32(value)
    assert (index[1:] == -1).all() and (score[1:] == NINF).all()


def test_all_minus_inf_has_no_peak():
  index, score, count = ref.vote_peaks(np.full((4, 3, 5), -np.inf, np.float32), 4, 1, 2)
  assert count.tolist() == [0, 0]
  assert (index == -1).all() and (score == NINF).all() and index.dtype == np.int32 and score.dtype == np.float32


def test_hand_built_case():
  """2 x 3 x 3, radius_r = 0 (planes do not see each other), radius_xy = 1.
  plane 0: a 5-plateau on the top row's ends and a lone 4 in the far corner; plane 1: NaN beside the maximum,
  a -0 / +0 tie."""
  nan = np.nan
  v = np.array([[[5, 1, 5],
                 [1, 1, 1],
                 [0, 1, 4]],
                [[nan, 7, -1],
                 [-1, -1, -1],
                 [-0.0, -1, 0.0]]], np.float32)
  index, score, count = ref.vote_peaks(v, 8, 0, 1)
  # value descending, flat ascending: 7 | 5 (flat 0) | 5 (flat 2) | 4 | the two zeros (equal: flat order)
  assert index[:6].tolist() == [[1, 0, 1], [0, 0, 0], [0, 0, 2], [0, 2, 2], [1, 2, 0], [1, 2, 2]]
  assert score[:6].tolist() == [7, 5, 5, 4, 0, 0]
  assert np.signbit(score[4]) and not np.signbit(score[5])            # the vote's own bits
  assert count.tolist() == [6, 1]
  assert (index[6:] == -1).all() and (score[6:] == NINF).all()
  # (0, 2, 0) = 0 is no peak: its neighbours are 1s.  With radius_r = 1 (R = 2: refused, 2 * 1 + 1 > R)
  with pytest.raises(ValueError):
    ref.vote_peaks(v, 8, 1, 1)
  # K smaller than the number of peaks: the head of the same list
  i3, s3, c3 = ref.vote_peaks(v, 3, 0, 1)
  assert i3.tolist() == index[:3].tolist() and s3.tolist() == [7, 5, 5] and c3.tolist() == [3, 1]


def test_rotation_axis_wraps():
  R = 5
  v = np.zeros((R, 3, 3), np.float32)
  v[R - 1, 1, 1] = 2
  v[0, 1, 1] = 2
  # radius_r = 0: both are peaks; flat order puts r = 0 first
  index, _, count = ref.vote_peaks(v, 2, 0, 1)
  assert index.tolist() == [[0, 1, 1], [R - 1, 1, 1]] and count[0] == 2
  # radius_r >= 1: r = R-1 and r = 0 are neighbours; of equal values the smaller flat (r = 0) survives ...
  for rr in (1, 2):
    index, _, _ = ref.vote_peaks(v, 1, rr, 1)
    assert index.tolist() == [[0, 1, 1]]
    assert not ref.peak_mask(v, rr, 1)[R - 1, 1, 1]
  # ... and a greater value at r = R-1 suppresses r = 0, only through the wrap
  v[R - 1, 1, 1] = 3
  assert ref.peak_mask(v, 0, 1)[0, 1, 1]
  assert not ref.peak_mask(v, 1, 1)[0, 1, 1] and ref.peak_mask(v, 1, 1)[R - 1, 1, 1]


@pytest.mark.parametrize('shape,k,rr,rx', [((4, 5, 7), 6, 1, 1), ((5, 4, 6), 64, 2, 4), ((3, 6, 5), 5, 0, 2),
                                           ((3, 1, 9), 4, 1, 3)])
def test_restatement_equals_the_plain_loops(shape, k, rr, rx):
  rng = np.random.default_rng(sum(shape) + k)
  for kind in range(3):
    v = rng.standard_normal(shape).astype(np.float32)
    if kind >= 1:
      v = np.clip(np.round(v), -2, 2).astype(np.float32)
    if kind == 2:
      v.reshape(-1)[rng.choice(v.size, v.size // 6, replace=False)] = np.nan
      v.reshape(-1)[rng.choice(v.size, v.size // 6, replace=False)] = -np.inf
      v.reshape(-1)[rng.choice(v.size, 3, replace=False)] = np.inf
    index, score, count = ref.vote_peaks(v, k, rr, rx)
    want_i, want_s = _loops(v, k, rr, rx)
    n = len(want_i)
    assert count[0] == n and count[1] == int(np.isnan(v).sum())
    assert [tuple(r) for r in index[:n].tolist()] == want_i
    assert score[:n].view(np.int32).tolist() == [s.view(np.int32) for s in want_s]
    assert (index[n:] == -1).all() and (score[n:] == NINF).all()


@pytest.mark.parametrize('extent,cell,R', [((48, 48), 0.5, 36), ((8, 8), 0.25, 8), ((256, 256), 0.2, 36),
                                           ((33, 33), 0.7, 12)])
def test_exhaustive_indices_to_tfm_equals_the_oracle_bit_for_bit(extent, cell, R):
  rng = np.random.default_rng(R + extent[0])
  n = 64
  idx = np.stack([rng.integers(0, R, n), rng.integers(0, 2 * extent[0] - 1, n), rng.integers(0, 2 * extent[1] - 1, n)], -1)
  idx[0] = (0, extent[0] - 1, extent[1] - 1)                 # the identity
  idx[1] = (-1, -1, -1)                                       # no peak
  tf = pev.exhaustive_indices_to_tfm(torch.tensor(idx, dtype=torch.int32), grids.Grid2D(extent, cell), R)
  assert tuple(tf.shape) == (n,) and tf.angle.dtype == torch.float32 and tf.t.dtype == torch.float32
  og = o_grids.Grid2D(extent, cell)
  for i, row in enumerate(idx):
    if row[0] < 0:
      assert bool(torch.isnan(tf.angle[i])) and bool(torch.isnan(tf.t[i]).all())
      continue
    want = o_voting.exhaustive_index_to_tfm(row, og, R)
    assert want.angle.dtype == np.float32 and want.t.dtype == np.float32
    assert tf.angle[i].numpy().view(np.int32) == want.angle.view(np.int32), (row, tf.angle[i], want.angle)
    assert (tf.t[i].numpy().view(np.int32) == want.t.view(np.int32)).all(), (row, tf.t[i], want.t)


def test_vote_peaks_entry_points_validate_before_any_launch():
  """Status codes for bad arguments with dummy non-null pointers: nothing is launched (CPU-safe)."""
  lib = _lib.load()
  one = ctypes.c_void_p(16)
  ws_bytes = lib.snap_vote_peaks_workspace_bytes

  def call(R=36, Ho=63, Wo=63, K=16, rr=1, rx=1, votes=one, index=one, score=one, count=one, ws=one, nbytes=None):
    nbytes = ws_bytes(R, Ho, Wo, K, rr, rx) if nbytes is None else nbytes
    return lib.snap_vote_peaks_f32(votes, R, Ho, Wo, K, rr, rx, index, score, count, ws, nbytes, None)

  need = ws_bytes(36, 63, 63, 16, 1, 1)
  assert need > 0 and need % 8 == 0
  assert ws_bytes(36, 511, 511, 16, 1, 1) > 0 and ws_bytes(36, 511, 511, 64, 2, 4) > 0
  bad_shapes = [dict(K=0), dict(K=65), dict(rr=-1), dict(rr=3), dict(R=4, rr=2), dict(rx=0), dict(rx=5),
                dict(R=0), dict(Ho=0), dict(Wo=-1), dict(R=2048, Ho=1024, Wo=1024)]
  for kw in bad_shapes:
    full = dict(dict(R=36, Ho=63, Wo=63, K=16, rr=1, rx=1), **kw)
    assert ws_bytes(*(full[n] for n in ('R', 'Ho', 'Wo', 'K', 'rr', 'rx'))) == 0, kw
    assert call(nbytes=1 << 30, **kw) == -1, kw                                   # shape
  assert ws_bytes(4, 5, 7, 64, 1, 4) > 0 and ws_bytes(5, 5, 7, 64, 2, 4) > 0       # 2 radius_r + 1 == R is allowed
  for name in ('votes', 'index', 'score', 'count', 'ws'):
    assert call(**{name: None}) == -3, name                                       # pointer
  assert call(nbytes=need - 1) == -5 and call(nbytes=0) == -5                      # workspace: short
  assert call(ws=ctypes.c_void_p(20)) == -5                                        # workspace: not 8-byte aligned
