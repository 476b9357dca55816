"""CPU checks of occupancy_vjp_reference.gather_vjp_f32, the host restatement of the gather VJP's order
contract: against a float64 adjoint of the forward gather, against torch float64 autograd of a trilinear
gather, and against a plain scalar loop over the contract on the degenerate cases."""
import numpy as np
import pytest
import torch

import occupancy_reference as occ_ref
import occupancy_vjp_reference as vjp_ref
from oracle import grids as o_grids

f32 = np.float32
U = 2.0 ** -24                # f32 unit roundoff
CELL = 0.25                   # a power of two: point / cell is exact


def _points(rng, B, P, extent, lo=-0.3, hi=1.3):
  return (rng.uniform(lo, hi, (B, P, 3)) * np.asarray(extent) * CELL).astype(f32)


def _scalar_vjp(points, dfeat, shape, cell, L):
  """The contract as a scalar loop: lists per voxel in record order, chunks of L, np.float32 scalars."""
  B, X, Y, Z, D = shape
  P = points.shape[1]
  vox, wt = vjp_ref.taps_f32(points, shape, cell)
  dfeat = np.asarray(dfeat, f32).reshape(B * P, D)
  lists = {}
  for b in range(B):
    for p in range(P):
      for c in range(8):
        lists.setdefault((b, int(vox[b, p, c])), []).append((wt[b, p, c], b * P + p))
  out = np.zeros((B, X * Y * Z, D), f32)
  with np.errstate(invalid='ignore', over='ignore'):
    for (b, v), recs in lists.items():
      for ch in range(D):
        total = None
        for j in range(0, len(recs), L):
          s = None
          for w, row in recs[j:j + L]:
            t = f32(w * dfeat[row, ch])
            s = t if s is None else f32(s + t)
          total = s if total is None else f32(total + s)
        out[b, v, ch] = total
  return out.reshape(shape)


def _bits_equal(got, want):
  got, want = np.asarray(got, f32), np.asarray(want, f32)
  assert got.shape == want.shape
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
  g = np.where(np.isnan(got), f32(0), got).view(np.uint32)
  w = np.where(np.isnan(want), f32(0), want).view(np.uint32)
  assert (g == w).all(), int((g != w).sum())


def _abs_sums(points, dfeat, shape, cell):
  """Per voxel element: sum over its records of |w * d| in float64, and the largest record count."""
  B, X, Y, Z, D = shape
  vox, wt = vjp_ref.taps_f32(points, shape, cell)
  keys = (np.arange(B)[:, None, None] * (X * Y * Z) + vox).reshape(-1)
  a = np.abs(wt.reshape(-1).astype(np.float64))[:, None] * np.abs(
      np.asarray(dfeat, np.float64).reshape(-1, D)[np.arange(len(keys)) // 8])
  out = np.zeros((B * X * Y * Z, D))
  np.add.at(out, keys, a)
  return out.reshape(shape), int(np.bincount(keys).max())


@pytest.mark.parametrize('L', [1, 3, 256])
def test_adjoint_identity_against_the_forward_gather(L):
  """<d_vol, V> == <d_feat, gather(V)> to f32 rounding: gather = occupancy_reference.gather_f32 (the forward's
  f32 restatement) and the oracle's interpolate_nd (float64 volume).  The bound: every d_vol element is a sum
  of n <= n_max f32 products (n_max + 1 roundings of its terms' magnitude), every gathered element a sum of
  8 (+ 8 for the weights' own f32 products); the inner products are float64."""
  rng = np.random.default_rng(L)
  B, X, Y, Z, D = 2, 7, 6, 5, 12
  shape = (B, X, Y, Z, D)
  pts = _points(rng, B, 300, (X, Y, Z))
  dfeat = rng.normal(size=(B * 300, D)).astype(f32)
  V = rng.normal(size=shape).astype(f32)
  dvol = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, L)
  lhs = float((dvol.astype(np.float64) * V).sum())
  absd, n_max = _abs_sums(pts, dfeat, shape, CELL)
  mag = float((absd * np.abs(V.astype(np.float64))).sum())
  g32, _ = occ_ref.gather_f32(V, None, pts, CELL)
  rhs32 = float((dfeat.astype(np.float64) * g32.reshape(-1, D)).sum())
  assert abs(lhs - rhs32) <= (n_max + 1 + 16) * U * mag, (lhs, rhs32, mag)
  V64 = V.astype(np.float64)
  g64 = np.concatenate([o_grids.interpolate_nd(V64[b], (pts[b] / f32(CELL)).astype(np.float64), None)[0]
                        for b in range(B)])
  rhs64 = float((dfeat.astype(np.float64) * g64).sum())
  assert abs(lhs - rhs64) <= (n_max + 1 + 16) * U * mag, (lhs, rhs64, mag)
  rhs_exact = float((dfeat.astype(np.float64) * vjp_ref.gather_f64(V, pts, CELL)).sum())
  assert abs(lhs - rhs_exact) <= (n_max + 1) * U * mag, (lhs, rhs_exact, mag)


def test_against_torch_fp64_autograd_of_a_trilinear_gather():
  """d_vol against torch float64 autograd of a gather with the same rule (weights from the unclipped
  floor, indices clamped to the grid): per element within (n_max + 8) u * sum |w d| (the f32 sum of
  n_max products; the f32 weights differ from the float64 ones by a few ulps)."""
  rng = np.random.default_rng(5)
  B, X, Y, Z, D = 2, 6, 5, 4, 8
  shape = (B, X, Y, Z, D)
  pts = _points(rng, B, 250, (X, Y, Z))
  dfeat = rng.normal(size=(B * 250, D)).astype(f32)
  got = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, 256)
  vol = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
  p = torch.from_numpy(pts).double() / CELL
  c = p - 0.5
  lo = torch.floor(c)
  whi = c - lo
  size = torch.tensor([X, Y, Z])
  il = lo.long()
  feats = 0
  for corner in range(8):
    bits = [(corner >> (2 - t)) & 1 for t in range(3)]
    w = torch.ones(c.shape[:-1], dtype=torch.float64)
    idx = []
    for t in range(3):
      w = w * (whi[..., t] if bits[t] else 1 - whi[..., t])
      idx.append(torch.clamp(il[..., t] + bits[t], 0, int(size[t]) - 1))
    bidx = torch.arange(B)[:, None].expand(idx[0].shape)
    feats = feats + w[..., None] * vol[bidx, idx[0], idx[1], idx[2]]
  (ref,) = torch.autograd.grad(feats.reshape(-1, D), vol, torch.from_numpy(dfeat).double())
  absd, n_max = _abs_sums(pts, dfeat, shape, CELL)
  err = np.abs(got.astype(np.float64) - ref.numpy())
  assert (err <= (n_max + 8) * U * absd).all(), float((err / np.maximum(absd, 1e-300)).max())
  assert np.abs(got).max() > 0


def test_degenerate_points_match_the_scalar_contract():
  """Taps coinciding on grid faces (p = 0 and p just below size: both taps of an axis on one voxel), points
  outside the grid, NaN / +-inf / 1e30 coordinates (a NaN point's 8 taps all land on voxel 0 with NaN
  weights): bitwise the scalar loop, for several L."""
  B, X, Y, Z, D = 2, 5, 3, 4, 3
  shape = (B, X, Y, Z, D)
  below = lambda n: float(np.nextafter(f32(n), f32(0)))
  p = [[0, 0, 0], [below(5), below(3), below(4)], [0, 1.5, 2.0], [2.5, 0, below(4)], [-3, 1, 1], [9, 9, 9],
       [np.nan] * 3, [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e30, 1, 1], [-1e30, 2, 2],
       [2.25, 1.75, 3.5]]
  pts = (np.asarray(p, f32) * f32(CELL))
  pts = np.stack([pts, pts[::-1]]).astype(f32)
  rng = np.random.default_rng(1)
  dfeat = rng.normal(size=(B * len(p), D)).astype(f32)
  for L in (1, 2, 3, 256):
    got = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, L)
    _bits_equal(got, _scalar_vjp(pts, dfeat, shape, CELL, L))
  vox, wt = vjp_ref.taps_f32(pts, shape, CELL)
  assert (vox[0, 6] == 0).all() and np.isnan(wt[0, 6]).all()                 # the all-NaN point
  assert len(set(vox[0, 0].tolist())) == 1                                    # p = 0: every tap on voxel 0
  got = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, 256)
  assert np.isnan(got[:, 0, 0, 0]).all()


def test_one_voxel_receives_every_record():
  """A 1 x 1 x 1 grid: every tap of every point clamps to the one voxel (2400 records per scene, segment
  >> L): bitwise the scalar loop for L = 1, 7, 256 and L >= the segment."""
  B, D, P = 2, 4, 300
  shape = (B, 1, 1, 1, D)
  rng = np.random.default_rng(2)
  pts = (rng.uniform(-2, 3, (B, P, 3)) * CELL).astype(f32)
  dfeat = rng.normal(size=(B * P, D)).astype(f32)
  for L in (1, 7, 256, 8 * P):
    _bits_equal(vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, L), _scalar_vjp(pts, dfeat, shape, CELL, L))


def test_chunk_length_sets_the_order():
  """Points at one voxel centre (weights 1 on that voxel, 0 elsewhere) with d = 1, 2^-24, 2^-24, 2^-24: the
  in-order sum (L = 1, or L >= the segment) rounds every 2^-24 away (ties to even) and gives 1; L = 2 adds
  (1 + 2^-24) + (2^-24 + 2^-24) = 1 + 2^-23."""
  shape = (1, 3, 3, 3, 1)
  pts = np.full((1, 4, 3), 1.5 * CELL, f32)
  dfeat = np.asarray([[1.0], [U], [U], [U]], f32)
  one = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, 1)
  whole = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, 4 * 8)
  pairs = vjp_ref.gather_vjp_f32(pts, dfeat, shape, CELL, 2)
  # voxel (1, 1, 1): records (p, c = 0) of each point; c >= 1 go to neighbours with weight 0
  assert one[0, 1, 1, 1, 0] == f32(1) and whole[0, 1, 1, 1, 0] == f32(1)
  # L = 2: chunks of the records of voxel (1, 1, 1), which has exactly one record per point
  assert pairs[0, 1, 1, 1, 0] == f32(1 + 2 * U)
  _bits_equal(pairs, _scalar_vjp(pts, dfeat, shape, CELL, 2))
  assert (one[0, 2, 2, 2] == 0).all() and np.signbit(one[0, 0, 0, 0]).sum() == 0   # untouched: +0
