"""Exact host restatement of occupancy.hip's gather VJP into the volume (TEST INFRASTRUCTURE).

``gather_vjp_f32`` restates the order contract of snap_occupancy_ray_features_vjp_f32 (include/snap_hip.h)
in numpy f32, every operation one IEEE f32 operation:
  - each point's 8 taps as occ_taps computes them (``occupancy_reference.gather_f32``'s expressions: the
    same f32 weights (w_x * w_y) * w_z and the same clamped indices; NaN points clamp to voxel 0 with NaN
    weights), one record (voxel, p, c) per tap, contribution = w_c * d_features[b * P + p] (one multiply);
  - per voxel of each scene its records in ascending (p, c) order, cut into consecutive chunks of L;
    a chunk sum starts from its first contribution and adds the rest in order; the voxel starts from its
    first chunk sum and adds the others in chunk order; a voxel without records is +0.
The sums are vectorised over all chunks / voxels at once by rank (rank within the chunk, then chunk index
within the voxel): at each step every affected row takes exactly one f32 add, so the order is the scalar
loop's.
"""
import numpy as np

import occupancy_reference as occ_ref

f32 = np.float32


def taps_f32(points, shape, cell):
  """occ_taps on points [B, P, 3]: -> (voxel [B, P, 8] int64 flat index within the scene, weight [B, P, 8] f32),
  taps in the forward's order c = 4 bx + 2 by + bz."""
  points = np.asarray(points, f32)
  X, Y, Z = (int(v) for v in shape[1:4])
  size = (X, Y, Z)
  cell = f32(cell)
  idx, w = [], []
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    for t in range(3):
      p = points[..., t] / cell
      c = p - f32(0.5)
      lo = np.floor(c)
      whi = c - lo
      w.append((f32(1) - whi, whi))
      il = occ_ref._tap_base(lo, size[t])
      idx.append((np.clip(il, 0, size[t] - 1), np.clip(il + 1, 0, size[t] - 1)))
    vox, wt = [], []
    for corner in range(8):
      bits = [(corner >> (2 - t)) & 1 for t in range(3)]
      wt.append((w[0][bits[0]] * w[1][bits[1]]) * w[2][bits[2]])
      ix, iy, iz = (idx[t][bits[t]] for t in range(3))
      vox.append((ix * Y + iy) * Z + iz)
  return np.stack(vox, -1).astype(np.int64), np.stack(wt, -1).astype(f32)


def gather_vjp_sparse_f32(points, d_features, shape, cell, L):
  """The contract on the touched voxels only -> (keys [K] = b * XYZ + voxel ascending, rows [K, D] f32)."""
  points = np.asarray(points, f32)
  B, X, Y, Z, D = (int(v) for v in shape)
  P = points.shape[1]
  dfeat = np.asarray(d_features, f32).reshape(B * P, D)
  L = int(L)
  assert L >= 1
  vox, wt = taps_f32(points, shape, cell)
  keys = (np.arange(B, dtype=np.int64)[:, None, None] * (X * Y * Z) + vox).reshape(-1)     # record id order
  w = wt.reshape(-1)
  order = np.argsort(keys, kind='stable')                  # ties keep record id order = (p, c) ascending
  skeys = keys[order]
  R = len(skeys)
  head = np.ones(R, bool)
  head[1:] = skeys[1:] != skeys[:-1]
  seg_id = np.cumsum(head) - 1                             # touched voxel of each sorted record
  seg_start = np.flatnonzero(head)
  rank = np.arange(R) - seg_start[seg_id]
  with np.errstate(invalid='ignore', over='ignore'):
    contrib = w[order][:, None] * dfeat[order // 8]          # [R, D]: one f32 multiply per element
    # chunk sums, vectorised by rank within the chunk
    chunk_of = rank // L
    nch = np.zeros(len(seg_start), np.int64)
    np.maximum.at(nch, seg_id, chunk_of + 1)
    chunk_base = np.concatenate([[0], np.cumsum(nch)[:-1]])
    chunk_id = chunk_base[seg_id] + chunk_of
    sums = np.zeros((int(nch.sum()), D), f32)
    pos = rank % L
    for u in range(min(L, R)):
      sel = pos == u
      if not sel.any():
        break
      sums[chunk_id[sel]] = contrib[sel] if u == 0 else sums[chunk_id[sel]] + contrib[sel]
    # voxel sums, vectorised by chunk index within the voxel
    rows = np.zeros((len(seg_start), D), f32)
    for j in range(int(nch.max())):
      sel = np.flatnonzero(nch > j)
      rows[sel] = sums[chunk_base[sel]] if j == 0 else rows[sel] + sums[chunk_base[sel] + j]
  return skeys[seg_start], rows


def gather_vjp_f32(points, d_features, shape, cell, L):
  """points [B, P, 3], d_features [B * P, D] (or [B, P, D]), shape = (B, X, Y, Z, D), chunk length L ->
  d_volume [B, X, Y, Z, D] f32 under the order contract."""
  B, X, Y, Z, D = (int(v) for v in shape)
  keys, rows = gather_vjp_sparse_f32(points, d_features, shape, cell, L)
  out = np.zeros((B * X * Y * Z, D), f32)
  out[keys] = rows
  return out.reshape(B, X, Y, Z, D)


def gather_f64(volume, points, cell):
  """The trilinear gather with the same weights and clamped indices as occ_taps, in float64 arithmetic on
  the f32 weights: volume [B, X, Y, Z, D] -> [B * P, D] float64 (the adjoint's other side)."""
  B, X, Y, Z, D = volume.shape
  vox, wt = taps_f32(points, volume.shape, cell)
  flat = np.asarray(volume, np.float64).reshape(B, X * Y * Z, D)
  bidx = np.arange(B)[:, None, None]
  out = (wt.astype(np.float64)[..., None] * flat[bidx, vox]).sum(-2)
  return out.reshape(-1, D)
