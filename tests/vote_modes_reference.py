"""float64 numpy restatement of the contract of snap_vote_modes_f32 (include/snap_hip.h) and of the propagation that
``pose_exhaustive_voting.modes_from_votes`` applies to its rows.  Written from the contract: ownership over the whole
volume at once, the sums per mode with numpy's own reductions, the NEES by a linear solve.

``vote_modes`` returns the float64 values BEFORE their rounding; ``round_stats`` applies the contract's single rounding
to f32 (and its rule for a mean rotation that rounds to R).  ``cases()`` lists the inputs the tests share."""
import math

import numpy as np

NAN_ROW = np.full(10, np.nan)


def supported(R, Ho, Wo, K, win_r, win_xy):
  return (R >= 1 and Ho >= 1 and Wo >= 1 and R * Ho * Wo < 2 ** 31 and 1 <= K <= 64 and 0 <= win_r <= 4
          and 2 * win_r + 1 <= R and 1 <= win_xy <= 32)


def nonempty_rows(peaks, shape):
  p = np.asarray(peaks, dtype=np.int64).reshape(-1, 3)
  return ((p >= 0) & (p < np.asarray(shape, dtype=np.int64)[None])).all(-1)


def wrap_offset(d, R):
  """(r - r_k) as its nearest representative; R / 2 stays R / 2 (outside every supported window)."""
  d = np.mod(d, R)
  return np.where(2 * d > R, d - R, d)


def ownership(shape, peaks, win_r, win_xy):
  """-> (owner int32 [R, Ho, Wo], -1 = nobody; offsets int64 [3, R, Ho, Wo] = (dr, da, db) from the owner)."""
  R, Ho, Wo = shape
  p = np.asarray(peaks, dtype=np.int64).reshape(-1, 3)
  ok = nonempty_rows(p, shape)
  wr = max(win_r, 1)
  r, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Wo), indexing='ij')
  owner = np.full(shape, -1, dtype=np.int32)
  best = np.full(shape, np.iinfo(np.int64).max, dtype=np.int64)
  off = np.zeros((3,) + tuple(shape), dtype=np.int64)
  for k in range(p.shape[0]):
    if not ok[k]:
      continue
    dr, da, db = wrap_offset(r - p[k, 0], R), a - p[k, 1], b - p[k, 2]
    inside = (np.abs(dr) <= win_r) & (np.abs(da) <= win_xy) & (np.abs(db) <= win_xy)
    D = wr * wr * (da * da + db * db) + win_xy * win_xy * dr * dr
    take = inside & (D < best)                              # (strictly: a tie stays with the lower k)
    owner[take] = k
    best[take] = D[take]
    for i, d in enumerate((dr, da, db)):
      off[i][take] = d[take]
  return owner, off


def ownership_loops(shape, peaks, win_r, win_xy):
  """The ownership rule as a literal loop over cells and peaks."""
  R, Ho, Wo = shape
  p = [tuple(int(x) for x in row) for row in np.asarray(peaks).reshape(-1, 3)]
  wr = max(win_r, 1)
  owner = np.full(shape, -1, dtype=np.int32)
  for r in range(R):
    for a in range(Ho):
      for b in range(Wo):
        best = None
        for k, (rk, ak, bk) in enumerate(p):
          if not (0 <= rk < R and 0 <= ak < Ho and 0 <= bk < Wo):
            continue
          dr = (r - rk) % R
          if 2 * dr > R:
            dr -= R
          da, db = a - ak, b - bk
          if abs(dr) > win_r or abs(da) > win_xy or abs(db) > win_xy:
            continue
          D = wr * wr * (da * da + db * db) + win_xy * win_xy * dr * dr
          if best is None or D < best:
            best = D
            owner[r, a, b] = k
  return owner


def vote_modes(votes, peaks, win_r=1, win_xy=4, scale=1.0, gt_index=None):
  """-> (stats float64 [K, 16], count int32 [K, 2], owner int32 [R, Ho, Wo])."""
  v = np.asarray(votes)
  assert v.dtype == np.float32 and v.ndim == 3
  p = np.asarray(peaks, dtype=np.int64).reshape(-1, 3)
  K = p.shape[0]
  R, Ho, Wo = v.shape
  if not supported(R, Ho, Wo, K, win_r, win_xy):
    raise ValueError(f'vote_modes: unsupported {v.shape} K={K} win_r={win_r} win_xy={win_xy}')
  scale = float(np.float32(scale))
  if not (scale > 0 and math.isfinite(scale)):
    raise ValueError(f'vote_modes: scale {scale}')
  owner, off = ownership(v.shape, p, win_r, win_xy)
  finite = np.isfinite(v)
  bad = np.isnan(v) | (v == np.inf)
  gt = None
  if gt_index is not None:
    g = np.asarray(gt_index, dtype=np.float32).astype(np.float64).reshape(3)
    gt = g if np.isfinite(g).all() else None
  stats = np.zeros((K, 16))
  count = np.zeros((K, 2), dtype=np.int32)
  for k in range(K):
    mine = owner == k
    sel = mine & finite
    count[k] = int(sel.sum()), int((mine & bad).sum())
    if count[k, 0] == 0:
      stats[k, 0:2] = -np.inf
      stats[k, 2:12] = np.nan
      continue
    x = scale * v[sel].astype(np.float64)
    m = x.max()
    w = np.exp(x - m)
    S0 = w.sum()
    d = np.stack([off[i][sel] for i in range(3)]).astype(np.float64)        # [3, n]
    e = (d * w).sum(-1) / S0
    second = (d[:, None] * d[None] * w).sum(-1) / S0
    cov = second - e[:, None] * e[None]
    mean = p[k].astype(np.float64) + e
    if mean[0] < 0:
      mean[0] += R
    if mean[0] >= R:
      mean[0] -= R
    stats[k, 0], stats[k, 1] = m + math.log(S0), m
    stats[k, 2:5] = mean
    stats[k, 5:11] = cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]
    stats[k, 11] = np.nan
    if gt is not None:
      err = gt - mean
      err[0] = math.remainder(err[0], R)
      A = cov + np.eye(3) / 12
      stats[k, 11] = float(err @ np.linalg.solve(A, err))
  return stats, count, owner


def nees_condition(stats):
  """The largest condition number of (Sigma + I / 12) over the non-empty modes of ``stats``."""
  worst = 1.0
  for row in np.asarray(stats):
    if np.isfinite(row[0]):
      c = np.array([[row[5], row[6], row[7]], [row[6], row[8], row[9]], [row[7], row[9], row[10]]]) + np.eye(3) / 12
      worst = max(worst, float(np.linalg.cond(c)))
  return worst


def round_stats(stats, R):
  """The contract's single rounding of the float64 rows to f32; a mean rotation that rounds to R is stored as 0."""
  s = np.asarray(stats).astype(np.float32)
  s[:, 2] = np.where(s[:, 2] >= np.float32(R), np.float32(0), s[:, 2])
  return s


def log_z(votes, scale=1.0):
  v = np.asarray(votes)
  x = float(np.float32(scale)) * v[np.isfinite(v)].astype(np.float64)
  if x.size == 0:
    return -np.inf
  return float(x.max() + math.log(np.exp(x - x.max()).sum()))


# ------------------------------- the wrapper's propagation ----------------------------------------
def _compose(p, q):
  """SE(2): (angle, tx, ty) of p @ q."""
  c, s = math.cos(p[0]), math.sin(p[0])
  return (p[0] + q[0], p[1] + c * q[1] - s * q[2], p[2] + s * q[1] + c * q[2])


def _inverse(p):
  c, s = math.cos(p[0]), math.sin(p[0])
  return (-p[0], -(c * p[1] + s * p[2]), -(-s * p[1] + c * p[2]))


def index_to_pose(index, extent, cell, R):
  """``exhaustive_index_to_tfm`` in float64 for a continuous index (k, a, b): c @ (-angle, xy_cell) @ c^-1 by explicit
  composition -> (angle, tx, ty)."""
  k, a, b = (float(x) for x in index)
  H, W = extent
  centre = (0.0, H * cell / 2, W * cell / 2)
  mid = (-(k * 2 * math.pi / R), (a - H + 1 + 0.5) * cell, (b - W + 1 + 0.5) * cell)
  return np.array(_compose(_compose(centre, mid), _inverse(centre)))


def pose_jacobian(index, extent, cell, R):
  """d (angle, tx, ty) / d (k, a, b) at a continuous index, analytically."""
  H, W = extent
  cx, cy = H * cell / 2, W * cell / 2
  dphi = -2 * math.pi / R
  phi = float(index[0]) * dphi
  c, s = math.cos(phi), math.sin(phi)
  return np.array([[dphi, 0, 0], [(s * cx + c * cy) * dphi, cell, 0], [(-c * cx + s * cy) * dphi, 0, cell]])


def modes(stats32, lz, extent, cell, R):
  """``modes_from_votes``' outputs from the op's f32 rows and a log_z, in float64 -> dict(weight [K], unassigned,
  pose [K, 3] = (angle, tx, ty), cov_index [K, 3, 3], cov [K, 3, 3])."""
  s = np.asarray(stats32).astype(np.float64)
  K = s.shape[0]
  with np.errstate(invalid='ignore'):
    weight = np.exp(s[:, 0] - float(lz))
  pose = np.full((K, 3), np.nan)
  cov_index = np.full((K, 3, 3), np.nan)
  cov = np.full((K, 3, 3), np.nan)
  for k in range(K):
    if not np.isfinite(s[k, 0]):
      continue
    pose[k] = index_to_pose(s[k, 2:5], extent, cell, R)
    c = np.array([[s[k, 5], s[k, 6], s[k, 7]], [s[k, 6], s[k, 8], s[k, 9]], [s[k, 7], s[k, 9], s[k, 10]]])
    J = pose_jacobian(s[k, 2:5], extent, cell, R)
    cov_index[k] = c
    cov[k] = J @ c @ J.T
  return dict(weight=weight, unassigned=1.0 - weight.sum(), pose=pose, cov_index=cov_index, cov=cov)


# ------------------------------- inputs ------------------------------------------------------------
SHAPES = ((4, 5, 7), (8, 31, 33), (36, 63, 63))
SETTINGS = ((1, 0, 1), (16, 1, 4), (64, 2, 16), (5, 3, 32))     # (K, win_r, win_xy)


def smooth_votes(shape, seed, bumps=6, amplitude=6.0):
  """A few Gaussian bumps (circular in r) plus noise: distinct peaks with mass around them."""
  rng = np.random.default_rng(seed)
  R, Ho, Wo = shape
  r, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Wo), indexing='ij')
  v = 0.3 * rng.standard_normal(shape)
  for _ in range(bumps):
    c = rng.uniform(0, 1, 3) * np.array(shape)
    sig = rng.uniform(0.6, 2.5, 3)
    dr = np.abs(r - c[0])
    dr = np.minimum(dr, R - dr)
    v += amplitude * rng.uniform(0.5, 1) * np.exp(-0.5 * ((dr / sig[0]) ** 2 + ((a - c[1]) / sig[1]) ** 2
                                                           + ((b - c[2]) / sig[2]) ** 2))
  return v.astype(np.float32)


def random_peaks(shape, K, seed):
  """K distinct random cells, in no particular order."""
  rng = np.random.default_rng(seed)
  flat = rng.choice(int(np.prod(shape)), size=K, replace=K > int(np.prod(shape)))
  return np.stack(np.unravel_index(flat, shape), -1).astype(np.int32)


def _case(name, votes, peaks, win_r, win_xy, scale=1.0, gt=None):
  return dict(name=name, votes=votes, peaks=np.ascontiguousarray(peaks, dtype=np.int32), win_r=win_r, win_xy=win_xy,
              scale=scale, gt=gt)


def normal_cases():
  """Every shape with every setting it supports, hand-written (random, unsorted) peak tables, a ground truth."""
  out = []
  for si, shape in enumerate(SHAPES):
    for (K, win_r, win_xy) in SETTINGS:
      if not supported(*shape, K, win_r, win_xy):
        continue
      v = smooth_votes(shape, seed=100 + si)
      peaks = random_peaks(shape, K, seed=7 * K + si)
      gt = (peaks[0, 0] + 0.3, min(peaks[0, 1] + 0.4, shape[1] - 1), max(peaks[0, 2] - 0.2, 0))
      out.append(_case(f'normal{shape}_K{K}_w{win_r}_{win_xy}', v, peaks, win_r, win_xy, 1.5, gt))
  return out


def special_cases():
  out = []
  shape = (8, 31, 33)
  R, Ho, Wo = shape
  v = smooth_votes(shape, seed=5)
  corners = [(r, a, b) for r in (0, R - 1) for a in (0, Ho - 1) for b in (0, Wo - 1)]
  out.append(_case('corners_w1_4', v, corners, 1, 4, 1.0, (7.6, 0.2, 32.0)))
  out.append(_case('corners_w3_32', v, corners, 3, 32, 0.5, (0.1, 30.0, 0.0)))
  # two peaks whose windows overlap; the cells of column 12 (and, a rotation apart, the planted pairs) are
  # equidistant from both and go to row 0, which lies to the RIGHT of row 1
  out.append(_case('ties_w1_4', v, [(2, 10, 14), (2, 10, 10), (3, 12, 12)], 1, 4, 1.0, (2.0, 10.0, 12.0)))
  out.append(_case('ties_w2_16', v, [(5, 20, 8), (5, 8, 20), (4, 14, 14), (6, 14, 14)], 2, 16, 1.0))
  out.append(_case('duplicate_w1_4', v, [(1, 5, 5), (6, 20, 20), (1, 5, 5), (6, 20, 21), (6, 20, 20)], 1, 4, 2.0,
                   (6.0, 20.0, 20.5)))
  big, small = np.iinfo(np.int32).max, np.iinfo(np.int32).min
  out.append(_case('empty_rows_w1_4', v,
                   [(-1, -1, -1), (3, 15, 16), (R, 15, 16), (3, Ho, 16), (3, 15, Wo), (-1, 15, 16), (3, -1, 16),
                    (3, 15, -1), (big, 15, 16), (3, big, big), (small, small, small), (3, small, 16), (-1, -1, -1),
                    (4, 15, 17)], 1, 4, 1.0, (3.2, 15.1, 16.3)))
  dirty = v.copy()
  dirty[3, 15, 16] = np.nan
  dirty[3, 14, 17] = np.inf
  dirty[4, 15, 15] = np.nan
  dirty[2, 13:18, 14] = -np.inf
  out.append(_case('nan_inf_w1_4', dirty, [(3, 15, 16), (6, 3, 3)], 1, 4, 1.0, (3.0, 15.0, 16.0)))
  hole = v.copy()
  hole[2:5, 9:22, 10:23] = -np.inf                           # every cell of peak 0's window
  out.append(_case('masked_window_w1_4', hole, [(3, 15, 16), (6, 3, 3), (3, 15, 22)], 1, 4, 1.0, (3.0, 15.0, 16.0)))
  one = np.full(shape, -np.inf, dtype=np.float32)
  one[0, 0, 0] = 2.5                                         # a mode of one cell: Sigma = 0, the I / 12 term alone
  out.append(_case('one_cell_w2_16', one, [(0, 0, 0), (4, 15, 15)], 2, 16, 1.0, (7.9, 0.25, 0.25)))
  out.append(_case('all_masked_w1_4', np.full(shape, -np.inf, dtype=np.float32), [(3, 15, 16), (-1, -1, -1)], 1, 4,
                   1.0, (3.0, 15.0, 16.0)))
  out.append(_case('gt_not_finite_w1_4', v, [(3, 15, 16)], 1, 4, 1.0, (np.nan, 15.0, 16.0)))
  out.append(_case('tiny_w0_1', smooth_votes((4, 5, 7), seed=9), [(3, 4, 6), (0, 0, 0), (3, 4, 5)], 0, 1, 1.0,
                   (3.0, 4.0, 6.0)))
  return out


def cases():
  return normal_cases() + special_cases()
