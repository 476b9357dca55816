"""float64 numpy restatement of the contract of snap_vote_recall_f32 (include/snap_hip.h).  Written from the contract,
nothing clever: the weights e = exp(x - m) of the finite cells as a float64 volume, and for every offset (dr, da, db)
of a ball one shifted copy of that volume added to the masses (circular in r, zeros outside the volume in a, b).

``vote_recall`` returns the float64 log masses BEFORE their rounding; ``round_log_mass`` applies the contract's single
rounding to f32; ``best_of`` is the contract's arg-max of an f32 map.  ``cases()`` lists the inputs the tests share."""
import functools
import math

import numpy as np

from vote_modes_reference import index_to_pose, smooth_votes   # noqa: F401  (the family's recipes, shared by import)

LATTICE_COUNTS = {0: 1, 1: 5, 2: 9, 4: 13, 25: 81}          # N(rho2): the points (da, db) with da^2 + db^2 <= rho2


def supported(R, Ho, Wo, K, rho2, half_r):
  rho2, half_r = list(rho2), list(half_r)
  return (1 <= R <= 64 and Ho >= 1 and Wo >= 1 and R * Ho * Wo < 2 ** 31 and 0 <= K <= 64 and 1 <= len(rho2) <= 8
          and len(half_r) == len(rho2) and all(0 <= q <= 1024 for q in rho2)
          and all(0 <= h <= 4 and 2 * h + 1 <= R for h in half_r))


def disc_offsets(rho2):
  rho = math.isqrt(rho2)
  return [(da, db) for da in range(-rho, rho + 1) for db in range(-rho, rho + 1) if da * da + db * db <= rho2]


def ball_mask(shape, centre, rho2, half_r):
  """The cells of the ball around ``centre`` = (r, a, b): circular in r, clipped in a and b."""
  R, Ho, Wo = shape
  mask = np.zeros(shape, dtype=bool)
  for dr in range(-half_r, half_r + 1):
    for da, db in disc_offsets(rho2):
      a, b = centre[1] + da, centre[2] + db
      if 0 <= a < Ho and 0 <= b < Wo:
        mask[(centre[0] + dr) % R, a, b] = True
  return mask


def gt_cell(gt_index, shape):
  """The contract's rounding of a ground-truth index (k, i, j) -> (r, a, b), or None when it is invalid."""
  if gt_index is None:
    return None
  R, Ho, Wo = shape
  g = np.asarray(gt_index, dtype=np.float32).reshape(3)
  if not np.isfinite(g).all():
    return None
  k, i, j = float(g[0]), float(g[1]), float(g[2])
  if not (abs(k) <= 2 ** 20 and 0 <= i <= Ho - 1 and 0 <= j <= Wo - 1):
    return None
  return int(np.rint(g[0])) % R, int(np.rint(i)), int(np.rint(j))      # (np.rint: half to even)


def weights(votes, scale):
  """-> (e float64 [R, Ho, Wo], 0 where the cell does not contribute; m; S; count (finite, NaN or +inf))."""
  v = np.asarray(votes)
  assert v.dtype == np.float32 and v.ndim == 3
  finite = np.isfinite(v)
  bad = int((np.isnan(v) | (v == np.inf)).sum())
  e = np.zeros(v.shape)
  if not finite.any():
    return e, -np.inf, 0.0, (0, bad)
  x = float(np.float32(scale)) * v[finite].astype(np.float64)
  m = x.max()
  e[finite] = np.exp(x - m)
  return e, float(m), float(e.sum()), (int(finite.sum()), bad)


def ball_masses(e, rho2, half_r):
  """The mass of every cell's ball: one shifted copy of the volume per offset."""
  R, Ho, Wo = e.shape
  rho = math.isqrt(rho2)
  w = np.zeros_like(e)
  for dr in range(-half_r, half_r + 1):
    w += np.roll(e, -dr, axis=0)                              # w[r] += e[(r + dr) mod R]
  pad = np.zeros((R, Ho + 2 * rho, Wo + 2 * rho))
  pad[:, rho:rho + Ho, rho:rho + Wo] = w
  mass = np.zeros_like(e)
  for da, db in disc_offsets(rho2):
    mass += pad[:, rho + da:rho + da + Ho, rho + db:rho + db + Wo]
  return mass


def log_mass(mass, S):
  out = np.full(mass.shape, -np.inf)
  pos = mass > 0                                              # (a positive mass implies S > 0)
  if pos.any():
    out[pos] = np.minimum(0.0, np.log(mass[pos]) - math.log(S))
  return out


def float64_slack(shape, log_z, m):
  """How far two float64 evaluations of log(sum over a ball) - log S can lie apart: each of the two sums of at most
  N = R Ho Wo non-negative terms has a relative error of at most N 2^-53 in any order, each logarithm one ulp of a
  value of at most log S = log_z - m, the subtraction one more; for both sides together.  Next to two f32 ulps of the
  log mass this matters only for a ball that holds nearly all of the mass (|log mass| < ~1e-4), where the difference
  cancels and an f32 ulp of the result is smaller than the float64 error of its operands."""
  n = int(np.prod(shape))
  log_s = max(1.0, abs(log_z - m)) if math.isfinite(log_z) else 1.0
  return 2.0 ** -52 * (2 * n + 8 * log_s)


def vote_recall(votes, rho2, half_r, centres=None, scale=1.0, gt_index=None):
  """-> dict(maps float64 [L, R, Ho, Wo], centre float64 [K, L], gt float64 [L], log_z, m, count int32 [4],
  gt_cell)."""
  v = np.asarray(votes)
  R, Ho, Wo = v.shape
  c = np.zeros((0, 3), dtype=np.int64) if centres is None else np.asarray(centres, dtype=np.int64).reshape(-1, 3)
  K, L = c.shape[0], len(rho2)
  if not supported(R, Ho, Wo, K, rho2, half_r):
    raise ValueError(f'vote_recall: unsupported {v.shape} K={K} rho2={rho2} half_r={half_r}')
  scale = float(np.float32(scale))
  if not (scale > 0 and math.isfinite(scale)):
    raise ValueError(f'vote_recall: scale {scale}')
  e, m, S, (n_ok, n_bad) = weights(v, scale)
  maps = np.stack([log_mass(ball_masses(e, rho2[l], half_r[l]), S) for l in range(L)])
  ok = ((c >= 0) & (c < np.asarray(v.shape)[None])).all(-1)
  centre = np.full((K, L), -np.inf)
  for k in range(K):
    if ok[k]:
      centre[k] = maps[:, c[k, 0], c[k, 1], c[k, 2]]
  cell = gt_cell(gt_index, v.shape)
  gt = np.full(L, np.nan) if cell is None else maps[:, cell[0], cell[1], cell[2]].copy()
  log_z = m + math.log(S) if S > 0 else -np.inf
  return dict(maps=maps, centre=centre, gt=gt, log_z=log_z, m=m,
              count=np.array([n_ok, n_bad, int(cell is not None), 0], dtype=np.int32), gt_cell=cell)


def round_log_mass(x64):
  """The contract's single rounding of a float64 log mass to f32."""
  return np.asarray(x64).astype(np.float32)


def round_stats(log_z, m):
  return np.array([log_z, m, 0.0, 0.0]).astype(np.float32)


def best_of(maps32):
  """The contract's arg-max of f32 maps [L, R, Ho, Wo]: the greater value, then the lower flat index ->
  (index int32 [L, 3], value f32 [L]); (-1, -1, -1) and -inf where no cell is above -inf."""
  m = np.asarray(maps32)
  assert m.dtype == np.float32
  L = m.shape[0]
  index = np.full((L, 3), -1, dtype=np.int32)
  value = np.full(L, -np.inf, dtype=np.float32)
  for l in range(L):
    flat = int(np.argmax(m[l]))                               # (the first maximum in flat order; no NaN in a map)
    if m[l].reshape(-1)[flat] > -np.inf:
      index[l] = np.unravel_index(flat, m.shape[1:])
      value[l] = m[l].reshape(-1)[flat]
  return index, value


# ------------------------------- inputs ------------------------------------------------------------
L8_RHO2 = (0, 1, 2, 25, 100, 625, 1024, 4)
L8_HALF_R = (0, 1, 2, 3, 4, 0, 1, 2)


def mask_border(v, width):
  v = v.copy()
  v[:, :width] = v[:, -width:] = -np.inf
  v[:, :, :width] = v[:, :, -width:] = -np.inf
  return v


def random_centres(shape, K, seed):
  rng = np.random.default_rng(seed)
  return np.stack([rng.integers(0, n, size=K) for n in shape], -1).astype(np.int32)


def planted_votes(shape, centre, seed, sigma=(0.8, 1.5, 1.5), height=9.0):
  """One Gaussian cluster (circular in r) on low noise."""
  rng = np.random.default_rng(seed)
  R, Ho, Wo = shape
  r, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Wo), indexing='ij')
  dr = np.abs(r - centre[0])
  dr = np.minimum(dr, R - dr)
  d2 = (dr / sigma[0]) ** 2 + ((a - centre[1]) / sigma[1]) ** 2 + ((b - centre[2]) / sigma[2]) ** 2
  return (0.05 * rng.standard_normal(shape) + height * np.exp(-0.5 * d2)).astype(np.float32)


def _case(name, votes, rho2, half_r, centres=None, scale=1.0, gt=None, planted=None):
  c = None if centres is None else np.ascontiguousarray(centres, dtype=np.int32).reshape(-1, 3)
  return dict(name=name, votes=votes, rho2=tuple(rho2), half_r=tuple(half_r), centres=c, scale=scale, gt=gt,
              planted=planted)


def cases():
  out = []
  one = np.full((1, 1, 1), 0.7, dtype=np.float32)
  out.append(_case('single_cell_L1', one, (0,), (0,), [(0, 0, 0)], 1.0, (0.0, 0.0, 0.0)))
  out.append(_case('single_cell_L2', one, (1024, 0), (0, 0)))
  # a ball larger than the volume: every log mass is exactly 0
  out.append(_case('ball_covers_volume', smooth_votes((3, 5, 6), seed=1), (1024,), (1,), random_centres((3, 5, 6), 4, 2),
                   1.5, (2.5, 4.0, 0.5)))
  # a single row / a single column, and a ragged last tile of 64 columns (700 = 10 * 64 + 60)
  out.append(_case('single_row', smooth_votes((2, 1, 700), seed=2), (0, 25, 1024), (0, 0, 0),
                   [(0, 0, 0), (1, 0, 699), (1, 0, 350), (-1, -1, -1)], 1.0, (1.0, 0.0, 698.5)))
  out.append(_case('single_column', smooth_votes((2, 700, 1), seed=3), (0, 25, 1024), (0, 0, 0),
                   [(0, 0, 0), (1, 699, 0), (1, 350, 0)], 1.0, (0.5, 127.5, 0.0)))
  shape = (8, 31, 33)
  v = smooth_votes(shape, seed=5)
  out.append(_case('odd_L1', v, (25,), (1,), None, 2.0))                                        # K = 0, no ground truth
  out.append(_case('odd_L8', v, L8_RHO2, (0, 1, 2, 3, 0, 1, 2, 3), random_centres(shape, 64, 6), 1.5,
                   (7.5, 30.0, 0.5)))                                                           # half-cells: to even
  out.append(_case('masked_border', mask_border(v, 3), (0, 2, 100), (0, 1, 3), random_centres(shape, 16, 7), 1.0,
                   (2.5, 1.5, 2.5)))                                                            # a masked truth cell
  dirty = v.copy()
  dirty[3, 15, 16] = np.nan
  dirty[3, 14, 17] = np.inf
  dirty[4, 15, 15] = np.nan
  dirty[2, 13:18, 14] = -np.inf
  out.append(_case('nan_inf', dirty, (0, 1, 25), (0, 0, 1), [(3, 15, 16), (3, 14, 17), (2, 15, 14), (6, 3, 3)], 1.0,
                   (3.0, 15.0, 16.0)))
  out.append(_case('all_masked', np.full(shape, -np.inf, dtype=np.float32), (0, 25), (0, 1),
                   [(3, 15, 16), (-1, -1, -1)], 1.0, (3.0, 15.0, 16.0)))
  big, small = np.iinfo(np.int32).max, np.iinfo(np.int32).min
  out.append(_case('empty_rows_gt_out_of_range', v, (2, 25), (1, 0),
                   [(-1, -1, -1), (3, 15, 16), (8, 15, 16), (3, 31, 16), (3, 15, 33), (3, -1, 16), (big, 15, 16),
                    (small, small, small), (4, 15, 17)], 1.0, (3.0, 30.5, 16.0)))               # i > Ho - 1
  out.append(_case('gt_not_finite', v, (2,), (1,), None, 1.0, (np.nan, 15.0, 16.0)))
  out.append(_case('gt_wraps', v, (2, 25), (1, 2), None, 1.0, (-0.6, 0.0, 32.0)))               # rotation -1 -> 7
  # a window over all of R
  out.append(_case('window_covers_R', smooth_votes((9, 20, 20), seed=8), (4, 100, 1024), (4, 4, 0),
                   random_centres((9, 20, 20), 8, 9), 1.0, (8.5, 19.0, 0.0)))
  shape = (36, 63, 63)
  out.append(_case('c4_small_L8', mask_border(smooth_votes(shape, seed=10), 2), L8_RHO2, L8_HALF_R,
                   random_centres(shape, 64, 11), 2.0, (35.5, 31.5, 40.5)))
  out.append(_case('c4_small_L1', smooth_votes(shape, seed=12), (3,), (0,), random_centres(shape, 5, 13), 1.0))
  shape = (64, 17, 19)
  out.append(_case('r64_L8', smooth_votes(shape, seed=14), L8_RHO2, L8_HALF_R, random_centres(shape, 16, 15), 1.0,
                   (63.5, 16.0, 18.0)))
  # planted single clusters: the best cell must lie in the ball around the reference's best
  out.append(_case('planted_centre', planted_votes((8, 31, 33), (5, 14, 20), seed=16), (3, 15, 63), (0, 0, 1),
                   [(5, 14, 20)], 1.0, (5.0, 14.0, 20.0), planted=(5, 14, 20)))
  out.append(_case('planted_corner_wrap', planted_votes((36, 63, 63), (0, 1, 61), seed=17), (3, 15, 63), (0, 1, 2),
                   [(0, 1, 61)], 2.0, (0.0, 1.0, 61.0), planted=(0, 1, 61)))
  return out


@functools.lru_cache(maxsize=None)
def shared():
  """name -> (case, the reference's result), computed once for all tests of a session and left unchanged."""
  return {c['name']: (c, vote_recall(c['votes'], c['rho2'], c['half_r'], c['centres'], c['scale'], c['gt']))
          for c in cases()}
