"""numpy restatement of the contract of snap_vote_peaks_f32 (include/snap_hip.h): top-K peaks of a vote volume.

Written from the header's comment; imports nothing of the package.  float32 values, padded-array comparisons.

  votes [R, Ho, Wo] f32, flat(r, a, b) = (r * Ho + a) * Wo + b.
  PEAK: a cell c whose value is a number > -inf and which, for every OTHER cell n of its window
    |dr| <= radius_r (circular), |da| <= radius_xy, |db| <= radius_xy (clipped: cells outside do not exist), has
    v(c) > v(n) or (v(c) == v(n) and flat(c) < flat(n)).  A NaN vote is never a peak and compares like -inf as a
    neighbour; +inf is an ordinary value; == is the float comparison (-0 == +0).
  SELECTION: the K peaks of greatest value, by value descending, then flat ascending.
  -> index int32 [K, 3] = (r, a, b), score f32 [K] (the vote's own bits), count int32 [2] = (peaks found clipped to K,
     NaN votes); rows past the found count: index -1, score -inf.
"""
import numpy as np


def supported(shape, k, radius_r, radius_xy):
  if len(shape) != 3 or min(shape) < 1:
    return False
  R, Ho, Wo = shape
  return (1 <= k <= 64 and 0 <= radius_r <= 2 and 2 * radius_r + 1 <= R and 1 <= radius_xy <= 4
          and R * Ho * Wo < 2 ** 31)


def peak_mask(votes, radius_r, radius_xy):
  """Boolean [R, Ho, Wo]: the cells that are peaks."""
  v = np.asarray(votes)
  assert v.dtype == np.float32 and v.ndim == 3
  R, Ho, Wo = v.shape
  x = radius_xy
  vn = np.where(np.isnan(v), np.float32(-np.inf), v)          # what a neighbour compares as
  flat = np.arange(v.size, dtype=np.int64).reshape(v.shape)
  pad = ((0, 0), (x, x), (x, x))
  vp = np.pad(vn, pad, constant_values=np.float32(-np.inf))
  fp = np.pad(flat, pad, constant_values=-1)
  ep = np.pad(np.ones(v.shape, bool), pad, constant_values=False)    # the neighbour exists
  peak = ~np.isnan(v) & (v > -np.inf)
  for dr in range(-radius_r, radius_r + 1):
    # neighbour rotation (r + dr) mod R
    vr, fr, er = (np.roll(t, -dr, axis=0) for t in (vp, fp, ep))
    for da in range(-x, x + 1):
      for db in range(-x, x + 1):
        if dr == 0 and da == 0 and db == 0:
          continue
        sl = (slice(None), slice(x + da, x + da + Ho), slice(x + db, x + db + Wo))
        n, fn, en = vr[sl], fr[sl], er[sl]
        peak &= ~en | (vn > n) | ((vn == n) & (flat < fn))
  return peak


def vote_peaks(votes, k, radius_r=1, radius_xy=1):
  v = np.asarray(votes)
  if not supported(v.shape, k, radius_r, radius_xy):
    raise ValueError(f'vote_peaks: unsupported shape {v.shape} k={k} radius_r={radius_r} radius_xy={radius_xy}')
  R, Ho, Wo = v.shape
  flat = np.flatnonzero(peak_mask(v, radius_r, radius_xy))
  val = v.reshape(-1)[flat]
  order = np.lexsort((flat, -val))[:k]                # value descending, then flat ascending
  found = len(order)
  index = np.full((k, 3), -1, np.int32)
  score = np.full((k,), -np.inf, np.float32)
  f = flat[order]
  index[:found] = np.stack([f // (Ho * Wo), f // Wo % Ho, f % Wo], -1)
  score[:found] = val[order]
  count = np.array([found, int(np.isnan(v).sum())], np.int32)
  return index, score, count
