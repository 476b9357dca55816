"""float64 numpy restatement of the contract of snap_vote_credible_f32 (include/snap_hip.h) BY FULL SORT, the error
bound of the kernel's selection arithmetic, the gap that makes a threshold decidable, and the inputs the tests share.

Written from the header's comment; imports nothing of the package.

  votes [R, Ho, Wo] f32, flat(r, a, b) = (r * Ho + a) * Wo + b.  F = the finite cells (-inf masked, NaN / +inf excluded
  and counted); vmax = max_F v; w = exp(float64(scale) * (float64(v) - float64(vmax))); Z = sum_F w.  The order of cells
  is the f32 order of the votes, -0 = +0.  Region l = {v >= tau_l}, tau_l = the largest vote value t of F with
  mass{v >= t} >= q_l Z (q_l = the level rounded to f32): stable descending sort, cumsum, and the cumulative mass read
  at the END of every class of tied values, so a class is in or out as a whole.  level(cell) = the smallest l with
  v >= tau_l, L if none or the cell is not in F.
  Outputs: threshold [L] (f32, exactly a vote value), mass [L] = mass{v >= tau_l} / Z, table [L, 8] = (cells, pixels,
  rotations, a_min, a_max, b_min, b_max, 0), level_xy [Ho, Wo] / level_r [R] / level_cell [R, Ho, Wo] uint8,
  gt_stats [4] = (v_gt, mass{v > v_gt} / Z, mass{v >= v_gt} / Z, 0), count [4] = (|F|, NaN or +inf cells, gt valid,
  gt level or -1).  The ground-truth cell is (rint(k) mod R, rint(i), rint(j)), valid iff k, i, j are finite,
  |k| <= 2^20, 0 <= i <= Ho-1, 0 <= j <= Wo-1 and the cell is in F.  F empty: NaN thresholds and masses, table rows
  (0, 0, 0, -1, -1, -1, -1, 0), level maps all L.

THE KERNEL'S METHOD AND ITS EPSILON (``bound``).  Six passes over the volume for every L: the maximum, four 8-bit digit
passes of a radix select over the monotone key of the vote, and the level pass.  The digit passes bin FIXED-POINT
weights wfix = rint(w 2^Q), Q = 62 - bit_length(R Ho Wo), with integer atomics (LDS, then global bins): exact sums.
Every cell is off by at most half a quantum, so a cumulative mass and the target q Zfix are each off by at most R Ho Wo 2^-(Q+1): the
selection decides "mass{v >= t} >= q Z" correctly whenever |mass{v >= t} / Z - q| exceeds
    eps = R Ho Wo 2^-Q / Z   (+ SLOP = 2^-40 for the float64 exp, products and conversions).
The masses that are RETURNED are float64 sums of float64 weights in a fixed order: their error (<= R Ho Wo 2^-53
relative) is far inside eps, so the same eps bounds them.  ``gap`` is, over the levels, the smaller distance from q to
the normalised cumulative mass at tau and to the one just above tau: with gap >= max(4 eps, 1e-9) the threshold is
decided beyond the kernel's arithmetic and the GPU test may demand EQUAL thresholds, tables and level maps.
"""
import functools

import numpy as np

SLOP = 2.0 ** -40
MAX_L = 8
LEVELS3 = (0.5, 0.9, 0.99)
LEVELS1 = (0.9,)
LEVELS8 = (0.1, 0.25, 0.5, 0.68, 0.9, 0.95, 0.99, 0.999)


def _f32_levels(levels):
  q = np.asarray(levels, np.float32).reshape(-1)
  if not (1 <= q.size <= MAX_L and (q > 0).all() and (q < 1).all() and (np.diff(q) > 0).all()):
    raise ValueError(f'vote_credible: levels {levels}')
  return q.astype(np.float64)


def _weights(v, scale):
  """(F mask, canonical f32 values of F, float64 weights of F, vmax)."""
  v = np.asarray(v)
  assert v.dtype == np.float32 and v.ndim == 3
  scale = np.float32(scale)
  if not (np.isfinite(scale) and scale > 0):
    raise ValueError(f'vote_credible: scale {scale}')
  F = np.isfinite(v)
  vals = v[F] + np.float32(0)                                  # -0 -> +0
  if vals.size == 0:
    return F, vals, np.zeros(0), np.float32(-np.inf)
  vmax = vals.max()
  w = np.exp(np.float64(scale) * (vals.astype(np.float64) - np.float64(vmax)))
  return F, vals, w, vmax


def _classes(vals, w):
  """Descending tie classes -> (class values f32 [K], cumulative mass at the END of each class f64 [K], Z)."""
  order = np.argsort(-vals, kind='stable')
  sv, cs = vals[order], np.cumsum(w[order])
  ends = np.flatnonzero(np.r_[sv[1:] != sv[:-1], True])
  return sv[ends], cs[ends], cs[-1]


def _gt_cell(shape, gt_index):
  R, Ho, Wo = shape
  if gt_index is None:
    return None
  k, i, j = (np.float32(c) for c in gt_index)
  if not (np.isfinite(k) and np.isfinite(i) and np.isfinite(j)):
    return None
  if not (abs(k) <= 2 ** 20 and 0 <= i <= Ho - 1 and 0 <= j <= Wo - 1):
    return None
  return int(np.rint(k)) % R, int(np.rint(i)), int(np.rint(j))  # np.rint: half to even


def vote_credible(votes, levels, scale=1.0, gt_index=None):
  """-> (threshold f32 [L], mass f64 [L], table int32 [L, 8], level_xy u8, level_r u8, level_cell u8, gt_stats f64
  [4], count int32 [4])."""
  v = np.asarray(votes)
  q = _f32_levels(levels)
  L = q.size
  R, Ho, Wo = v.shape
  F, vals, w, _ = _weights(v, scale)
  count = np.array([int(F.sum()), int((np.isnan(v) | (v == np.inf)).sum()), 0, -1], np.int32)
  gt_stats = np.array([np.nan, np.nan, np.nan, 0.0])
  table = np.tile(np.array([0, 0, 0, -1, -1, -1, -1, 0], np.int32), (L, 1))
  level_cell = np.full(v.shape, L, np.uint8)
  if vals.size == 0:
    return (np.full(L, np.nan, np.float32), np.full(L, np.nan), table, np.full((Ho, Wo), L, np.uint8),
            np.full(R, L, np.uint8), level_cell, gt_stats, count)
  cv, cc, Z = _classes(vals, w)
  pick = np.minimum(np.searchsorted(cc, q * Z, side='left'), len(cc) - 1)
  threshold, mass = cv[pick].astype(np.float32), cc[pick] / Z
  with np.errstate(invalid='ignore'):
    lev = (np.where(F, v, np.float32(0))[..., None] < threshold).sum(-1)
  level_cell = np.where(F, lev, L).astype(np.uint8)
  level_xy, level_r = level_cell.min(0), level_cell.reshape(R, -1).min(1)
  for l in range(L):
    inside = level_xy <= l
    aa, bb = np.nonzero(inside)
    table[l] = (int((level_cell <= l).sum()), int(inside.sum()), int((level_r <= l).sum()), aa.min(), aa.max(),
                bb.min(), bb.max(), 0)
  cell = _gt_cell(v.shape, gt_index)
  if cell is not None and F[cell]:
    vgt = v[cell]
    gt_stats[:3] = (vgt, w[vals > vgt].sum() / Z, w[vals >= vgt].sum() / Z)
    count[2], count[3] = 1, int((vgt < threshold).sum())
  return threshold, mass, table, level_xy, level_r, level_cell, gt_stats, count


def credibility_of_cells(votes, scale=1.0):
  """mass{v > v_c} / Z for EVERY cell c (NaN outside F) -> f64 [R, Ho, Wo]: the ground-truth credibility of each cell."""
  v = np.asarray(votes)
  F, vals, w, _ = _weights(v, scale)
  cv, cc, Z = _classes(vals, w)
  above = np.r_[0.0, cc[:-1]] / Z                              # per class, descending
  idx = np.searchsorted(-cv, -vals, side='left')
  out = np.full(v.shape, np.nan)
  out[F] = above[idx]
  return out


def bound(votes, scale=1.0):
  """eps of the kernel's selection arithmetic (module docstring), a function of the input alone."""
  v = np.asarray(votes)
  _, vals, w, _ = _weights(v, scale)
  if vals.size == 0:
    return 0.0
  Q = 62 - int(v.size).bit_length()
  return v.size * 2.0 ** -Q / float(w.sum()) + SLOP


def gap(votes, scale, levels):
  """Over all levels, the smaller distance from q to the normalised cumulative mass at tau and to the one just above
  tau (0 mass above the first class).  inf for an empty F."""
  q = _f32_levels(levels)
  _, vals, w, _ = _weights(votes, scale)
  if vals.size == 0:
    return np.inf
  _, cc, Z = _classes(vals, w)
  pick = np.minimum(np.searchsorted(cc, q * Z, side='left'), len(cc) - 1)
  at = cc[pick] / Z
  above = np.where(pick > 0, cc[np.maximum(pick - 1, 0)], 0.0) / Z
  return float(np.minimum(np.abs(at - q), np.abs(q - above)).min())


# ---- the inputs the CPU and GPU tests share -------------------------------------------------------------------------
SHAPES = [(3, 1, 1), (1, 5, 5), (4, 7, 7), (36, 31, 33), (64, 5, 300), (2, 520, 520)]
PEAK_SHAPE = (8, 200, 210)


def smooth_votes(shape, seed=0, modes=3):
  """Multi-modal log-scores: the maximum of ``modes`` Gaussian bumps (heights 0.2 .. 1, so 0 lies among the high
  values) in (r circular, a, b), plus a little noise that breaks the ties."""
  R, Ho, Wo = shape
  rng = np.random.default_rng(seed + 13 * sum(shape))
  r = np.arange(R, dtype=np.float64)[:, None, None]
  a = np.arange(Ho, dtype=np.float64)[None, :, None]
  b = np.arange(Wo, dtype=np.float64)[None, None, :]
  sa, sb, sr = max(1.0, Ho / 6), max(1.0, Wo / 6), max(0.7, R / 8)
  out = np.full(shape, -np.inf)
  for _ in range(modes):
    cr, ca, cb, amp = rng.uniform(0, R), rng.uniform(0, Ho - 1), rng.uniform(0, Wo - 1), rng.uniform(0.2, 1.0)
    dr = np.minimum(np.abs(r - cr), R - np.abs(r - cr))
    out = np.maximum(out, amp - (a - ca) ** 2 / (2 * sa ** 2) - (b - cb) ** 2 / (2 * sb ** 2) - dr ** 2 / (2 * sr ** 2))
  return (out + 0.05 * rng.standard_normal(shape)).astype(np.float32)


def dirty_votes(shape, seed=0):
  """``smooth_votes`` with 30 % of the cells -inf, a few NaN / +inf cells and a (-0, +0) pair of tied cells."""
  rng = np.random.default_rng(seed + 17 * sum(shape))
  v = smooth_votes(shape, seed)
  flat = v.reshape(-1)
  flat[rng.random(flat.size) < 0.3] = -np.inf
  cells = rng.permutation(flat.size)[:7]
  flat[cells[0]], flat[cells[1]], flat[cells[2]] = np.nan, np.inf, np.nan
  flat[cells[3]], flat[cells[4]] = np.inf, np.nan
  flat[cells[5]], flat[cells[6]] = np.float32(-0.0), np.float32(0.0)
  return v


def tie_votes(shape, seed=0):
  """``smooth_votes`` quantised to the integers 0 .. 5, 10 % masked: six heavy tie classes."""
  rng = np.random.default_rng(seed + 19 * sum(shape))
  s = smooth_votes(shape, seed).astype(np.float64)
  lo, hi = s.min(), s.max()
  v = np.rint((s - lo) / (hi - lo) * 5).astype(np.float32)
  v[rng.random(shape) < 0.1] = -np.inf
  return v


def tie_levels(votes, scale, L=3):
  """Levels for ``tie_votes``: inside the heaviest tie class at 0.3 and 0.7 of its mass (two levels, one class: equal
  tau, equal regions) and, for L = 3, the middle of a neighbouring class (deep inside it); for L = 8, eight levels
  spread over the heaviest class and its neighbour.  Rounded to f32."""
  _, vals, w, _ = _weights(votes, scale)
  _, cc, Z = _classes(vals, w)
  c = np.r_[0.0, cc / Z]
  own = np.diff(c)
  j = int(np.argmax(own))
  n = j + 1 if j + 1 < len(own) and own[j + 1] > 1e-4 else j - 1
  inside = lambda k, f: c[k] + f * own[k]
  if L == 1:
    q = [inside(j, 0.5)]
  elif L == 3:
    q = [inside(j, 0.3), inside(j, 0.7), inside(n, 0.5)]
  else:
    q = [inside(j, f) for f in (0.1, 0.3, 0.5, 0.7, 0.9)] + [inside(n, f) for f in (0.25, 0.5, 0.75)]
  q = np.sort(np.asarray(q, np.float32))
  assert (np.diff(q) > 0).all() and q[0] > 0 and q[-1] < 1
  return tuple(float(x) for x in q)


def equal_votes(shape, seed=0):
  """Votes in {0, -inf}: one tie class, every tau = 0, every region = F."""
  rng = np.random.default_rng(seed + 11 * sum(shape))
  v = np.where(rng.random(shape) < 0.4, np.float32(0), np.float32(-np.inf)).astype(np.float32)
  v.reshape(-1)[-1] = 0
  return v


def peak_votes(shape=PEAK_SHAPE):
  """A sharp Gaussian log-score in the far corner, sigma 0.7 cells, the same in every rotation (8-fold ties): region 0
  is a handful of cells."""
  R, Ho, Wo = shape
  a, b = np.arange(Ho, dtype=np.float64)[:, None], np.arange(Wo, dtype=np.float64)[None, :]
  x = -((a - (Ho - 1.3)) ** 2 + (b - (Wo - 1.6)) ** 2) / (2 * 0.7 ** 2)
  return np.broadcast_to(x.astype(np.float32), shape).copy()


GT_SHAPE = (36, 31, 33)


@functools.lru_cache(maxsize=None)
def gt_cases():
  """(votes, levels, scale, [(name, (k, i, j), the cell it names (written out here) or None = invalid)]) on the
  dirty volume: a cell centre inside region 0, between regions and outside all; half-way indices (half to even); the
  two wraps of k and one 29127 turns away; a masked cell; out of range; non-finite."""
  v = dirty_votes(GT_SHAPE, seed=3)
  R, Ho, Wo = GT_SHAPE
  lev = vote_credible(v, LEVELS3, 1.0)[5]
  first = lambda mask: tuple(int(x) for x in np.argwhere(mask)[0])
  fl = lambda c: tuple(float(x) for x in c)
  in0, between, outside = first(lev == 0), first((lev == 1) | (lev == 2)), first((lev == 3) & np.isfinite(v))
  masked = first(v == -np.inf)
  even = tuple(2 * x for x in first(np.isfinite(v[::2, ::2, ::2])))   # x + 0.5 rounds DOWN to an even x
  up = tuple(2 * x + 2 for x in first(np.isfinite(v[2::2, 2::2, 2::2])))   # another even, contributing cell
  odd = tuple(x - 1 for x in up)                                          # x + 0.5 rounds UP to the even x + 1
  fin = first(np.isfinite(v[0]))                           # a contributing cell of rotation 0, for the wraps
  cases = [('centre', fl(in0), in0), ('between', fl(between), between), ('outside', fl(outside), outside),
           ('half_even_down', tuple(x + 0.5 for x in even), even),
           ('half_even_up', tuple(x + 0.5 for x in odd), tuple(x + 1 for x in odd)),
           ('wrap_neg', (-0.4, float(fin[0]), float(fin[1])), (0,) + fin),
           ('wrap_top', (R - 0.4, float(fin[0]), float(fin[1])), (0,) + fin),
           ('wrap_far', (-36.0 * 29127, float(fin[0]), float(fin[1])), (0,) + fin),
           ('masked', fl(masked), None), ('too_far_k', (float(2 ** 20 + 36), 3.0, 3.0), None),
           ('negative_i', (1.0, -0.25, 3.0), None), ('past_last_j', (1.0, 3.0, Wo - 0.75), None),
           ('nan', (np.nan, 3.0, 3.0), None), ('inf', (1.0, np.inf, 3.0), None)]
  return v, LEVELS3, 1.0, cases


@functools.lru_cache(maxsize=None)
def all_inputs():
  """[(name, votes, scale, levels, gt_index)]: every input of the GPU tests that is compared with equality."""
  out = []
  for shape in SHAPES:
    out.append(('smooth%s_s1_L3' % (shape,), smooth_votes(shape), 1.0, LEVELS3, None))
    out.append(('equal%s_s1_L3' % (shape,), equal_votes(shape), 1.0, LEVELS3, None))
  for shape in SHAPES[2:]:
    out.append(('dirty%s_s4_L3' % (shape,), dirty_votes(shape), 4.0, LEVELS3, None))
    for scale, L in ((1.0, 3), (4.0, 8)):
      v = tie_votes(shape)
      out.append(('ties%s_s%g_L%d' % (shape, scale, L), v, scale, tie_levels(v, scale, L), None))
  for scale in (1.0, 4.0):
    for lv in (LEVELS1, LEVELS8):
      out.append(('smooth%s_s%g_L%d' % (GT_SHAPE, scale, len(lv)), smooth_votes(GT_SHAPE), scale, lv, None))
  out.append(('dirty%s_s1_L8' % (GT_SHAPE,), dirty_votes(GT_SHAPE), 1.0, LEVELS8, None))
  out.append(('smooth%s_s4_L8' % (SHAPES[-1],), smooth_votes(SHAPES[-1]), 4.0, LEVELS8, None))
  out.append(('ties%s_s1_L1' % (GT_SHAPE,), tie_votes(GT_SHAPE), 1.0, tie_levels(tie_votes(GT_SHAPE), 1.0, 1), None))
  out.append(('equal%s_s4_L8' % (GT_SHAPE,), equal_votes(GT_SHAPE), 4.0, LEVELS8, None))
  out.append(('peak_s1_L3', peak_votes(), 1.0, LEVELS3, None))
  out.append(('peak_s4_L8', peak_votes(), 4.0, LEVELS8, None))
  for shape in ((3, 1, 1), GT_SHAPE):
    out.append(('masked%s' % (shape,), np.full(shape, -np.inf, np.float32), 1.0, LEVELS3, None))
  v, levels, scale, cases = gt_cases()
  for name, idx, _ in cases:
    out.append(('gt_' + name, v, scale, levels, idx))
  return out
