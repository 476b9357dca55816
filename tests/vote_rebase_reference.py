"""A float64 numpy restatement of ``snap_vote_rebase_f32`` (include/snap_hip.h), written from the contract, not from
the kernel: whole-volume arrays, eight masked taps.

The contract, restated
----------------------
``src [R, Ho, Wo]`` f32, ``table = (dk, A [2, 2], o [2])`` float64, ``scale``.

* M = the largest finite source value.  p = fl32(exp(scale (v - M))) in float64 rounded once, 0 for -inf; a NaN or
  +inf cell is counted and poisons its readers.
* Destination cell (r, a, b): k = r - dk, sa = (A00 a + A01 b) + oa, sb = (A10 a + A11 b) + ob, each split into
  floor and fraction; axis weights (1 - f, f); a tap's weight is (wk wa) wb.  These are the kernel's own float64
  expressions, so the coordinates, weights and skip decisions are the kernel's bit for bit.  A tap is skipped when
  its weight is exactly 0 or it lies outside the plane.  mass = sum weight p in the order k, a, b (float64), rounded
  to f32; NaN when a tap is a NaN / +inf cell.  S = sum of the f32 masses that are not NaN.
* dst = log(mass) - log(S) (not rounded here); -inf where the mass is 0.
* stats = (scale M + log(sum p), S / sum p (0 when sum p == 0), M, max dst); count = (finite cells of dst, NaN
  cells of dst, NaN / +inf cells of src, cells of dst with no tap).

The error bound (``bound``), derived, not measured
--------------------------------------------------
u = 2^-24.  ``all_inputs`` keeps scale (v - M) > -80 and the smallest non-zero cell mass above 2^-120 (asserted in
``_walk``), so no f32 mass is subnormal and the -inf mask is decided by geometry alone.

* p: the kernel's and numpy's float64 exp each differ from the exact value by about one float64 ulp, so the two f32
  roundings can fall to different neighbours: at most one f32 ulp = 2 u relative.
* The weights are identical and non-negative, so the float64 cell mass inherits at most 2 u relative (plus float64
  noise); its rounding to f32 can again fall to different neighbours: mass32 is off by at most 4 u (1 + 2 u) relative.
* S is a float64 sum of those masses: at most the same relative error.  log(mass) - log(S) is therefore off by at most
  -2 log(1 - 4.01 u) in absolute terms, plus float64 noise of the logarithms and the sum (n 2^-53 relative on S, a few
  2^-53 of the magnitudes: the ``_F64`` terms).
* The final rounding to f32: u |dst|.

bound = 8.04 u + f64 terms + u |dst| per finite cell.  The tests allow twice that.  ``stats_bound`` gives the same for
the four statistics (float64, so without the final rounding): log_z 2 u for sum p; mass_kept 4.01 u + 2 u relative;
M exact; the largest dst the largest cell bound.
"""
import math

import numpy as np

TILE = 16             # vote_rebase.hip: the gather's tile is TILE x TILE cells of one plane (RB_T)
TILE_1D = 256         # vote_rebase.hip: cells of a tile of the other launches (RB_NT)
MAX_GROUPS = 2048     # vote_rebase.hip: workgroups of a launch (RB_MAX_GROUPS); beyond it they stride over tiles
U = 2.0 ** -24
_F64 = 2.0 ** -50


def masses(src, scale):
  """-> (p float64 [R, Ho, Wo] holding f32 values, NaN for NaN / +inf cells; M float64; bad cells; the lowest
  scale (v - M) over the finite cells)."""
  src = np.asarray(src)
  assert src.dtype == np.float32 and src.ndim == 3
  scale = float(np.float32(scale))
  fin = np.isfinite(src)
  bad = np.isnan(src) | (src == np.inf)
  M = float(src[fin].max()) if fin.any() else -np.inf
  p = np.zeros(src.shape)
  x = scale * (src[fin].astype(np.float64) - M)
  p[fin] = np.exp(x).astype(np.float32).astype(np.float64)
  p[bad] = np.nan
  return p, M, int(bad.sum()), (x.min() if x.size else 0.0)


def coordinates(shape, table):
  """The kernel's float64 coordinate expressions -> (k [R], sa [Ho, Wo], sb [Ho, Wo])."""
  R, Ho, Wo = shape
  dk, A, o = table
  A, o = np.asarray(A, np.float64).reshape(2, 2), np.asarray(o, np.float64).reshape(2)
  a = np.arange(Ho, dtype=np.float64)[:, None]
  b = np.arange(Wo, dtype=np.float64)[None, :]
  k = np.arange(R, dtype=np.float64) - float(dk)
  sa = (A[0, 0] * a + A[0, 1] * b) + o[0]
  sb = (A[1, 0] * a + A[1, 1] * b) + o[1]
  return k, sa, sb


def gather(p, table):
  """The 8-tap blend of the masses -> (mass float64 [R, Ho, Wo] before its rounding, NaN where poisoned; any_tap bool)."""
  R, Ho, Wo = p.shape
  k, sa, sb = coordinates(p.shape, table)
  k0, ia, ib = np.floor(k), np.floor(sa), np.floor(sb)
  fk, fa, fb = k - k0, sa - ia, sb - ib
  planes = np.mod(k0.astype(np.int64), R)
  mass = np.zeros(p.shape)
  poisoned = np.zeros(p.shape, bool)
  any_tap = np.zeros(p.shape, bool)
  for kk in range(2):
    wk = (fk if kk else 1.0 - fk)[:, None, None]
    plane = (planes + kk) % R
    for da in range(2):
      wa = (fa if da else 1.0 - fa)[None]
      row = ia + da
      for db in range(2):
        wb = (fb if db else 1.0 - fb)[None]
        col = ib + db
        w = (wk * wa) * wb
        inside = ((row >= 0) & (row < Ho) & (col >= 0) & (col < Wo))[None]
        take = (w != 0.0) & inside
        rr = np.clip(row, 0, Ho - 1).astype(np.int64)
        cc = np.clip(col, 0, Wo - 1).astype(np.int64)
        v = p[plane[:, None, None], rr[None], cc[None]]
        nan = np.isnan(v)
        poisoned |= take & nan
        mass = mass + np.where(take & ~nan, w * np.where(nan, 0.0, v), 0.0)
        any_tap |= take
  return np.where(poisoned, np.nan, mass), any_tap


def _walk(src, table, scale):
  p, M, bad, lowest = masses(src, scale)
  assert lowest > -80.0, 'inputs keep scale (v - M) > -80'
  mass, any_tap = gather(p, table)
  nan = np.isnan(mass)
  pos = ~nan & (mass > 0)
  assert not pos.any() or mass[pos].min() > 2.0 ** -120, 'no f32 cell mass may be subnormal'
  m32 = np.where(nan, np.nan, mass.astype(np.float32).astype(np.float64))
  S = m32[~nan].sum()
  sum_p = p[~np.isnan(p)].sum()
  with np.errstate(divide='ignore', invalid='ignore'):
    out = np.where(nan, np.nan, np.where(m32 > 0, np.log(m32) - (math.log(S) if S > 0 else 0.0), -np.inf))
  fin = np.isfinite(out)
  scale = float(np.float32(scale))
  stats = np.array([scale * M + math.log(sum_p) if sum_p > 0 else -np.inf, S / sum_p if sum_p > 0 else 0.0, M,
                    out[fin].max() if fin.any() else -np.inf])
  count = np.array([fin.sum(), nan.sum(), bad, (~any_tap).sum()], np.int64)
  return out, stats, count, dict(fin=fin, S=S, sum_p=sum_p, m32=m32, n=out.size, M=M, scale=scale)


def vote_rebase(src, table, scale=1.0):
  """-> (dst float64 [R, Ho, Wo], stats float64 [4], count int64 [4])."""
  return _walk(src, table, scale)[:3]


_CELL = -2.0 * math.log1p(-4.01 * U)


def bound(src, table, scale=1.0):
  """The derived bound of |fl32 result - reference| per cell (module docstring); 0 where the result is not finite."""
  out, _, _, w = _walk(src, table, scale)
  fin = w['fin']
  if not fin.any():
    return np.zeros(out.shape)
  with np.errstate(invalid='ignore', divide='ignore'):
    mags = np.abs(np.log(w['m32'])) + abs(math.log(w['S']))
    b = _CELL + _F64 * mags + w['n'] * 2.0 ** -53 + U * np.abs(out)
  return np.where(fin, b, 0.0)


def stats_bound(src, table, scale=1.0):
  """Bounds of the four statistics: log_z; S / sum p; M (exact); the largest dst (the largest cell bound)."""
  out, stats, _, w = _walk(src, table, scale)
  noise = w['n'] * 2.0 ** -53
  b_lz = (-math.log1p(-2.01 * U) + noise + _F64 * (abs(stats[0]) + abs(w['scale'] * w['M']))) if np.isfinite(stats[0]) else 0.0
  b_kept = (6.02 * U + 2 * noise) * abs(stats[1]) * 1.0001
  return np.array([b_lz, b_kept, 0.0, bound(src, table, scale).max()])


# ---------------------------------------------------------------------------------------------------------------
# tables and inputs
# ---------------------------------------------------------------------------------------------------------------
def index_table(phi, shift, dk, shape, about=None):
  """A table written directly in index space: the destination reads Rot(-phi) ((a, b) - about - shift) + about, i.e.
  the source turned by ``phi`` about the index point ``about`` (default: the plane's middle) and then moved by
  ``shift`` cells.  cos / sin snapped to 0 below 2^-40 as ``rebase_table`` does."""
  _, Ho, Wo = shape
  c, s = (0.0 if abs(v) < 2.0 ** -40 else v for v in (math.cos(phi), math.sin(phi)))
  A = np.array([[c, s], [-s, c]]) + 0.0
  about = np.array([(Ho - 1) / 2, (Wo - 1) / 2]) if about is None else np.asarray(about, np.float64)
  o = (about - A @ (about + np.asarray(shift, np.float64))) + 0.0
  return float(dk), A, o


IDENTITY = (0.0, np.eye(2), np.zeros(2))


def border_mask(Ho, Wo):
  """The low-overlap border of a vote volume of a (Ho + 1) / 2 x (Wo + 1) / 2 query on its own map: True = kept."""
  H, W = (Ho + 1) // 2, (Wo + 1) // 2
  oa = (H - np.abs(np.arange(Ho) - (H - 1))).astype(np.float64)
  ob = (W - np.abs(np.arange(Wo) - (W - 1))).astype(np.float64)
  return oa[:, None] * ob[None, :] > 0.05 * H * W


def _volume(rng, shape, masked=0.0, border=False):
  """Log scores within 24 of their peak: a smooth bump plus noise."""
  R, Ho, Wo = shape
  k, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Wo), indexing='ij')
  c = (rng.uniform(0, R), rng.uniform(0, Ho), rng.uniform(0, Wo))
  dk = (k - c[0] + R / 2) % R - R / 2
  x = -(dk ** 2 / (2 * max(R / 4, 1) ** 2) + ((a - c[1]) ** 2 + (b - c[2]) ** 2) / (2 * (max(Ho, Wo) / 3) ** 2))
  x = np.clip(x * 2.0 + rng.standard_normal(shape) * 0.5, -10.0, None).astype(np.float32) - np.float32(3)
  if masked:
    x[rng.random(shape) < masked] = -np.inf
  if border:
    x[:, ~border_mask(Ho, Wo)] = -np.inf
  return x


def _case(name, src, table, scale=1.0):
  return dict(name=name, src=src, table=table, scale=scale)


def all_inputs():
  """-> list of case dicts (name, src, table, scale); seeded: the same arrays in every process."""
  rng = np.random.default_rng(20261020)
  cases = [_case('tiny', np.array([[[-3.5]]], np.float32), IDENTITY, 2.0)]
  shape = (36, 31, 33)
  v = _volume(rng, shape, masked=0.30, border=True)
  ragged = index_table(0.37, (1.3, -2.6), 35.25, shape)
  cases.append(_case('identity', v, IDENTITY, 2.0))
  cases.append(_case('shift', v, index_table(0.0, (2, -3), 0.0, shape), 2.0))
  cases.append(_case('ragged', v, ragged, 2.0))
  cases.append(_case('scale', v, ragged, 0.5))
  # a quarter turn: about the lattice's middle (a permutation of every plane) and about the point half a cell from it
  # that is the map centre (index extent - 1.5: one row leaves, one is not covered)
  q = _volume(rng, (8, 15, 15), masked=0.2)
  cases.append(_case('quarter', q, index_table(math.pi / 2, (0, 0), 6.0, q.shape, about=(6.5, 6.5))))
  cases.append(_case('quarter_lattice', q, index_table(math.pi / 2, (0, 0), 6.0, q.shape)))
  # dk within 1e-9 of R and of 0, from both sides (and exactly 0 with the turn)
  w = _volume(rng, (4, 7, 7))
  for name, dk in (('wrap_below_R', 4 - 1e-9), ('wrap_above_0', 1e-9), ('wrap_below_1', 1 - 1e-9),
                   ('wrap_above_3', 3 + 1e-9)):
    cases.append(_case(name, w, index_table(0.2, (0.4, -0.7), dk, w.shape)))
  # a NaN and a +inf source cell: under the identity exactly those two cells are NaN
  v2 = v.copy()
  v2[3, 10, 11], v2[30, 20, 5] = np.nan, np.inf
  cases.append(_case('bad_identity', v2, IDENTITY, 2.0))
  cases.append(_case('bad_ragged', v2, ragged, 2.0))
  # a translation larger than the volume
  cases.append(_case('gone', v, index_table(0.0, (40, 0), 0.0, shape), 2.0))
  # planes one cell high and one cell wide
  for name, shape_t in (('thin_row', (4, 1, 300)), ('thin_col', (4, 300, 1))):
    t = _volume(rng, shape_t)
    cases.append(_case(name, t, index_table(0.0, (0.0, 17.4) if shape_t[1] == 1 else (-8.3, 0.0), 1.5, shape_t)))
    cases.append(_case(name + '_turned', t, index_table(0.3, (0.2, 0.1), 1.5, shape_t)))
  # more gather tiles than workgroups, and more 1-D tiles too: every launch strides and every fold of the partials
  # has more entries than one pass of its 256 threads
  shape = (2, 520, 520)
  assert 2 * (-(-520 // TILE)) ** 2 > MAX_GROUPS and 2 * -(-520 * 520 // TILE_1D) > MAX_GROUPS
  cases.append(_case('tiles', _volume(rng, shape, masked=0.1, border=True), index_table(0.37, (5.3, -7.6), 0.4, shape), 2.0))
  return cases
