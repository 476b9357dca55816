"""A float64 numpy restatement of ``snap_vote_filter_f32`` (include/snap_hip.h), written from the contract, not from
the kernel: plain slices over whole planes, one rotation at a time.

The contract, restated
----------------------
``belief [R, Ho, Wo]`` f32 or None, ``votes [R, Ho, Wo]`` f32, ``taps = (taps_k [Tk], lk, taps_a [R, Ta],
taps_b [R, Tb], offsets [R, 2] = (la, lb))``, ``scale``, ``uniform_mix`` = eps, n = R Ho Wo.

* M = the largest finite belief.  NaN / +inf cells: no mass, counted.  d = fl32(belief - M); the cell has the mass
  p = fl32(exp(float64(d))) iff d >= -40, else 0.  These three f32 decisions are reproduced exactly.
* t0[r, a, b] = sum_tk taps_k[tk] p[(r + lk + tk) mod R, a, b]; t1[r, a, b] = sum_ta taps_a[r, ta] t0[r, a + la[r] +
  ta, b]; t2[r, a, b] = sum_tb taps_b[r, tb] t1[r, a, b + lb[r] + tb]; sources outside the volume contribute 0.
  Here the sums are float64 (every product of two f32 numbers is exact); the kernel's are f32 fma chains.
* S = sum t2.  prior = ((1 - eps) t2) / S + eps / n (first term 0 when S == 0 or belief is None, where eps acts as 1);
  u = scale * votes + log(prior); -inf vote -> -inf; NaN / +inf vote -> NaN; log_z = logsumexp over the finite u;
  belief_out = u - log_z (not rounded here).
* stats = (log_z, S / sum p (1 without a belief, 0 when sum p == 0), M (-inf without a belief), max belief_out);
  count = (finite cells of belief_out, NaN / +inf cells of belief, NaN cells of belief_out, cells of belief with mass).

The error bound (``bound``), derived, not measured
--------------------------------------------------
u = 2^-24, every f32 operation rounds to nearest, the taps obey the contract's precondition (finite, >= 0, either 0 or
>= 2^-20), so with p >= e^-40 no product or partial sum is subnormal and all terms are non-negative (no cancellation).

* p: the kernel's and numpy's float64 exp each differ from the exact value by about one float64 ulp, so the two f32
  roundings can fall to different neighbours: at most one f32 ulp = 2 u relative.  c = 2.
* A term taps_b * taps_a * taps_k * p passes through at most Tk roundings of the k chain (the store of t0 is the
  chain's last fma), Ta of the row chain and Tb of the column chain: t2 = exact * (1 + delta)^m, m = Tk + Ta + Tb + c,
  relative error at most g = m u / (1 - m u).
* S is a float64 sum of those t2: relative error at most g (plus float64 noise).  So the transported term
  A = (1 - eps) t2 / S has relative error at most rho = 2 g / (1 - g), the uniform term B = eps / n none, and
  log(prior) = log(A + B) an absolute error of at most -log(1 - rho A / (A + B)).
* scale * votes is exact in float64 (two f32 factors); the sum u, log_z's fold over n cells and the subtraction are
  float64: n 2^-53 relative on exp-sums plus a few 2^-53 of the magnitudes, added as ``_F64`` terms.
* log_z is a logsumexp of values each off by at most e_cell: it is off by at most max e_cell.
* The final rounding to f32: u |belief_out|.

bound = e_cell + max e_cell + f64 terms + u |belief_out| per finite cell.  The tests allow twice that.
``stats_bound`` gives the same for the four statistics.
"""
import math

import numpy as np

TILE = 256            # vote_filter.hip: cells of a tile (FL_NT)
MAX_GROUPS = 2048     # vote_filter.hip: workgroups of a launch (FL_MAX_GROUPS); beyond it they stride over tiles
CUT = np.float32(-40.0)
MIN_TAP = 2.0 ** -20
U = 2.0 ** -24
_F64 = 2.0 ** -50


def masses(belief):
  """-> (p float64 [R, Ho, Wo] holding f32 values, M f32, bad cells, cells with mass): the f32 decisions, exactly."""
  belief = np.asarray(belief)
  assert belief.dtype == np.float32
  fin = np.isfinite(belief)
  bad = int((np.isnan(belief) | (belief == np.inf)).sum())
  if not fin.any():
    return np.zeros(belief.shape), np.float32(-np.inf), bad, 0
  M = belief[fin].max()
  with np.errstate(invalid='ignore'):
    d = (belief - M).astype(np.float32)                     # one f32 subtraction
  has = fin & (d >= CUT)
  p = np.zeros(belief.shape)
  p[has] = np.exp(d[has].astype(np.float64)).astype(np.float32).astype(np.float64)
  return p, M, bad, int(has.sum())


def predict(p, taps):
  """The three passes on the masses, float64 -> t2 [R, Ho, Wo]."""
  taps_k, lk, taps_a, taps_b, offsets = taps
  taps_k, taps_a, taps_b = (np.asarray(t, np.float32).astype(np.float64) for t in (taps_k, taps_a, taps_b))
  offsets = np.asarray(offsets, np.int64)
  R, Ho, Wo = p.shape
  t0 = np.zeros_like(p)
  for r in range(R):
    for tk in range(len(taps_k)):
      t0[r] += taps_k[tk] * p[(r + int(lk) + tk) % R]
  t1 = np.zeros_like(p)
  t2 = np.zeros_like(p)
  for r in range(R):
    la, lb = int(offsets[r, 0]), int(offsets[r, 1])
    for ta in range(taps_a.shape[1]):
      s = la + ta                                           # t1[a] += w * t0[a + s]
      a0, a1 = max(0, -s), min(Ho, Ho - s)
      if a0 < a1:
        t1[r, a0:a1] += taps_a[r, ta] * t0[r, a0 + s:a1 + s]
    for tb in range(taps_b.shape[1]):
      s = lb + tb
      b0, b1 = max(0, -s), min(Wo, Wo - s)
      if b0 < b1:
        t2[r, :, b0:b1] += taps_b[r, tb] * t1[r, :, b0 + s:b1 + s]
  return t2


def _logsumexp(x):
  """float64 logsumexp of a 1-D array of finite numbers (-inf when empty)."""
  if x.size == 0:
    return -np.inf
  m = x.max()
  return m + math.log(np.exp(x - m).sum())


def _walk(belief, votes, taps, scale, uniform_mix):
  votes = np.asarray(votes)
  assert votes.dtype == np.float32 and votes.ndim == 3
  n = votes.size
  scale, eps = float(np.float32(scale)), float(np.float32(uniform_mix))
  if belief is None:
    t2, M, bad, mass, kept, S = np.zeros(votes.shape), np.float32(-np.inf), 0, 0, 1.0, 0.0
    A = np.zeros(votes.shape)
    B = 1.0 / n
  else:
    p, M, bad, mass = masses(belief)
    t2 = predict(p, taps)
    S, sum_p = t2.sum(), p.sum()
    kept = S / sum_p if sum_p > 0 else 0.0
    A = ((1.0 - eps) * t2) / S if S > 0 else np.zeros(votes.shape)
    B = eps / n
  prior = A + B
  v = votes.astype(np.float64)
  with np.errstate(divide='ignore', invalid='ignore'):
    u = scale * v + np.log(prior)
  bad_vote = np.isnan(v) | (v == np.inf)
  u = np.where(bad_vote, np.nan, np.where((v == -np.inf) | (prior == 0), -np.inf, u))
  fin = np.isfinite(u)
  log_z = _logsumexp(u[fin])
  with np.errstate(invalid='ignore'):
    out = np.where(fin, u - log_z, u)
  stats = np.array([log_z, kept, float(M), out[fin].max() if fin.any() else -np.inf])
  count = np.array([fin.sum(), bad, np.isnan(out).sum(), mass], np.int64)
  return out, stats, count, dict(A=A, B=B, v=v, scale=scale, prior=prior, fin=fin, log_z=log_z, n=n)


def vote_filter(belief, votes, taps, scale=1.0, uniform_mix=0.0):
  """-> (belief_out float64 [R, Ho, Wo], stats float64 [4], count int64 [4])."""
  return _walk(belief, votes, taps, scale, uniform_mix)[:3]


def _gamma(taps):
  m = len(taps[0]) + np.asarray(taps[2]).shape[1] + np.asarray(taps[3]).shape[1] + 2
  return m * U / (1 - m * U)


def _cell_error(belief, taps, w):
  """e_cell [R, Ho, Wo] (0 where the cell is not finite): the absolute error of log(prior)."""
  if belief is None:
    return np.zeros(w['v'].shape)
  g = _gamma(taps)
  rho = 2 * g / (1 - g)
  with np.errstate(divide='ignore', invalid='ignore'):
    share = np.where(w['prior'] > 0, w['A'] / w['prior'], 0.0)
  return np.where(w['fin'], -np.log1p(-rho * share), 0.0)


def bound(belief, votes, taps, scale=1.0, uniform_mix=0.0):
  """The derived bound of |fl32 result - reference| per cell (module docstring); 0 where the result is not finite."""
  out, _, _, w = _walk(belief, votes, taps, scale, uniform_mix)
  e = _cell_error(belief, taps, w)
  fin = w['fin']
  if not fin.any():
    return np.zeros(out.shape)
  with np.errstate(invalid='ignore', divide='ignore'):
    mags = np.abs(w['scale'] * w['v']) + np.abs(np.log(w['prior'])) + abs(w['log_z'])
    f64 = _F64 * mags + w['n'] * 2.0 ** -53
    b = e + e.max() + f64 + U * np.abs(out)
  return np.where(fin, b, 0.0)


def stats_bound(belief, votes, taps, scale=1.0, uniform_mix=0.0):
  """Bounds of the four statistics: log_z (max e_cell, f64 noise, the f32 rounding); S / sum p (g for S, 2 u for
  sum p, the quotient's rounding); M (exact); the largest belief_out (the largest cell bound)."""
  out, stats, _, w = _walk(belief, votes, taps, scale, uniform_mix)
  e = _cell_error(belief, taps, w)
  g = 0.0 if belief is None else _gamma(taps)
  lz = stats[0]
  b_lz = (e.max() + w['n'] * 2.0 ** -53 + (_F64 + U) * abs(lz)) if np.isfinite(lz) else 0.0
  b_kept = ((g + 2 * U) / (1 - 2 * U) + U) * abs(stats[1]) * 1.0001
  cell = bound(belief, votes, taps, scale, uniform_mix)
  return np.array([b_lz, b_kept, 0.0, cell.max()])


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def rand_taps(rng, rows, T, zeros=0.0):
  """[rows, T] f32 rows that obey the tap precondition: entries 0 (a share ``zeros`` of them, never a whole row) or
  >= 2^-20, each row summing to 1 within f32 rounding."""
  w = rng.uniform(0.05, 1.0, (rows, T))
  if zeros > 0 and T > 1:
    drop = rng.random((rows, T)) < zeros
    drop[:, 0] = False
    w[drop] = 0.0
  w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
  assert ((w == 0) | (w >= MIN_TAP)).all()
  return w


def border_mask(Ho, Wo):
  """The low-overlap border of a vote volume of a (Ho + 1) / 2 x (Wo + 1) / 2 query on its own map: True = kept."""
  H, W = (Ho + 1) // 2, (Wo + 1) // 2
  oa = (H - np.abs(np.arange(Ho) - (H - 1))).astype(np.float64)
  ob = (W - np.abs(np.arange(Wo) - (W - 1))).astype(np.float64)
  return oa[:, None] * ob[None, :] > 0.05 * H * W


def _belief(rng, shape, masked=0.0, spread=6.0):
  """A normalised-looking log belief: a smooth bump plus noise, most cells within the cut, some below it."""
  R, Ho, Wo = shape
  k, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Wo), indexing='ij')
  c = (rng.uniform(0, R), rng.uniform(0, Ho), rng.uniform(0, Wo))
  dk = (k - c[0] + R / 2) % R - R / 2
  x = -(dk ** 2 / (2 * max(R / 4, 1) ** 2) + ((a - c[1]) ** 2 + (b - c[2]) ** 2) / (2 * (max(Ho, Wo) / 3) ** 2))
  x = x * spread + rng.standard_normal(shape) * 2 - 11.0
  x = x.astype(np.float32)
  x[rng.random(shape) < 0.02] -= np.float32(45)             # below the cut
  if masked:
    x[rng.random(shape) < masked] = -np.inf
  return x


def _case(name, belief, votes, taps, scale=1.0, uniform_mix=0.0):
  return dict(name=name, belief=belief, votes=votes, taps=taps, scale=scale, uniform_mix=uniform_mix)


def exact_case():
  """Every quantity of the predict step is exact in f32: beliefs in {0, -inf} (masses 1 / 0), taps that are powers of
  two, integer shifts of both signs, the k wrap.  eps = 0, scale = 1, votes 0: belief_out = log(t2 / S), and t2, S are
  the reference's bit for bit, so the kernel's result is the reference's float64 expression rounded once."""
  rng = np.random.default_rng(7)
  R, Ho, Wo = 4, 9, 11
  belief = np.where(rng.random((R, Ho, Wo)) < 0.4, 0.0, -np.inf).astype(np.float32)
  taps_k = np.array([0.25, 0.5, 0.25], np.float32)
  taps_a = np.tile(np.array([0.5, 0.5], np.float32), (R, 1))
  taps_b = np.tile(np.array([0.125, 0.75, 0.125], np.float32), (R, 1))
  offsets = np.array([[-2, 1], [0, -1], [1, 0], [-1, -3]], np.int32)
  votes = np.zeros((R, Ho, Wo), np.float32)
  return _case('exact', belief, votes, (taps_k, -1, taps_a, taps_b, offsets))


def all_inputs():
  """-> list of case dicts (name, belief, votes, taps, scale, uniform_mix); seeded: the same arrays in every process."""
  rng = np.random.default_rng(20261019)
  cases = []
  one = lambda R: np.ones((R, 1), np.float32)
  # the smallest volume, one tap per axis
  cases.append(_case('tiny', np.array([[[-3.5]]], np.float32), np.array([[[0.75]]], np.float32),
                     (np.ones(1, np.float32), 0, one(1), one(1), np.zeros((1, 2), np.int32)), 2.0, 0.0))
  # the k wrap from both sides; lk beyond R
  shape = (4, 7, 7)
  b, v = _belief(rng, shape), rng.standard_normal(shape).astype(np.float32)
  tk, ta, tb = rand_taps(rng, 1, 3)[0], rand_taps(rng, 4, 2), rand_taps(rng, 4, 2)
  off = rng.integers(-2, 2, (4, 2)).astype(np.int32)
  cases.append(_case('wrap', b, v, (tk, -1, ta, tb, off), 1.0, 1e-3))
  cases.append(_case('wrap_far', b, v, (tk, 4 + 2, ta, tb, off), 1.0, 1e-3))
  cases.append(_case('wrap_neg', b, v, (tk, -4 * 3 - 2, ta, tb, off), 1.0, 1e-3))
  # ragged tiles, Ho != Wo, per-rotation offsets of both signs, two rotations whose taps all fall outside, 30 % -inf
  # in the belief, the border mask in the votes
  shape = (36, 31, 33)
  b = _belief(rng, shape, masked=0.30)
  v = (rng.standard_normal(shape) * 0.25).astype(np.float32)
  v[:, ~border_mask(31, 33)] = -np.inf
  off = rng.integers(-6, 3, (36, 2)).astype(np.int32)
  off[5] = (31, 0)                                          # every row source is below the volume
  off[17] = (0, -33 - 6)                                    # every column source is left of it
  ragged_taps = (rand_taps(rng, 1, 4)[0], 34, rand_taps(rng, 36, 8, zeros=0.2), rand_taps(rng, 36, 6, zeros=0.2), off)
  cases.append(_case('ragged', b, v, ragged_taps, 8.0, 1e-3))
  for eps in (0.0, 1.0):
    cases.append(_case(f'mix{eps:g}', b, v, ragged_taps, 8.0, eps))
  cases.append(_case('start', None, v, ragged_taps, 8.0, 0.25))
  # one NaN and one +inf belief cell, one NaN (and one +inf) vote cell
  b2, v2 = b.copy(), v.copy()
  b2[3, 10, 11], b2[30, 20, 5] = np.nan, np.inf
  v2[7, 15, 16], v2[8, 15, 16] = np.nan, np.inf
  cases.append(_case('bad', b2, v2, ragged_taps, 8.0, 1e-3))
  # the widest tables: rows that span workgroups
  for name, shape, Ta, Tb in (('wide', (2, 20, 300), 1, 32), ('tall', (2, 300, 20), 32, 1)):
    b, v = _belief(rng, shape), rng.standard_normal(shape).astype(np.float32)
    off = np.array([[-15 if Ta > 1 else 1, -15 if Tb > 1 else -1], [-3 if Ta > 1 else 0, -40 if Tb > 1 else 2]], np.int32)
    cases.append(_case(name, b, v, (rand_taps(rng, 1, 2)[0], 1, rand_taps(rng, 2, Ta), rand_taps(rng, 2, Tb), off),
                       1.0, 1e-3))
  # the most taps in k; Tk > R wraps more than once
  shape = (5, 6, 9)
  b, v = _belief(rng, shape), rng.standard_normal(shape).astype(np.float32)
  cases.append(_case('tk16', b, v, (rand_taps(rng, 1, 16)[0], -7, rand_taps(rng, 5, 3), rand_taps(rng, 5, 3),
                                   rng.integers(-2, 1, (5, 2)).astype(np.int32)), 1.0, 0.0))
  # more tiles than workgroups: 2 * ceil(520 * 520 / TILE) = 2114 > MAX_GROUPS
  shape = (2, 520, 520)
  assert 2 * -(-520 * 520 // TILE) > MAX_GROUPS
  b, v = _belief(rng, shape, masked=0.1), (rng.standard_normal(shape) * 0.25).astype(np.float32)
  v[:, ~border_mask(520, 520)] = -np.inf
  cases.append(_case('tiles', b, v, (rand_taps(rng, 1, 4)[0], 1, rand_taps(rng, 2, 8), rand_taps(rng, 2, 8),
                                    np.array([[-5, 2], [1, -9]], np.int32)), 8.0, 1e-3))
  # no finite belief cell: no mass, the prior is the uniform share alone
  shape = (3, 5, 6)
  cases.append(_case('empty_belief', np.full(shape, -np.inf, np.float32), rng.standard_normal(shape).astype(np.float32),
                     (rand_taps(rng, 1, 2)[0], 0, rand_taps(rng, 3, 2), rand_taps(rng, 3, 2),
                      np.zeros((3, 2), np.int32)), 1.0, 0.5))
  cases.append(exact_case())
  return cases
