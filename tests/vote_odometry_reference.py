"""float64 numpy restatement of the contract of snap_vote_odometry_f32 (include/snap_hip.h).  Written from the contract,
not from the kernel: the masses by the filter's predict rule with a scale (one f32 subtraction, the e^-40 cut, ``np.exp``
in float64 rounded to f32), the table as one vectorised product-and-sum per (k, i, j) over a zero-padded copy of the
previous frame's masses, the candidates as a gather.  ``vote_odometry`` returns the float64 logarithms BEFORE their
rounding; ``round_log`` applies the contract's single rounding.  ``cases()`` is the list both test files share."""
import functools

import numpy as np

CUT = -40.0
MAX_R, MAX_S = 64, 32


def masses(v, scale):
  """f32 volume, scale -> (mass f32, M f32 or -inf, cells with mass, NaN / +inf cells)."""
  v = np.asarray(v, dtype=np.float32)
  fin = np.isfinite(v)
  bad = int((np.isnan(v) | np.isposinf(v)).sum())
  if not fin.any():
    return np.zeros(v.shape, np.float32), np.float32(-np.inf), 0, bad
  M = np.float32(v[fin].max())
  with np.errstate(invalid='ignore', over='ignore'):
    d = (v - M).astype(np.float32)                           # one f32 subtraction
    x = np.float64(np.float32(scale)) * d.astype(np.float64)
    keep = fin & (x >= CUT)
    mass = np.where(keep, np.exp(np.where(keep, x, 0.0)).astype(np.float32), np.float32(0))
  return mass.astype(np.float32), M, int((mass > 0).sum()), bad


def table(p, q, Kr, S):
  """T [2 Kr + 1, R, 2 S + 1, 2 S + 1] float64 from the f32 masses."""
  R, Ho, Wo = p.shape
  W = 2 * S + 1
  pp = np.zeros((R, Ho + 2 * S, Wo + 2 * S), np.float64)
  pp[:, S:S + Ho, S:S + Wo] = p
  q64 = q.astype(np.float64)
  T = np.zeros((2 * Kr + 1, R, W, W), np.float64)
  for k in range(-Kr, Kr + 1):
    src = pp[(np.arange(R) + k) % R]
    for i in range(W):
      for j in range(W):
        T[k + Kr, :, i, j] = (q64 * src[:, i:i + Ho, j:j + Wo]).sum((1, 2))
  return T


def table_brute(p, q, Kr, S):
  """The same by the definition: six loops, Python floats (float64), no numpy arithmetic."""
  R, Ho, Wo = p.shape
  W = 2 * S + 1
  T = np.zeros((2 * Kr + 1, R, W, W), np.float64)
  for k in range(-Kr, Kr + 1):
    for r in range(R):
      for i in range(-S, S + 1):
        for j in range(-S, S + 1):
          s = 0.0
          for a in range(Ho):
            for b in range(Wo):
              if 0 <= a + i < Ho and 0 <= b + j < Wo:
                s += float(q[r, a, b]) * float(p[(r + k) % R, a + i, b + j])
          T[k + Kr, r, i + S, j + S] = s
  return T


def _log(x):
  with np.errstate(divide='ignore'):
    return np.log(np.asarray(x, dtype=np.float64))


def round_log(x64):
  return np.asarray(x64, dtype=np.float64).astype(np.float32)


def vote_odometry(prev, cur, Kr, S, shifts=None, scale_prev=1.0, scale_cur=1.0):
  prev, cur = np.asarray(prev, np.float32), np.asarray(cur, np.float32)
  if prev.ndim != 3 or prev.shape != cur.shape:
    raise ValueError(f'vote_odometry: shapes {prev.shape} and {cur.shape}')
  R = prev.shape[0]
  if not (1 <= R <= MAX_R and 0 <= Kr and 2 * Kr + 1 <= R and 0 <= S <= MAX_S):
    raise ValueError(f'vote_odometry: unsupported R={R} Kr={Kr} S={S}')
  p, Mp, np_mass, np_bad = masses(prev, scale_prev)
  q, Mq, nq_mass, nq_bad = masses(cur, scale_cur)
  zp, zq = float(p.astype(np.float64).sum()), float(q.astype(np.float64).sum())
  lzp, lzq = float(_log(zp)), float(_log(zq))
  T = table(p, q, Kr, S)
  with np.errstate(invalid='ignore'):
    log_table = np.where(T > 0, (_log(T) - lzp) - lzq, -np.inf)
  sh = np.zeros((0, R, 3), np.int32) if shifts is None else np.asarray(shifts, np.int32)
  U = sh.shape[0]
  k, i, j = (sh[..., n].astype(np.int64) for n in range(3))
  inside = (np.abs(k) <= Kr) & (np.abs(i) <= S) & (np.abs(j) <= S)
  E = np.zeros(U, np.float64)
  for r in range(R):                                        # r = 0 .. R-1, in that order
    ok = inside[:, r]
    E[ok] += T[k[ok, r] + Kr, r, i[ok, r] + S, j[ok, r] + S]
  with np.errstate(invalid='ignore'):
    log_evidence = np.where(E > 0, (_log(E) - lzp) - lzq, -np.inf)
  le32 = round_log(log_evidence)
  fin = np.isfinite(le32)
  best = int(np.argmax(np.where(fin, le32, -np.inf))) if fin.any() else -1
  lse = -np.inf
  if fin.any():
    m = float(le32[fin].max())
    lse = m + float(np.log(np.exp(le32[fin].astype(np.float64) - m).sum()))
  ninf = -np.inf
  stats = np.array([lzp + float(np.float32(scale_prev)) * float(Mp) if zp > 0 else ninf,
                    lzq + float(np.float32(scale_cur)) * float(Mq) if zq > 0 else ninf, lse,
                    float(le32[best]) if best >= 0 else ninf], np.float64)
  count = np.array([np_mass, np_bad, nq_mass, nq_bad, int((~inside).sum()), int(fin.sum())], np.int32)
  return dict(T=T, log_table=log_table, E=E, log_evidence=log_evidence, best=best, stats=stats, count=count, zp=zp,
              zq=zq, p=p, q=q)


def tolerance(want32):
  """The bound of the GPU test on a finite log value against the rounded reference: 2 f32 ulps + 2^-22 (two correct
  exp implementations may round one f32 mass an ulp apart, 2^-23 relative per factor, so 2^-22 on T, absolute on
  log T).  The order of the float64 sums adds < n 2^-53 relative with n < 2^31 cells: below 2^-22 at every shape."""
  x = np.where(np.isfinite(want32), np.abs(want32), 0).astype(np.float32)
  return 2 * np.spacing(x).astype(np.float64) + 2.0 ** -22


def runner_up_margin(out):
  """The reference's best log-evidence minus its runner-up's (inf with fewer than two finite candidates)."""
  le = round_log(out['log_evidence']).astype(np.float64)
  if out['best'] < 0:
    return np.inf
  rest = np.delete(le, out['best'])
  rest = rest[np.isfinite(rest)]
  return np.inf if rest.size == 0 else float(le[out['best']] - rest.max())


def transported(prev, k, i, j):
  """cur[r, a, b] = prev[(r + k) mod R, a + i, b + j], -inf where the source lies outside the plane."""
  R, Ho, Wo = prev.shape
  cur = np.full(prev.shape, -np.inf, np.float32)
  a0, a1 = max(0, -i), min(Ho, Ho - i)
  b0, b1 = max(0, -j), min(Wo, Wo - j)
  src = prev[(np.arange(R) + k) % R]
  if a0 < a1 and b0 < b1:
    cur[:, a0:a1, b0:b1] = src[:, a0 + i:a1 + i, b0 + j:b1 + j]
  return cur


def _two_peaks(rng, shape, sharp=1.5):
  R, Ho, Wo = shape
  v = rng.normal(0.0, 1.0, shape)
  a, b = np.mgrid[0:Ho, 0:Wo]
  for n in range(2):
    r0, a0, b0 = rng.integers(0, R), rng.integers(Ho // 4, Ho - Ho // 4 + 1), rng.integers(Wo // 4, Wo - Wo // 4 + 1)
    bump = (12.0 - 3.0 * n) * np.exp(-((a - a0) ** 2 + (b - b0) ** 2) / (2 * sharp ** 2))
    v[r0 % R] += bump
  return v.astype(np.float32)


def _shift_rows(rng, R, Kr, S, U, planted=None, outside=0):
  """U candidate rows: constant over r for the planted one, jittered by a cell for the others, ``outside`` rows beyond
  the window."""
  sh = np.zeros((U, R, 3), np.int32)
  for u in range(U):
    base = np.array([rng.integers(-Kr, Kr + 1), rng.integers(-S, S + 1), rng.integers(-S, S + 1)])
    sh[u] = base
    sh[u, :, 1:] += rng.integers(-1, 2, (R, 2))
  np.clip(sh[..., 1:], -S, S, out=sh[..., 1:])
  if planted is not None:
    sh[U // 2] = np.asarray(planted, np.int32)
  for n in range(outside):
    u, r, c = rng.integers(0, U), rng.integers(0, R), n % 3
    if planted is not None and u == U // 2:
      u = (u + 1) % U
    sh[u, r, c] = (Kr + 1, S + 1, -S - 1)[c] if n % 2 == 0 else (-Kr - 1, -S - 2, S + 3)[c]
  return sh


@functools.lru_cache(maxsize=None)
def cases():
  out = []

  def add(name, prev, cur, Kr, S, shifts, scale_prev=1.0, scale_cur=1.0, planted=None):
    out.append(dict(name=name, prev=np.ascontiguousarray(prev, np.float32), cur=np.ascontiguousarray(cur, np.float32),
                    Kr=Kr, S=S, shifts=shifts, scale_prev=scale_prev, scale_cur=scale_cur, planted=planted))

  rng = np.random.default_rng(20261020)
  # [1, 1, 1]: one cell each, one candidate
  add('minimal', np.full((1, 1, 1), 0.25), np.full((1, 1, 1), -3.0), 0, 0, np.zeros((1, 1, 3), np.int32), planted=0)
  # the full circle of a 3-rotation volume, a planted shift
  prev = _two_peaks(rng, (3, 5, 6), 0.8)
  add('full_circle', prev, transported(prev, 1, -1, 2), 1, 2, _shift_rows(rng, 3, 1, 2, 9, (1, -1, 2)))
  # a window larger than the plane: most shifts have no overlap at all
  add('window_larger_than_plane', prev, transported(prev, -1, 2, -3) + rng.normal(0, 0.1, prev.shape).astype(np.float32),
      1, 7, _shift_rows(rng, 3, 1, 7, 11, (-1, 2, -3), outside=3), planted=5)
  add('no_candidates', prev, _two_peaks(rng, (3, 5, 6), 0.8), 1, 2, None)
  add('all_masked', np.full((3, 5, 6), -np.inf), np.full((3, 5, 6), -np.inf), 1, 2, _shift_rows(rng, 3, 1, 2, 5))
  # ragged tiles and bands; a -inf half-plane, NaN and +inf cells in each input, cells below the cut, scales != 1
  prev = _two_peaks(rng, (5, 37, 70))
  cur = transported(prev, 2, 3, -2) + rng.normal(0, 0.2, prev.shape).astype(np.float32)
  prev, cur = prev.copy(), cur.copy()
  prev[:, :, :20] = -np.inf
  prev[1, 30, 40:50] = -150.0                                # 0.7 * (-150 - max) < -40: below the cut
  cur[2, 5:9, 60:] = -90.0
  prev[0, 20, 30], prev[3, 1, 69], prev[4, 36, 25] = np.nan, np.inf, np.nan
  cur[1, 0, 0], cur[4, 36, 69] = np.inf, np.nan
  add('ragged', prev, cur, 2, 3, _shift_rows(rng, 5, 2, 3, 16, (2, 3, -2), outside=4), 0.7, 1.3, planted=8)
  # the largest window
  prev = _two_peaks(rng, (4, 19, 300), 2.0)
  add('largest_window', prev, transported(prev, -1, -9, 31), 1, 32, _shift_rows(rng, 4, 1, 32, 24, (-1, -9, 31), outside=2),
      planted=12)
  # medium: several bands, two column tiles, NACC = 2
  prev = _two_peaks(rng, (8, 96, 80), 2.5)
  cur = transported(prev, -2, 7, -8) + rng.normal(0, 0.3, prev.shape).astype(np.float32)
  cur[:, 48:, :] = np.where(rng.random((8, 48, 80)) < 0.5, -np.inf, cur[:, 48:, :])
  add('medium', prev, cur, 2, 8, _shift_rows(rng, 8, 2, 8, 40, (-2, 7, -8), outside=5), 1.0, 0.5, planted=20)
  # one case per accumulator count of the hot kernel that the shapes above do not reach (3, 5, 7, 10, 13, 17 per thread:
  # W = 2 S + 1 = 25, 33, 41, 49, 51, 57), on a plane of two ragged column tiles
  prev = _two_peaks(rng, (2, 23, 70), 2.0)
  for S in (12, 16, 20, 24, 25, 28):
    shift = (0, S // 2, -S)
    add(f'window_{S}', prev, transported(prev, *shift), 0, S, _shift_rows(rng, 2, 0, S, 6, shift) if S % 8 else None,
        planted=3 if S % 8 else None)
  return tuple(out)


@functools.lru_cache(maxsize=None)
def shared():
  """name -> (case, reference result), computed once for all tests."""
  return {c['name']: (c, vote_odometry(c['prev'], c['cur'], c['Kr'], c['S'], c['shifts'], c['scale_prev'],
                                       c['scale_cur'])) for c in cases()}
