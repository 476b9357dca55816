"""float64 numpy restatement of the contract of snap_vote_temper_f32 (include/snap_hip.h), its documented error bound,
the exact minimiser of the ground-truth NLL over a set of volumes, and the inputs the tests share.

Written from the header's comment; imports nothing of the package and no torch.

  votes [R, Ho, Wo] f32, flat(r, a, b) = (r * Ho + a) * Wo + b; F = the finite cells (-inf masked, NaN / +inf excluded
  and counted); m = max_F v, d = v - m <= 0.  For every scale s of the ladder (the float64 value of its f32 rounding),
  with e = exp(s d): A = log sum_F e, mu = sum e d / sum e, q = sum e d^2 / sum e.
  table[l] = (log_z = s m + A, E[v] = m + mu, Var[v] = q - mu^2, entropy = A - s mu, log p_max = -A,
              log_prob_gt = s v_gt - log_z, dnll = E[v] - v_gt, 0); stats = (m, v_gt, 0, 0);
  count = (|F|, NaN or +inf cells, ground-truth sample valid, 0).
  v_gt: the trilinear interpolation of v at (k, i, j), circular in k, taps of weight 0 not read; valid iff k, i, j
  finite, 0 <= i <= Ho-1, 0 <= j <= Wo-1 and every tap of non-zero weight is in F; else v_gt, log_prob_gt, dnll NaN.
  F empty: m = log_z = -inf, columns 1 .. 6 NaN.

THE ERROR BOUND (``bound``), from the kernel's rounding points.  u = 2^-24.
  The kernel sums the moments in x = s d, not in d (a term with e > 0 has |x| < 104: nothing overflows), and divides by
  s and s^2 in float64.  d = fl32(v - m): |d| u (one f32 subtraction).  x = fl32(s d): one f32 product on top of the
  rounded d: x is relatively off by 2 u, so the argument of the exponential by 2 |x| u, and so is the weight,
  relatively.  e = expf(x) is within 1 ulp = 2 u (the documented accuracy of the device library's expf).  fl32(e x)
  adds one product rounding and the error of x (3 u), fl32(fl32(e x) x) the same again (3 u).  A pixel's three sums are
  f32 sums of <= R terms of one sign each: (R - 1) u relative.  So every term of S0, S1 and S2 of a cell c is
  relatively off by at most
      eps_c = (2 |x_c| + R + 7) u
  (1.01 covers the second order).  Everything above the pixel is float64 (SLOP = 2^-40 relative to the magnitudes
  involved covers those paths, the device's log and the sum s m + A).  With p_c = e_c / S0:
      A:         eZ = 1.01 sum p eps + UF0                                   (log: relative error of S0)
      mu:        eM = 1.01 sum p eps (|d| + |mu|) + UF1 + UF0 |mu|           (a ratio: numerator and denominator)
      q:         eQ = 1.01 sum p eps (d^2 + q) + UF2 + UF0 q
      Var:       eQ + 2 |mu| eM + eM^2      (ABSOLUTE, on the scale of q: the subtraction q - mu^2 cancels)
      log_z:     eZ; E[v]: eM; entropy = A - s mu: eZ + s eM; log p_max: eZ;
      log_prob_gt = s v_gt - log_z: eZ plus the float64 rounding of the two large terms; dnll = E[v] - v_gt: eM.
  Underflow: a weight below 2^-126 is kept with an absolute error of 2^-149 or lost: with n = |F| that is at most
  UF0 = n 2^-126 of S0 (S0 >= 1: the maximum's weight is 1), n 2^-119 of S1 (|x| e^-|x| < 2^-119 beyond |x| = 87) and
  n 2^-112 of S2, and a denormal product adds at most n 2^-149 and n 2^-142: UF1 = n 2^-118 / s, UF2 = n 2^-111 / s^2.
  The outputs are float64: there is no final f32 rounding term.
The bound is a function of the input alone; the GPU test allows twice it.
"""
import numpy as np

U = 2.0 ** -24
SLOP = 2.0 ** -40
TILE = 256          # pixels of one workgroup tile (flat order)
COLUMNS = ('log_z', 'mean_vote', 'var_vote', 'entropy', 'log_p_max', 'log_prob_gt', 'dnll', 'zero7')


def supported(shape, S):
  if len(shape) != 3 or min(shape) < 1:
    return False
  R, Ho, Wo = shape
  return R <= 64 and R * Ho * Wo < 2 ** 31 and 1 <= S <= 16


def ladder(scales):
  """The scales as the kernel uses them: float64 values of the f32 roundings; finite, > 0, strictly increasing."""
  with np.errstate(over='ignore'):
    s = np.asarray(scales, dtype=np.float64).reshape(-1).astype(np.float32)
  if not (s.size >= 1 and np.all(np.isfinite(s)) and np.all(s > 0) and np.all(np.diff(s) > 0)):
    raise ValueError(f'vote_temper: scales {scales}')
  return s.astype(np.float64)


def _prepare(votes, scales):
  v = np.asarray(votes)
  assert v.dtype == np.float32 and v.ndim == 3
  s = ladder(scales)
  if not supported(v.shape, s.size):
    raise ValueError(f'vote_temper: unsupported shape {v.shape} S={s.size}')
  F = np.isfinite(v)
  return v, s, F


def gt_sample(v, F, gt_index):
  """(interpolated v, valid, taps) at a continuous index; taps = [(weight, r, a, b)] of non-zero weight."""
  R, Ho, Wo = v.shape
  if gt_index is None:
    return np.nan, 0, []
  k, i, j = (np.float64(np.float32(c)) for c in gt_index)
  if not (np.isfinite(k) and np.isfinite(i) and np.isfinite(j) and 0 <= i <= Ho - 1 and 0 <= j <= Wo - 1):
    return np.nan, 0, []
  kf, i0, j0 = np.floor(k), int(np.floor(i)), int(np.floor(j))
  k0 = int(kf % R)
  taps, total, ok = [], 0.0, True
  for dk, wk in ((0, 1 - (k - kf)), (1, k - kf)):
    for di, wi in ((0, 1 - (i - i0)), (1, i - i0)):
      for dj, wj in ((0, 1 - (j - j0)), (1, j - j0)):
        w = wk * wi * wj
        if w == 0:
          continue
        c = ((k0 + dk) % R, i0 + di, j0 + dj)
        taps.append((w,) + c)
        if F[c]:
          total += w * np.float64(v[c])
        else:
          ok = False
  return (total, 1, taps) if ok else (np.nan, 0, taps)


def moments(d, s):
  """(A, mu, q) of the float64 offsets d <= 0 of the contributing cells (their maximum is 0) at the float64 scale s."""
  with np.errstate(under='ignore'):
    e = np.exp(s * d)
  S0 = e.sum()
  return np.log(S0), (e * d).sum() / S0, (e * d * d).sum() / S0


def vote_temper(votes, scales, gt_index=None):
  """-> (table f64 [S, 8], stats f64 [4], count int32 [4])."""
  v, s, F = _prepare(votes, scales)
  table = np.full((s.size, 8), np.nan)
  table[:, 7] = 0
  stats = np.array([-np.inf, np.nan, 0.0, 0.0])
  count = np.array([int(F.sum()), int((np.isnan(v) | (v == np.inf)).sum()), 0, 0], np.int32)
  if not F.any():
    table[:, 0] = -np.inf
    return table, stats, count
  m = np.float64(v[F].max())
  d = v[F].astype(np.float64) - m
  v_gt, valid, _ = gt_sample(v, F, gt_index)
  stats[0], stats[1], count[2] = m, v_gt, valid
  for l, sl in enumerate(s):
    A, mu, q = moments(d, sl)
    log_z = sl * m + A
    table[l, :7] = (log_z, m + mu, max(q - mu * mu, 0.0), A - sl * mu, -A, sl * v_gt - log_z, (m + mu) - v_gt)
  return table, stats, count


def bound(votes, scales, gt_index=None):
  """-> tol f64 [S, 8]: the documented absolute error bound of every table entry (module docstring); 0 where the output
  is exact by contract (column 7, and everything of an empty volume).  stats and count are exact."""
  v, s, F = _prepare(votes, scales)
  R = v.shape[0]
  tol = np.zeros((s.size, 8))
  if not F.any():
    return tol
  n = int(F.sum())
  m = np.float64(v[F].max())
  d = v[F].astype(np.float64) - m
  ad = np.abs(d)
  v_gt, valid, taps = gt_sample(v, F, gt_index)
  tap_mag = max((abs(float(v[c[1:]])) for c in taps), default=0.0) if valid else 0.0
  for l, sl in enumerate(s):
    A, mu, q = moments(d, sl)
    with np.errstate(under='ignore'):
      p = np.exp(sl * d - A)
    eps = (2 * sl * ad + R + 7) * U
    with np.errstate(invalid='ignore'):                      # (0 * inf: a cell of weight 0 and an unbounded argument)
      pe = np.where(p > 0, p * eps, 0.0)
    uf0 = n * 2.0 ** -126
    uf1 = n * 2.0 ** -118 / sl
    uf2 = n * 2.0 ** -111 / sl ** 2
    eZ = 1.01 * pe.sum() + uf0
    eM = 1.01 * (pe * (ad + abs(mu))).sum() + uf1 + uf0 * abs(mu)
    eQ = 1.01 * (pe * (d * d + q)).sum() + uf2 + uf0 * q
    big = abs(sl * m) + abs(A)
    tol[l, 0] = eZ + SLOP * big
    tol[l, 1] = eM + SLOP * (abs(m) + abs(mu))
    tol[l, 2] = eQ + 2 * abs(mu) * eM + eM ** 2 + SLOP * (q + mu * mu)
    tol[l, 3] = eZ + sl * eM + SLOP * (abs(A) + sl * abs(mu))
    tol[l, 4] = eZ + SLOP * abs(A)
    if valid:
      tol[l, 5] = tol[l, 0] + SLOP * sl * tap_mag
      tol[l, 6] = tol[l, 1] + SLOP * tap_mag
  return tol


def nll_minimiser(volumes, gts, lo, hi, iters=200):
  """The exact minimiser in [lo, hi] of sum_f (log_z_f(s) - s v_gt_f) over the frames with a valid ground truth, by
  bisection on its derivative sum_f (E_s[v] - v_gt_f) in float64 (the NLL is convex in s) -> (s, valid frames);
  ``lo`` / ``hi`` where the derivative does not change sign inside."""
  frames = []
  for v, gt in zip(volumes, gts):
    v = np.asarray(v)
    F = np.isfinite(v)
    v_gt, valid, _ = gt_sample(v, F, gt)
    if valid:
      m = np.float64(v[F].max())
      frames.append((v[F].astype(np.float64) - m, v_gt - m))
  slope = lambda s: sum(moments(d, s)[1] - g for d, g in frames)
  if not frames or slope(lo) >= 0:
    return float(lo), len(frames)
  if slope(hi) <= 0:
    return float(hi), len(frames)
  a, b = float(lo), float(hi)
  for _ in range(iters):
    c = 0.5 * (a + b)
    if slope(c) < 0:
      a = c
    else:
      b = c
  return 0.5 * (a + b), len(frames)


# ---- the inputs the CPU and GPU tests share -------------------------------------------------------------------------
RANDOM_SHAPES = [(4, 7, 7), (1, 5, 5), (3, 1, 1), (36, 31, 33), (64, 5, 300)]
FOLD_SHAPE = (2, 520, 520)     # 1057 tiles of 256 pixels > 1024 workgroups: workgroups 0 .. 32 own two tiles each
LADDERS = {1: (1.5,), 5: (0.25, 1.0, 3.0, 10.0, 30.0), 16: tuple(2.0 ** (-2 + 4 * i / 15) for i in range(16))}


def random_votes(shape, seed=0):
  """Uniform votes in [-1, 1], 30 % of the cells -inf."""
  rng = np.random.default_rng(seed + 7 * sum(shape))
  v = rng.uniform(-1, 1, shape).astype(np.float32)
  v[rng.random(shape) < 0.3] = -np.inf
  if not np.isfinite(v).any():
    v.reshape(-1)[0] = 0.25
  return v


def exact_votes(shape, seed=0):
  """Votes in {0, -inf}: every exponential is exactly 1 or 0 at every scale."""
  rng = np.random.default_rng(seed + 11 * sum(shape))
  v = np.where(rng.random(shape) < 0.4, np.float32(0), np.float32(-np.inf)).astype(np.float32)
  v.reshape(-1)[-1] = 0
  return v


def single_cell_votes(shape=(36, 31, 33), value=-3.25):
  v = np.full(shape, -np.inf, np.float32)
  c = tuple(x // 2 for x in shape)
  v[c] = value
  return v, c


def tied_votes(shape=(4, 7, 7)):
  """Two cells at 0.5, every other cell at or below 0.25: at scale 1e4 only the tie has weight."""
  v = random_votes(shape, seed=3)
  v = np.where(np.isfinite(v), np.minimum(v, np.float32(0.25)), v).astype(np.float32)
  v[0, 1, 2] = v[3, 6, 6] = 0.5
  return v


def nan_inf_votes(shape=(36, 31, 33)):
  """(votes with a few NaN / +inf cells planted, the same votes with those cells masked instead, cells planted)."""
  v = random_votes(shape, seed=5)
  cells = [(0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1), (3, 8, 32), (3, 8, 31), (17, 30, 0)]
  bad, masked = v.copy(), v.copy()
  for n, c in enumerate(cells):
    bad[c] = np.inf if n % 2 else np.nan
    masked[c] = -np.inf
  return bad, masked, len(cells)


def huge_votes(shape=(4, 7, 7)):
  """Votes around 1e30 (spaced by whole f32 steps of 7.6e22 there), two of them tied at the top, 30 % masked: with a
  scale of 1e10 the product scale * v is 1e40, beyond f32."""
  rng = np.random.default_rng(41)
  v = (np.float32(1e30) * (1 + rng.uniform(-0.5, 0, shape))).astype(np.float32)
  v[rng.random(shape) < 0.3] = -np.inf
  v[1, 2, 3] = v[2, 5, 1] = np.float32(1.25e30)
  return v


HUGE_SCALES = (1e-30, 1e-29, 1.0, 1e10)
HUGE_GT = (1.0, 2.0, 3.0)


def gt_cases(shape=(36, 31, 33)):
  """(votes, [(name, (k, i, j), valid)]) for the ground-truth sample."""
  R, Ho, Wo = shape
  rng = np.random.default_rng(99)
  v = rng.uniform(-1, 1, shape).astype(np.float32)
  v[5, 10, 12] = -np.inf                                    # a masked tap
  cases = [('interior', (7.25, 3.5, 20.75), 1), ('integer', (2.0, 4.0, 9.0), 1), ('wrap', (R - 0.25, 6.5, 6.5), 1),
           ('past_R', (R + 2.5, 6.5, 6.5), 1), ('last_row', (1.5, float(Ho - 1), 3.25), 1),
           ('last_col_corner', (0.0, float(Ho - 1), float(Wo - 1)), 1), ('past_last_row', (1.5, Ho - 0.5, 3.25), 0),
           ('masked_tap', (4.5, 9.5, 11.5), 0), ('masked_tap_weight_zero', (6.0, 10.0, 12.0), 1),
           ('nan', (np.nan, 3.0, 3.0), 0), ('negative', (1.0, -0.25, 3.0), 0), ('negative_k', (-0.5, 2.0, 2.5), 1)]
  return v, cases


def fold_votes(shape=FOLD_SHAPE):
  """Uniform votes in [-1, 1], 30 % masked, on a plane of more than 1024 tiles: workgroup g < 33 walks tile g and then
  tile g + 1024.  Tiles 0 .. 9 are fully masked, tiles 1040 .. 1049 too; tiles 10 .. 15 are raised by 3 and tiles
  1024 .. 1039 by 2, so the second tile of a workgroup carries most of the weight of some and little of others."""
  R, Ho, Wo = shape
  P = Ho * Wo
  v = random_votes(shape, seed=21).reshape(R, P)
  tile = np.arange(P) // TILE
  v[:, (tile < 10) | ((tile >= 1040) & (tile < 1050))] = -np.inf
  fin = np.isfinite(v)
  v[:, (tile >= 10) & (tile < 16)] += np.float32(3)
  v[:, (tile >= 1024) & (tile < 1040)] += np.float32(2)
  v[~fin] = -np.inf
  return np.ascontiguousarray(v.reshape(shape))


def all_inputs():
  """[(name, votes, scales, gt_index)]: every input of the GPU tests that is compared within the bound."""
  out = []
  for shape in RANDOM_SHAPES:
    v = random_votes(shape)
    cells = np.argwhere(np.isfinite(v))
    gt = tuple(float(i) for i in cells[len(cells) // 2])      # a contributing cell: the sample is valid
    for S, scales in LADDERS.items():
      out.append(('random%s_S%d' % (shape, S), v, scales, gt))
  out.append(('fold', fold_votes(), LADDERS[16], (0.5, 517.25, 103.5)))
  out.append(('exact', exact_votes((36, 31, 33)), LADDERS[5], None))
  out.append(('single', single_cell_votes()[0], LADDERS[5], None))
  out.append(('tied', tied_votes(), (1.0, 1e4), None))
  out.append(('nan_inf', nan_inf_votes()[0], LADDERS[5], None))
  out.append(('huge', huge_votes(), HUGE_SCALES, HUGE_GT))
  v, cases = gt_cases()
  for name, idx, _ in cases:
    out.append(('gt_' + name, v, LADDERS[5], idx))
  return out


# ---- the fit tests' validation set ----------------------------------------------------------------------------------
FIT_SHAPE = (4, 9, 9)
FIT_FRAMES = 32
FIT_TRUE_SCALE = 2.0
FIT_LADDER = (0.25, 16.0, 16)      # lo, hi, num of the first round


def fit_frames(seed=2024):
  """(volumes, gt indices): FIT_FRAMES volumes of FIT_SHAPE with normal votes of standard deviation 1.5 (10 % masked)
  and, per volume, the index of ONE cell drawn from softmax(FIT_TRUE_SCALE * v) as (k, i, j) floats.  Frames 5 and 17
  get an invalid ground truth instead (outside the volume; on a masked cell): they must change nothing."""
  rng = np.random.default_rng(seed)
  volumes, gts = [], []
  for f in range(FIT_FRAMES):
    v = (1.5 * rng.standard_normal(FIT_SHAPE)).astype(np.float32)
    v[rng.random(FIT_SHAPE) < 0.1] = -np.inf
    F = np.isfinite(v)
    x = np.where(F, FIT_TRUE_SCALE * np.where(F, v, 0).astype(np.float64), -np.inf)
    p = np.exp(x - x.max())
    p /= p.sum()
    c = np.unravel_index(rng.choice(p.size, p=p.reshape(-1)), FIT_SHAPE)
    gt = tuple(float(i) for i in c)
    if f == 5:
      gt = (1.0, float(FIT_SHAPE[1]), 2.0)
    if f == 17:
      gt = tuple(float(i) for i in np.argwhere(~F)[0])
    volumes.append(v)
    gts.append(gt)
  return volumes, gts
