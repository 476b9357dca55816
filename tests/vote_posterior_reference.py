"""float64 numpy restatement of the contract of snap_vote_posterior_f32 (include/snap_hip.h), its documented error
bound, a float32 restatement of the kernel's two-level summation, and the inputs the tests share.

Written from the header's comment; imports nothing of the package.

  votes [R, Ho, Wo] f32, flat(r, a, b) = (r * Ho + a) * Wo + b; x = scale * v over the FINITE cells F (-inf masked,
  NaN / +inf excluded and counted).  log_z = log sum_F exp(x); log_prob_xy = log sum_r exp(x) - log_z;
  log_prob_r = log sum_ab exp(x) - log_z; p = exp(x - log_z).
  stats[16] = (log_z, max x, E[a], E[b], Var a, Cov ab, Var b, C, S, mean rotation index in [0, R), resultant length,
  entropy = log_z - E[x], log_prob_gt, 0, 0, 0); count = (|F|, NaN or +inf cells, ground-truth sample valid).
  log_prob_gt: trilinear interpolation of x at (k, i, j) minus log_z, circular in k, taps of weight 0 not read;
  valid iff k, i, j finite, 0 <= i <= Ho-1, 0 <= j <= Wo-1 and every tap of non-zero weight is in F; else NaN.
  F empty: log_z = max x = -inf, marginals -inf, stats[2..12] NaN.

THE ERROR BOUND (``bound``), from the kernel's rounding points.  u = 2^-24.
  A cell's weight is e = expf(d), d = fma(scale, v, -m_p) (m_p: the pixel's maximum of fl(scale v)): the argument is
  rounded once, |d| u, and expf is within 1 ulp = 2 u (the documented accuracy of the device library's expf and
  logf); a pixel's s_p = sum_r e is an f32 sum of <= R terms of one sign: (R - 1) u.  The pixel enters every sum
  above it through f_p = expf(fl(m_p - m_t)) (m_t the tile maximum, m_p - m_t <= M - m_p =: g_p): (g_p + 2) u; the
  per-rotation sums add one f32 product and a 6-level f32 tree over the wave: 7 u.  Everything above is float64.
  So the relative error of a pixel's (or of any of its cells') weight is at most
      eps_p = (D_p + g_p + R + 12) u,      D_p = m_p - min_r x  (the largest |d| of the pixel),
  and a sum of weights is off by at most its probability-weighted mean of eps_p: eps_Z = sum_p q_p eps_p for log_z,
  eps_r = sum_p q_rp eps_p / q_r for a rotation.  A normalised expectation E[g] moves by at most
  sum q eps |g - E g| (to first order; 1.01 covers the rest), which gives the moment, C / S and entropy terms below.
  Underflow: a weight below 2^-126 relative to its tile maximum may be lost; that is at most UF = R P 2^-126 of
  probability, which matters only for log_prob_r of a rotation of probability ~ UF (tolerance UF / q_r).
  log_prob_xy is computed per pixel as (m_p - M) + log s_p - log Z' in float64 and rounded once:
  (D_p + R + 4) u + eps_Z + u |result|.  Every f32 store adds u |value|; SLOP = 2^-40 covers the float64 paths.
The bound is a function of the input alone; the GPU test allows twice it.
"""
import numpy as np

U = 2.0 ** -24
SLOP = 2.0 ** -40
TILE = 256          # pixels of one workgroup tile (flat order); 64 per wave
STAT_NAMES = ('log_z', 'max_x', 'E_a', 'E_b', 'Var_a', 'Cov_ab', 'Var_b', 'C', 'S', 'mean_r', 'resultant', 'entropy',
              'log_prob_gt', 'zero13', 'zero14', 'zero15')


def supported(shape):
  if len(shape) != 3 or min(shape) < 1:
    return False
  R, Ho, Wo = shape
  return R <= 64 and R * Ho * Wo < 2 ** 31


def _lse(x, axis=None):
  """log sum exp over ``axis`` of float64 ``x`` (-inf = absent); -inf where nothing is present."""
  m = np.max(x, axis=axis, keepdims=True)
  ms = np.where(np.isfinite(m), m, 0.0)
  with np.errstate(divide='ignore'):
    out = np.log(np.sum(np.exp(x - ms), axis=axis, keepdims=True)) + ms
  return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def _prepare(votes, scale):
  v = np.asarray(votes)
  assert v.dtype == np.float32 and v.ndim == 3
  if not supported(v.shape):
    raise ValueError(f'vote_posterior: unsupported shape {v.shape}')
  scale = np.float32(scale)
  if not (np.isfinite(scale) and scale > 0):
    raise ValueError(f'vote_posterior: scale {scale}')
  F = np.isfinite(v)
  x = np.where(F, np.float64(scale) * np.where(F, v, 0).astype(np.float64), -np.inf)
  return v, scale, F, x


def _gt_sample(v, F, x, gt_index):
  """(interpolated x, valid, taps) at a continuous index; taps = [(weight, r, a, b)] of non-zero weight."""
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
          total += w * x[c]
        else:
          ok = False
  return (total, 1, taps) if ok else (np.nan, 0, taps)


def vote_posterior(votes, scale=1.0, gt_index=None):
  """-> (log_prob_xy f64 [Ho, Wo], log_prob_r f64 [R], stats f64 [16], count int32 [3])."""
  v, scale, F, x = _prepare(votes, scale)
  R, Ho, Wo = v.shape
  stats = np.full(16, np.nan)
  stats[13:] = 0
  count = np.array([int(F.sum()), int((np.isnan(v) | (v == np.inf)).sum()), 0], np.int32)
  if not F.any():
    stats[0] = stats[1] = -np.inf
    return np.full((Ho, Wo), -np.inf), np.full(R, -np.inf), stats, count
  log_z = float(_lse(x))
  lxy = _lse(x, axis=0) - log_z
  lr = _lse(x.reshape(R, -1), axis=1) - log_z
  p = np.exp(x - log_z)
  p /= p.sum()
  pxy, pr = p.sum(0), p.sum((1, 2))
  a, b = np.arange(Ho, dtype=np.float64)[:, None], np.arange(Wo, dtype=np.float64)[None, :]
  ea, eb = float((pxy * a).sum()), float((pxy * b).sum())
  ang = 2 * np.pi * np.arange(R) / R
  C, S = float((pr * np.cos(ang)).sum()), float((pr * np.sin(ang)).sum())
  stats[0], stats[1] = log_z, x.max()
  stats[2], stats[3] = ea, eb
  stats[4] = (pxy * (a - ea) ** 2).sum()
  stats[5] = (pxy * (a - ea) * (b - eb)).sum()
  stats[6] = (pxy * (b - eb) ** 2).sum()
  stats[7], stats[8] = C, S
  stats[9] = (np.arctan2(S, C) * R / (2 * np.pi)) % R
  stats[10] = np.hypot(C, S)
  stats[11] = log_z - float((p[F] * x[F]).sum())
  g, valid, _ = _gt_sample(v, F, x, gt_index)
  stats[12] = g - log_z if valid else np.nan
  count[2] = valid
  return lxy, lr, stats, count


def bound(votes, scale=1.0, gt_index=None):
  """-> (tol_xy [Ho, Wo], tol_r [R], tol_stats [16]): the documented absolute error bound of every output (module
  docstring).  mean_r (stats[9]) is to be compared circularly (mod R).  0 where the output is exact by contract."""
  v, scale, F, x = _prepare(votes, scale)
  R, Ho, Wo = v.shape
  P = Ho * Wo
  tol_xy, tol_r, ts = np.zeros((Ho, Wo)), np.zeros(R), np.zeros(16)
  if not F.any():
    return tol_xy, tol_r, ts
  lxy, lr, st, _ = vote_posterior(v, scale, gt_index)
  log_z, M = st[0], st[1]
  live = F.any(0)
  m_p = np.where(live, x.max(0), 0.0)
  D_p = np.where(live, m_p - np.where(F, x, np.inf).min(0), 0.0)
  g_p = np.where(live, M - m_p, 0.0)
  eps_p = np.where(live, (D_p + g_p + R + 12) * U, 0.0)
  q = np.where(F, np.exp(x - log_z), 0.0)
  q_p, q_r = q.sum(0), q.sum((1, 2))
  eps_z = float((q_p * eps_p).sum())
  UF = R * P * 2.0 ** -126
  a, b = np.arange(Ho, dtype=np.float64)[:, None], np.arange(Wo, dtype=np.float64)[None, :]
  tol_xy = np.where(live, (D_p + R + 4) * U + eps_z + U * np.abs(np.where(live, lxy, 0)) + SLOP + R * 2.0 ** -126, 0.0)
  with np.errstate(divide='ignore', invalid='ignore'):
    eps_r = np.where(q_r > 0, (q * eps_p[None]).sum((1, 2)) / q_r, 0.0)
    tol_r = np.where(F.any((1, 2)), eps_r + eps_z + UF / q_r + U * np.abs(np.where(q_r > 0, lr, 0)) + SLOP, 0.0)
  ts[0] = eps_z + U * abs(log_z) + SLOP + UF
  ts[1] = U * abs(M)
  da, db = np.abs(a - st[2]), np.abs(b - st[3])
  w = q_p * eps_p
  ts[2] = 1.01 * (w * da).sum() + U * abs(st[2]) + (SLOP + UF) * Ho
  ts[3] = 1.01 * (w * db).sum() + U * abs(st[3]) + (SLOP + UF) * Wo
  ts[4] = 1.01 * (w * (da ** 2 + st[4])).sum() + ts[2] ** 2 + U * st[4] + (2.0 ** -48 + UF) * (q_p * a * a).sum() + SLOP
  ts[5] = (1.01 * (w * (da * db + abs(st[5]))).sum() + ts[2] * ts[3] + U * abs(st[5])
           + (2.0 ** -48 + UF) * (q_p * a * b).sum() + SLOP)
  ts[6] = 1.01 * (w * (db ** 2 + st[6])).sum() + ts[3] ** 2 + U * st[6] + (2.0 ** -48 + UF) * (q_p * b * b).sum() + SLOP
  ang = 2 * np.pi * np.arange(R) / R
  wr = q_r * eps_r
  ts[7] = 1.01 * (wr * np.abs(np.cos(ang) - st[7])).sum() + U * abs(st[7]) + SLOP + UF
  ts[8] = 1.01 * (wr * np.abs(np.sin(ang) - st[8])).sum() + U * abs(st[8]) + SLOP + UF
  h = float(np.hypot(ts[7], ts[8]))
  ts[9] = R if h >= 0.5 * st[10] else R / (2 * np.pi) * 1.1 * h / st[10] + U * R + SLOP
  ts[10] = h + U * st[10]
  y, d = np.where(F, x - M, 0.0), np.where(F, x - m_p[None], 0.0)
  ey = float((q * y).sum())
  ts[11] = (eps_z + 1.01 * (q * eps_p[None] * (np.abs(y - ey) + np.abs(d))).sum() + U * abs(st[11]) + SLOP
            + UF * (1 + float(np.abs(y).max())))
  _, valid, taps = _gt_sample(v, F, x, gt_index)
  if valid:
    ts[12] = max(abs(x[c[1:]]) for c in taps) * U + ts[0] + U * abs(st[12]) + SLOP
  return tol_xy, tol_r, ts


def two_level_f32(votes, scale=1.0, gt_index=None):
  """The kernel's arithmetic restated in numpy: f32 weights relative to the pixel's own maximum, f32 sums over the
  <= R terms of a pixel and over the 64 pixels of a wave, float64 above, one rounding to f32 at the end.  Not
  bit-equal to the device (numpy's exp and its 64-term sum round differently); the same rounding points."""
  v, scale, F, x = _prepare(votes, scale)
  R, Ho, Wo = v.shape
  P = Ho * Wo
  f32, f64 = np.float32, np.float64
  want = vote_posterior(v, scale, gt_index)
  stats = want[2].copy().astype(f32)
  if not F.any():
    return want[0].astype(f32), want[1].astype(f32), stats, want[3]
  vf = np.where(F, v, 0).reshape(R, P)
  Ff = F.reshape(R, P)
  with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
    x32 = np.where(Ff, scale * vf, f32(-np.inf)).astype(f32)
    m_p = x32.max(0)
    live = m_p > -np.inf
    mp0 = np.where(live, m_p, 0).astype(f64)
    d = np.where(Ff, (f64(scale) * vf.astype(f64) - mp0[None]), 0).astype(f32)        # fma: one rounding
    e = np.where(Ff, np.exp(d), f32(0)).astype(f32)
    s_p, t_p = np.zeros(P, f32), np.zeros(P, f32)
    for r in range(R):
      s_p = (s_p + e[r]).astype(f32)
      t_p = (t_p + (e[r] * d[r]).astype(f32)).astype(f32)
    nt = -(-P // TILE)
    pad = nt * TILE - P
    m_t = np.pad(m_p, (0, pad), constant_values=-np.inf).reshape(nt, TILE).max(1)
    m_t_p = np.repeat(m_t, TILE)[:P]
    f_p = np.where(live, np.exp(np.where(live, m_p - m_t_p, 0).astype(f32)), 0).astype(f32)
    M = f64(m_t.max())
    fg = np.where(m_t > -np.inf, np.exp(m_t.astype(f64) - M), 0.0)               # [nt]
    fg_p = np.repeat(fg, TILE)[:P]
    # per-rotation sums: f32 product, f32 sum over each wave of 64 pixels, float64 above
    wr = np.pad((e * f_p[None]).astype(f32), ((0, 0), (0, pad))).reshape(R, nt, TILE // 64, 64)
    s_r = (wr.sum(-1, dtype=f32).astype(f64).sum(-1) * fg[None]).sum(-1)
    W = s_p.astype(f64) * f_p.astype(f64) * fg_p
    T = fg_p * f_p.astype(f64) * (t_p.astype(f64) + (mp0 - np.where(live, m_t_p, 0).astype(f64)) * s_p.astype(f64))
    T = T + W * (np.where(live, m_t_p, 0).astype(f64) - M)                         # relative to M
    Zp = W.sum()
    logZp = np.log(Zp)
    log_z = M + logZp
    lxy = np.where(live, (mp0 - M) + np.log(np.where(live, s_p, 1).astype(f64)) - logZp, -np.inf)
    lr = np.where(s_r > 0, np.log(np.where(s_r > 0, s_r, 1)) - logZp, -np.inf)
  a, b = (np.arange(P) // Wo).astype(f64), (np.arange(P) % Wo).astype(f64)
  ea, eb = (W * a).sum() / Zp, (W * b).sum() / Zp
  ang = 2 * np.pi * np.arange(R) / R
  C, S = (np.cos(ang) * s_r).sum() / s_r.sum(), (np.sin(ang) * s_r).sum() / s_r.sum()
  out = [log_z, M, ea, eb, (W * a * a).sum() / Zp - ea * ea, (W * a * b).sum() / Zp - ea * eb,
         (W * b * b).sum() / Zp - eb * eb, C, S, (np.arctan2(S, C) * R / (2 * np.pi)) % R, np.hypot(C, S),
         logZp - T.sum() / Zp]
  stats[:12] = np.array(out, f64).astype(f32)
  if stats[9] >= R:
    stats[9] = 0
  _, valid, taps = _gt_sample(v, F, x, gt_index)
  if valid:
    stats[12] = f32(sum(w * f64(scale * v[r_, a_, b_]) for w, r_, a_, b_ in taps) - log_z)
  return lxy.reshape(Ho, Wo).astype(f32), lr.astype(f32), stats, want[3]


# ---- the inputs the CPU and GPU tests share -------------------------------------------------------------------------
RANDOM_SHAPES = [(4, 7, 7), (36, 31, 33), (1, 5, 5), (64, 5, 300), (3, 1, 1)]
PEAK_SHAPE = (8, 200, 210)


def random_votes(shape, seed=0):
  """Uniform votes in [-1, 1], 30 % of the cells -inf."""
  rng = np.random.default_rng(seed + 7 * sum(shape))
  v = rng.uniform(-1, 1, shape).astype(np.float32)
  v[rng.random(shape) < 0.3] = -np.inf
  if not np.isfinite(v).any():
    v.reshape(-1)[0] = 0.25
  return v


def exact_votes(shape, seed=0):
  """Votes in {0, -inf}: with scale 1 every exponential is exactly 1 or 0."""
  rng = np.random.default_rng(seed + 11 * sum(shape))
  v = np.where(rng.random(shape) < 0.4, np.float32(0), np.float32(-np.inf)).astype(np.float32)
  v.reshape(-1)[-1] = 0
  return v


def single_cell_votes(shape=(36, 31, 33), value=-3.25):
  v = np.full(shape, -np.inf, np.float32)
  c = tuple(s // 2 for s in shape)
  v[c] = value
  return v, c


def peak_votes(shape=PEAK_SHAPE):
  """A sharp Gaussian log-score in the far corner: sigma 0.7 cells around (Ho - 1.3, Wo - 1.6), every rotation."""
  R, Ho, Wo = shape
  a, b = np.arange(Ho, dtype=np.float64)[:, None], np.arange(Wo, dtype=np.float64)[None, :]
  x = -((a - (Ho - 1.3)) ** 2 + (b - (Wo - 1.6)) ** 2) / (2 * 0.7 ** 2)
  return np.broadcast_to(x.astype(np.float32), shape).copy()


def nan_inf_votes(shape=(36, 31, 33)):
  """(votes with a few NaN / +inf cells planted, the same votes with those cells masked instead, cells planted)."""
  v = random_votes(shape, seed=5)
  cells = [(0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1), (3, 8, 32), (3, 8, 31), (17, 30, 0)]
  bad, masked = v.copy(), v.copy()
  for n, c in enumerate(cells):
    bad[c] = np.inf if n % 2 else np.nan
    masked[c] = -np.inf
  return bad, masked, len(cells)


def gt_cases(shape=(36, 31, 33)):
  """(votes, [(name, (k, i, j), valid)]) for the ground-truth sample."""
  R, Ho, Wo = shape
  rng = np.random.default_rng(99)
  v = rng.uniform(-1, 1, shape).astype(np.float32)
  v[5, 10, 12] = -np.inf                                    # a masked tap
  cases = [('interior', (7.25, 3.5, 20.75), 1), ('integer', (2.0, 4.0, 9.0), 1), ('wrap', (R - 0.25, 6.5, 6.5), 1),
           ('last_row', (1.5, float(Ho - 1), 3.25), 1), ('last_col_corner', (0.0, float(Ho - 1), float(Wo - 1)), 1),
           ('past_last_row', (1.5, Ho - 0.5, 3.25), 0), ('masked_tap', (4.5, 9.5, 11.5), 0),
           ('masked_tap_weight_zero', (6.0, 10.0, 12.0), 1), ('nan', (np.nan, 3.0, 3.0), 0),
           ('negative', (1.0, -0.25, 3.0), 0), ('negative_k', (-0.5, 2.0, 2.5), 1)]
  return v, cases


FOLD_SHAPE = (2, 520, 520)     # 1057 tiles of 256 pixels > 1024 workgroups: workgroups 0 .. 32 own two tiles each


def fold_votes(shape=FOLD_SHAPE):
  """Uniform votes in [-1, 1], 30 % masked, on a plane of more than 1024 tiles: workgroup g < 33 folds tile g and
  then tile g + 1024.  Tiles 0 .. 9 are fully masked (a masked tile BEFORE a live one), tiles 1040 .. 1049 too (a
  live one before a masked one); tiles 10 .. 15 are raised by 35 and tiles 1024 .. 1039 by 20, so workgroups
  0 .. 9 and 16 fold a low first maximum into a high second one, 10 .. 15 a high first one into a lower second."""
  R, Ho, Wo = shape
  P = Ho * Wo
  v = random_votes(shape, seed=21).reshape(R, P)
  tile = np.arange(P) // TILE
  v[:, (tile < 10) | ((tile >= 1040) & (tile < 1050))] = -np.inf
  fin = np.isfinite(v)
  v[:, (tile >= 10) & (tile < 16)] += np.float32(35)
  v[:, (tile >= 1024) & (tile < 1040)] += np.float32(20)
  v[~fin] = -np.inf
  return np.ascontiguousarray(v.reshape(shape))


def aniso_votes(shape=(8, 31, 31), centre=(15.0, 9.0), sigma=(3.0, 1.0)):
  """A Gaussian log-score on rotation 0 alone, wider along a than along b, off-centre."""
  R, Ho, Wo = shape
  a, b = np.arange(Ho, dtype=np.float64)[:, None], np.arange(Wo, dtype=np.float64)[None, :]
  v = np.full(shape, -np.inf, np.float32)
  v[0] = (-(a - centre[0]) ** 2 / (2 * sigma[0] ** 2) - (b - centre[1]) ** 2 / (2 * sigma[1] ** 2)).astype(np.float32)
  return v


def all_inputs():
  """[(name, votes, scale, gt_index)]: every input of the GPU tests that is compared within the bound."""
  out = []
  for shape in RANDOM_SHAPES:
    for scale in (1.0, 30.0):
      out.append(('random%s_s%g' % (shape, scale), random_votes(shape), scale, None))
  out.append(('exact', exact_votes((36, 31, 33)), 1.0, None))
  out.append(('single', single_cell_votes()[0], 2.5, None))
  out.append(('nan_inf', nan_inf_votes()[0], 30.0, None))
  out.append(('peak', peak_votes(), 1.0, None))
  out.append(('fold', fold_votes(), 1.0, (0.5, 517.25, 103.5)))
  out.append(('aniso', aniso_votes(), 1.0, None))
  v, cases = gt_cases()
  for name, idx, _ in cases:
    out.append(('gt_' + name, v, 3.0, idx))
  return out
