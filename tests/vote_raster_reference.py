"""A float64 numpy restatement of the raster-prior table (``pose_exhaustive_voting.raster_prior``) and of the operator
``snap_vote_raster_f32`` (include/snap_hip.h), with the error bound of the f32 kernel against it.

``table`` restates the table's geometry for ANY lattice shape [R, Ho, Wo] (extent = ((Ho + 1) / 2, (Wo + 1) / 2), which
need not be whole: the operator itself knows no grid), rotation by rotation with a rotation matrix.  ``vote_raster``
evaluates the operator in float64 FROM THE ROUNDED TABLE (the f32 / int32 arrays the kernel reads; the four tap weights
are formed in f32 by the header's three operations each, which numpy's float32 arithmetic reproduces bit for bit, so
"a tap of weight exactly 0" is the same decision on both sides, and so is inside / outside: integer arithmetic).

``bound`` follows the header's rounding points, eps = 2^-24 (one rounding to nearest), with expf taken within 2 ulp
(E = 4 eps relative; the device library documents 1 ulp):

  bQ            per plane Q of A, C, S over T taps present: T products (eps |w Q| each) and T - 1 additions that round
                (the first adds to 0: exact), each eps times a partial sum <= Babs_Q = sum |w Q|: |dbQ| <= 2 T eps Babs_Q
                (T = 1 with w = 1: exact, bounded all the same);
  g             fl(c bC), fl(s bS): the factor's error times |c|, |s| <= 1 plus eps of the product; two additions of
                partial sums <= Gabs = Babs_A + |c| Babs_C + |s| Babs_S: |dg| <= (2 T + 3) eps Gabs;
  lg_s, x, t_s  dlg = lambda dg + eps |lambda g|; dx = eps |x| (0 without votes); dt = dx + dlg + eps |t|;
  a log-sum     of values z with errors dz over a set (``vote_prior_reference._log_sum_bound``): LSE(z + dz) - LSE(z),
                plus sum p eps min(|z - max|, 105) (the argument), E (expf), (R - 1) eps (one pixel's f32 sum), the
                denormal floor and 1e-13 (1 + |value|) for the float64 sums and the final log;
  out           dt_w + dlog_z_w + eps |out| (the rounding to f32);
  E_s[g]        with rho_i = expm1(dt_i + eps min(|d_i|, 105) + E) the relative error of a cell's weight (the common
                shift cancels in the ratio), eta = sum p rho + R eps: dE = [sum p rho |g - E| + sum p (1 + rho) dg +
                |E| R eps] / (1 - eta);
  Var_s[g]      the perturbed weights q = p (1 + r) / norm satisfy |q - p| <= p (rho + eta) / (1 - eta), and Var_q(g) =
                sum q (g - E)^2 - (E_q - E)^2, so the weights move the variance by at most W = sum p (rho + eta) (g -
                E)^2 / (1 - eta) + dE^2; the cells' own errors add 2 sqrt((Var + W) D) + D with D = sum p (1 + rho) dg^2 /
                (1 - eta) (Cauchy-Schwarz); the kernel forms S2 / S0 - (S1 / S0)^2 in float64 (1e-13 (1 + E[g^2])) with
                S1 and S2 summed in float64 but S0 from the pixels' f32 sums, S0 (1 + d) with |d| <= R eps, which does
                not cancel between the two terms: S2 / S0 - (S1 / S0)^2 moves by d (Var - E^2), at most R eps (Var + E^2);
Everything is multiplied by 1 + 2^-10 for the second-order terms left out.  The bound is a function of the input."""
import numpy as np

import vote_prior_reference as pr

EPS = pr.EPS
E_FN = pr.E_FN
TILE = 256
MAX_GROUPS = 1024
COLUMNS = ('log_z', 'log_z_prior', 'mean_g', 'var_g')
SHAPES = pr.SHAPES
FOLD_SHAPE = pr.FOLD_SHAPE
LADDERS = {1: (1.0,), 3: (0.25, 1.0, 3.0), 8: (0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)}
_lse = pr._lse


def table(shape, cell, log_area=None, valid=None, heading=None, concentration=None, harmonic=1, outside=-np.inf,
          origin=(0.0, 0.0), sensor_q=None, normalise_heading=True, strengths=(1.0,)):
  """-> dict(shape, raster f32 [X, Y, 4], offset float64 [R, 2], offsets int32 [R, 2], planes f32 [R, 4], outside,
  strengths float64 [S] (f32 values), harmonic)."""
  R, Ho, Wo = shape
  extent = np.array([(Ho + 1) / 2, (Wo + 1) / 2])
  c = extent * cell / 2
  e = extent - 1.5
  s = c if sensor_q is None else np.asarray(sensor_q, np.float64)
  given = log_area if log_area is not None else heading
  X, Y = np.asarray(given).shape
  ok = np.ones((X, Y), bool) if valid is None else np.asarray(valid, bool)
  A = np.zeros((X, Y)) if log_area is None else np.asarray(log_area, np.float64).copy()
  C, S = np.zeros((X, Y)), np.zeros((X, Y))
  if heading is not None:
    kappa = np.broadcast_to(np.asarray(1.0 if concentration is None else concentration, np.float64), (X, Y))
    C = kappa * np.cos(harmonic * np.asarray(heading, np.float64))
    S = kappa * np.sin(harmonic * np.asarray(heading, np.float64))
    if normalise_heading:
      A = A - np.log(np.i0(kappa))
  raster = np.zeros((X, Y, 4), np.float32)
  for i, plane in enumerate((A, C, S)):
    raster[..., i] = np.where(ok, plane, 0.0)
  raster[..., 3] = ok
  offset = np.zeros((R, 2))
  planes = np.zeros((R, 4))
  for k in range(R):
    th = -2 * np.pi * k / R
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    offset[k] = (c - np.asarray(origin, np.float64) + rot @ (s - c)) / cell - e - 0.5
    planes[k, 2:] = np.cos(harmonic * th), np.sin(harmonic * th)
  planes[:, 2:][np.abs(planes[:, 2:]) < 2.0 ** -40] = 0.0
  n = np.floor(offset)
  f = (offset - n).astype(np.float32)
  n, f = n + (f >= 1), np.where(f >= 1, np.float32(0), f)
  planes[:, :2] = f
  return dict(shape=tuple(shape), raster=raster, offset=offset, offsets=n.astype(np.int32),
              planes=planes.astype(np.float32), outside=float(outside),
              strengths=np.asarray(strengths, np.float32).astype(np.float64), harmonic=harmonic)


def sensor_position(shape, cell, k, a, b, sensor_q):
  return pr.sensor_position(shape, cell, k, a, b, sensor_q)


def weights(tab):
  """f32 [R, 4]: the taps (0,0), (0,1), (1,0), (1,1), by the header's f32 operations."""
  fa, fb = tab['planes'][:, 0], tab['planes'][:, 1]
  ga, gb = np.float32(1) - fa, np.float32(1) - fb
  return np.stack([ga * gb, ga * fb, fa * gb, fa * fb], -1).astype(np.float32)


def bilin(plane, ok, n, w, Ho, Wo):
  """One rotation plane: sum over the taps of non-zero weight of w * plane at (a + n_a + i, b + n_b + j), float64
  [Ho, Wo]; NaN where such a tap is off the raster or not ``ok``.  Also sum |w plane| and the number of taps present."""
  X, Y = plane.shape
  a = np.arange(Ho)[:, None] + int(n[0])
  b = np.arange(Wo)[None, :] + int(n[1])
  acc, mag = np.zeros((Ho, Wo)), np.zeros((Ho, Wo))
  good = np.ones((Ho, Wo), bool)
  taps = 0
  for tap in range(4):
    wt = float(w[tap])
    if wt == 0.0:
      continue
    taps += 1
    x, y = a + (tap >> 1), b + (tap & 1)
    inside = (x >= 0) & (x < X) & (y >= 0) & (y < Y)
    xc, yc = np.clip(x, 0, X - 1), np.clip(y, 0, Y - 1)
    good &= inside & ok[xc, yc]
    q = np.where(inside, plane[xc, yc], 0.0)
    acc += wt * q
    mag += np.abs(wt * q)
  return np.where(good, acc, np.nan), mag, taps


def log_prior(tab):
  """g [R, Ho, Wo] float64 (``outside`` where the raster has no data), Gabs, the taps per rotation [R] and the mask of
  the cells whose taps all hold data."""
  R, Ho, Wo = tab['shape']
  ras = tab['raster'].astype(np.float64)
  ok = tab['raster'][..., 3] != 0
  w = weights(tab)
  g, gabs, taps = np.zeros(tab['shape']), np.zeros(tab['shape']), np.zeros(R, int)
  inside = np.zeros(tab['shape'], bool)
  for k in range(R):
    c, s = float(tab['planes'][k, 2]), float(tab['planes'][k, 3])
    bA, mA, t = bilin(ras[..., 0], ok, tab['offsets'][k], w[k], Ho, Wo)
    bC, mC, _ = bilin(ras[..., 1], ok, tab['offsets'][k], w[k], Ho, Wo)
    bS, mS, _ = bilin(ras[..., 2], ok, tab['offsets'][k], w[k], Ho, Wo)
    gk = bA + c * bC + s * bS
    g[k] = np.where(np.isnan(gk), tab['outside'], gk)
    gabs[k] = mA + abs(c) * mC + abs(s) * mS
    taps[k] = t
    inside[k] = ~np.isnan(gk)
  return g, gabs, taps, inside


def _x(votes, tab):
  return np.zeros(tab['shape'], np.float32) if votes is None else votes.astype(np.float32)


def vote_raster(votes, tab, scale=1.0, write=0, gt=-1):
  """-> dict(out float64 [R, Ho, Wo], table float64 [S, 4], stats float64 [3] = (log_z_votes, x_gt, g_gt), count [3],
  zero_lo, zero_hi)."""
  g = log_prior(tab)[0]
  v = _x(votes, tab)
  V = np.isfinite(v)
  on = g > -np.inf
  F = V & on
  bad = int((np.isnan(v) | (v == np.inf)).sum())
  sc = 1.0 if votes is None else float(np.float32(scale))
  with np.errstate(invalid='ignore'):
    x = np.where(V, sc * v.astype(np.float64), -np.inf)
  lam = tab['strengths']
  tbl = np.zeros((lam.size, 4))
  stats = np.array([_lse(x[V]) if V.any() else -np.inf, np.nan, np.nan])
  if gt >= 0:
    vg = v.reshape(-1)[gt]
    stats[1] = sc * float(vg) if np.isfinite(vg) else (-np.inf if vg == -np.inf else np.nan)
    stats[2] = g.reshape(-1)[gt]
  out = np.full(tab['shape'], -np.inf)
  zero_lo = zero_hi = 0
  for s, l in enumerate(lam):
    tbl[s, 1] = _lse(l * g[on]) if on.any() else -np.inf
    if not F.any():
      tbl[s, 0], tbl[s, 2], tbl[s, 3] = -np.inf, np.nan, np.nan
      continue
    t = x[F] + l * g[F]
    tbl[s, 0] = _lse(t)
    p = np.exp(t - tbl[s, 0])
    tbl[s, 2] = float((p * g[F]).sum())
    tbl[s, 3] = float((p * (g[F] - tbl[s, 2]) ** 2).sum())
    if s == write:
      out[F] = t - tbl[s, 0]
      d = t - t.max()
      zero_lo, zero_hi = int((d < -105).sum()), int((d < -86).sum())
  return dict(out=out, table=tbl, stats=stats, count=[int(V.sum()), bad, int((V & ~on).sum())], zero_lo=zero_lo,
              zero_hi=zero_hi)


def bound(votes, tab, scale=1.0, write=0, gt=-1):
  """-> dict(out [R, Ho, Wo], table [S, 4], stats [3]): what the f32 kernel may differ by (the module docstring)."""
  R = tab['shape'][0]
  g, gabs, taps, inside = log_prior(tab)
  dg = np.where(inside, (2 * taps[:, None, None] + 3) * EPS * gabs + 2.0 ** -140, 0.0)   # (`outside` itself is exact)
  v = _x(votes, tab)
  V = np.isfinite(v)
  on = g > -np.inf
  F = V & on
  sc = 1.0 if votes is None else float(np.float32(scale))
  with np.errstate(invalid='ignore'):
    x = np.where(V, sc * v.astype(np.float64), 0.0)
  dx = np.zeros_like(x) if votes is None else EPS * np.abs(x)
  k = 1 + 2.0 ** -10
  lam = tab['strengths']
  tbl = np.zeros((lam.size, 4))
  stats = np.zeros(3)
  if V.any():
    stats[0] = k * pr._log_sum_bound(x[V], dx[V], R)
  if gt >= 0:
    stats[1] = k * dx.reshape(-1)[gt]
    stats[2] = k * dg.reshape(-1)[gt] if on.reshape(-1)[gt] else 0.0
  out = np.zeros(tab['shape'])
  for s, l in enumerate(lam):
    lg = l * np.where(on, g, 0.0)
    dlg = l * dg + EPS * np.abs(lg)
    if on.any():
      tbl[s, 1] = k * pr._log_sum_bound(lg[on], dlg[on], R)
    if not F.any():
      continue
    t = x + lg
    dt = dx + dlg + EPS * np.abs(t)
    tF, dtF, gF, dgF = t[F], dt[F], g[F], dg[F]
    tbl[s, 0] = k * pr._log_sum_bound(tF, dtF, R)
    log_z = _lse(tF)
    p = np.exp(tF - log_z)
    with np.errstate(over='ignore', invalid='ignore'):
      rho = np.expm1(dtF + EPS * np.minimum(np.abs(tF - tF.max()), 105.0) + E_FN)
      eta = float((p * rho).sum()) + R * EPS + 1e-13
      E = float((p * gF).sum())
      var = float((p * (gF - E) ** 2).sum())
      if eta < 0.5:
        dE = (float((p * rho * np.abs(gF - E)).sum()) + float((p * (1 + rho) * dgF).sum()) + abs(E) * R * EPS
              + 1e-13 * (1 + abs(E))) / (1 - eta)
        W = float((p * (rho + eta) * (gF - E) ** 2).sum()) / (1 - eta) + dE * dE
        D = float((p * (1 + rho) * dgF ** 2).sum()) / (1 - eta)
        tbl[s, 2] = k * dE
        tbl[s, 3] = k * (W + 2 * np.sqrt((var + W) * D) + D + R * EPS * (var + E * E)
                         + 1e-13 * (1 + float((p * gF * gF).sum())))
      else:
        tbl[s, 2] = tbl[s, 3] = np.inf
    if s == write:
      out = np.where(F, k * (dt + tbl[s, 0] + EPS * np.abs(t - log_z)), 0.0)
  return dict(out=out, table=tbl, stats=stats)


# ---- the inputs the CPU and GPU tests share (a seed per case) ----------------------------------
random_votes = pr.random_votes


def random_raster(X, Y, seed, invalid=True, kappa=None):
  """(log_area, valid, heading, concentration) [X, Y]: a smooth-free random log-prior in about [-6, 0], headings on the
  circle, concentrations from {0, 2, 40}, and (``invalid``) an invalid rectangle and scattered invalid cells, whose A
  holds NaN: nothing of an invalid cell may reach a result."""
  rng = np.random.default_rng(seed)
  A = -6.0 * rng.random((X, Y))
  phi = rng.uniform(-np.pi, np.pi, (X, Y))
  kap = np.full((X, Y), kappa, np.float64) if kappa is not None else rng.choice([0.0, 2.0, 40.0], (X, Y))
  ok = np.ones((X, Y), bool)
  if invalid and X * Y > 1:
    ok[X // 3: X // 3 + max(1, X // 5), Y // 2: Y // 2 + max(1, Y // 4)] = False
    ok[rng.random((X, Y)) < 0.03] = False
    ok[0, 0] = True
  return np.where(ok, A, np.nan), ok, phi, kap


def synthetic(shape, seed, S=1, harmonic=1, taps=4, cover='cut', outside=-np.inf, invalid=True, kappa=None):
  """A table on ``shape`` with the offsets set by hand.  ``taps`` = 1: f = 0 in every plane; 2: f = 0 on one axis,
  alternating with the rotation; 4: both fractions non-zero.  ``cover`` = 'covers': the raster holds every tap of the
  lattice; 'cut': it is smaller than the lattice and shifted with the rotation, so the lattice leaves it on every side
  (planes that miss it altogether included, where the lattice is a single cell)."""
  rng = np.random.default_rng(seed)
  R, Ho, Wo = shape
  if cover == 'covers':
    X, Y = Ho + 3, Wo + 3
    n = rng.integers(0, 2, (R, 2))
  else:
    X, Y = max(2, Ho - 3), max(2, Wo - 3)
    n = np.stack([-2 + (np.arange(R) % 2), -2 + ((np.arange(R) // 2) % 2)], -1)
  A, ok, phi, kap = random_raster(X, Y, seed + 1, invalid, kappa)
  tab = table(shape, 0.25, A, ok, phi, kap, harmonic, outside, strengths=LADDERS[S])
  f = rng.uniform(0.05, 0.95, (R, 2)).astype(np.float32)
  if taps == 1:
    f[:] = 0
  elif taps == 2:
    f[0::2, 0] = 0
    f[1::2, 1] = 0
  tab['offsets'] = np.ascontiguousarray(n.astype(np.int32))
  tab['planes'][:, :2] = f
  tab['offset'] = n + f.astype(np.float64)
  return tab


def fold_votes():
  return pr.fold_votes()
