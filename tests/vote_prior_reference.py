"""A float64 numpy restatement of the prior table (``pose_exhaustive_voting.pose_prior``) and of the operator
``snap_vote_prior_f32`` (include/snap_hip.h), with the error bound of the f32 kernel against it.

``table`` restates the table for ANY lattice shape [R, Ho, Wo] (extent = ((Ho + 1) / 2, (Wo + 1) / 2), which need not be
whole: the operator itself knows no grid).  ``vote_prior`` evaluates the operator in float64 FROM THE ROUNDED TABLE (the
f32 / int32 arrays the kernel reads; c = fl32(log w + y) is formed in f32 as the kernel does, one exact IEEE addition).

``bound`` follows the header's rounding points, eps = 2^-24 (one rounding to nearest), with the cell's f32 functions
taken within 2 ulp (E = 4 eps relative; the device library documents 1 ulp for expf and logf):

  da, db        one rounding each of an exact difference: eps |d| each;
  q             three products of two multiplications on factors carrying eps each (4 eps each, relative), two
                additions: |dq| <= 6.1 eps Qabs, Qabs = |Pxx da^2| + |2 Pxy da db| + |Pyy db^2|;
  term_m        one subtraction: dterm = 3.05 eps Qabs + eps |term|;
  u, M = 1      du = dterm;
  u, M > 1      log-sum-exp moves by at most log sum_m r_m exp(dterm_m), r the cell's responsibilities (evaluated as a
                difference of two log-sum-exps: a far component of weight 0 adds nothing), plus the evaluation:
                sum_m r_m eps |term_m - mx| (arguments), E (expf), (M - 1) eps (the f32 sum), E |log s| (logf), eps |u|
                (the last addition);
  x, t          dx = eps |x|, dt = dx + du + eps |t|;
  a log-sum     of values z with errors dz over a set: LSE(z + dz) - LSE(z) (weights each cell's error by its share),
                plus sum p eps min(|z - max|, 105) (the argument), E (expf), (R - 1) eps (one pixel's f32 sum), the
                denormal floor n 2^-149 / S and 1e-13 (1 + |value|) for the float64 sums and the final log;
  out           dt + dlog_z + eps |out| (the rounding to f32);
  E_post[u]     with rho_i = expm1(dt_i + eps min(|d_i|, 105) + E) the relative error of a cell's weight (the common
                shift cancels in the ratio), eta = sum p rho + R eps: [sum p rho |u - E| + sum p (1 + rho) du + |E| R eps]
                / (1 - eta);
  resp_m        [sum p (r_m ((1 + rho) (1 + rel_m) - 1)) + resp_m (eta + 2 R eps)] / (1 - eta), rel_m = expm1(dterm_m + du
                + eps |term_m - u| + E + eps); M = 1 is exactly 1 (bound 0).
Everything is multiplied by 1 + 2^-10 for the second-order terms left out.  The bound is a function of the input."""
import numpy as np

EPS = 2.0 ** -24
E_FN = 4 * EPS
TILE = 256
MAX_GROUPS = 1024
STATS = ('log_z', 'log_z_votes', 'log_z_prior', 'log_z_prior_F', 'expected_log_prior')
SHAPES = ((1, 5, 5), (3, 1, 1), (4, 7, 7), (36, 31, 33), (64, 5, 300))
FOLD_SHAPE = (2, 520, 520)
COMPONENTS = (1, 3, 8)


def _rows(v, tail, M=None):
  v = np.asarray(v, np.float64)
  if v.shape == tuple(tail):
    v = v[None]
  assert v.shape[1:] == tuple(tail), v.shape
  return v


def table(shape, cell, position=None, covariance=None, heading=None, concentration=None, weights=None, sensor_q=None):
  """-> dict(shape, weights [M], mu float64 [M, R, 2], centres int32 [M, R, 2], planes f32 [M, R, 3], comps f32 [M, 4])."""
  R, Ho, Wo = shape
  extent = np.array([(Ho + 1) / 2, (Wo + 1) / 2])
  c = extent * cell / 2
  e = extent - 1.5
  given = [np.asarray(v).shape[0] if np.asarray(v).ndim > d else 1
           for v, d in ((position, 1), (heading, 0), (weights, 0)) if v is not None]
  M = max(given)
  w = np.ones(M) if weights is None else _rows(weights, ())
  w = w / w.sum()
  s = c if sensor_q is None else np.asarray(sensor_q, np.float64)
  mu = np.zeros((M, R, 2))
  P = np.zeros((M, 3))
  y = np.zeros((M, R))
  for k in range(R):
    al = -2 * np.pi * k / R
    rot = np.array([[np.cos(al), -np.sin(al)], [np.sin(al), np.cos(al)]])
    lever = rot @ (s - c)
    for m in range(M):
      if position is not None:
        mu[m, k] = (_rows(position, (2,))[m] - c - lever) / cell + e
      if heading is not None:
        kappa = 1.0 if concentration is None else _rows(concentration, ())[m]
        y[m, k] = kappa * (np.cos(al - _rows(heading, ())[m]) - 1.0)
  if position is not None:
    for m in range(M):
      prec = np.linalg.inv(_rows(covariance, (2, 2))[m]) * cell ** 2
      P[m] = prec[0, 0], 0.5 * (prec[0, 1] + prec[1, 0]), prec[1, 1]
  n = np.rint(mu)
  planes = np.concatenate([mu - n, y[..., None]], -1).astype(np.float32)
  comps = np.concatenate([P, np.log(w)[:, None]], -1).astype(np.float32)
  return dict(shape=tuple(shape), weights=w, mu=mu, centres=n.astype(np.int32), planes=planes, comps=comps)


def sensor_position(shape, cell, k, a, b, sensor_q):
  """The map position of the query-frame point ``sensor_q`` under the pose of the index (k, a, b), float64."""
  R, Ho, Wo = shape
  extent = np.array([(Ho + 1) / 2, (Wo + 1) / 2])
  c = extent * cell / 2
  al = -2 * np.pi * k / R
  rot = np.array([[np.cos(al), -np.sin(al)], [np.sin(al), np.cos(al)]])
  return c + (np.array([a, b], np.float64) - (extent - 1.5)) * cell + rot @ (np.asarray(sensor_q, np.float64) - c)


def _cells(tab):
  """terms [M, R, Ho, Wo], Qabs [M, R, Ho, Wo] in float64 from the rounded table."""
  R, Ho, Wo = tab['shape']
  n = tab['centres'].astype(np.float64)
  f = tab['planes'].astype(np.float64)
  P = tab['comps'].astype(np.float64)
  cf = (tab['comps'][:, 3:4] + tab['planes'][:, :, 2]).astype(np.float64)   # fl32(log w + y): one exact IEEE addition
  a = np.arange(Ho, dtype=np.float64)[None, None, :, None]
  b = np.arange(Wo, dtype=np.float64)[None, None, None, :]
  da = (a - n[:, :, 0, None, None]) - f[:, :, 0, None, None]
  db = (b - n[:, :, 1, None, None]) - f[:, :, 1, None, None]
  A = P[:, 0, None, None, None] * da * da
  B = 2 * P[:, 1, None, None, None] * da * db
  C = P[:, 2, None, None, None] * db * db
  terms = cf[:, :, None, None] - 0.5 * (A + B + C)
  return np.broadcast_to(terms, (n.shape[0], R, Ho, Wo)), np.broadcast_to(np.abs(A) + np.abs(B) + np.abs(C),
                                                                          (n.shape[0], R, Ho, Wo))


def _lse(z, axis=None):
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    m = np.max(z, axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    r = m0 + np.log(np.sum(np.exp(z - m0), axis=axis, keepdims=True))
  return r.reshape(()) if axis is None else np.squeeze(r, axis)


def log_prior(tab):
  """u [R, Ho, Wo] float64 (and the terms [M, R, Ho, Wo])."""
  terms, _ = _cells(tab)
  return (terms[0] if terms.shape[0] == 1 else _lse(terms, 0)), terms


def _x(votes, tab, scale):
  if votes is None:
    return np.zeros(tab['shape'], np.float32)
  return votes.astype(np.float32)


def vote_prior(votes, tab, scale=1.0):
  """-> dict(out float64 [R, Ho, Wo], stats float64 [8], resp float64 [M], count [2], zero_lo, zero_hi)."""
  u, terms = log_prior(tab)
  v = _x(votes, tab, scale)
  F = np.isfinite(v)
  bad = int((np.isnan(v) | (v == np.inf)).sum())
  s = 1.0 if votes is None else float(np.float32(scale))
  with np.errstate(invalid='ignore'):
    x = np.where(F, s * v.astype(np.float64), -np.inf)
  t = np.where(F, x + u, -np.inf)
  M = terms.shape[0]
  stats = np.zeros(8)
  stats[2] = _lse(u)
  if not F.any():
    stats[[0, 1, 3]] = -np.inf
    stats[4] = np.nan
    return dict(out=t, stats=stats, resp=np.full(M, np.nan), count=[0, bad], zero_lo=0, zero_hi=0)
  stats[0] = _lse(t[F])
  stats[1] = _lse(x[F])
  stats[3] = _lse(u[F])
  p = np.where(F, np.exp(t - stats[0]), 0.0)
  stats[4] = float((p[F] * u[F]).sum())
  resp = np.array([(p[F] * np.exp(terms[m][F] - u[F])).sum() for m in range(M)])
  d = t[F] - t[F].max()
  return dict(out=np.where(F, t - stats[0], -np.inf), stats=stats, resp=resp, count=[int(F.sum()), bad],
              zero_lo=int((d < -105).sum()), zero_hi=int((d < -86).sum()))


def _log_sum_bound(z, dz, R):
  """The bound of one log-sum-exp of the values z (1-D, finite) carrying the errors dz."""
  n = z.size
  val = _lse(z)
  p = np.exp(z - val)
  S = float(np.exp(z - z.max()).sum())
  with np.errstate(over='ignore'):
    lip = float(_lse(z + dz) - val)
  return (lip + float((p * EPS * np.minimum(np.abs(z - z.max()), 105.0)).sum()) + E_FN + (R - 1) * EPS
          + n * 2.0 ** -149 / S + 1e-13 * (1 + abs(float(val))))


def bound(votes, tab, scale=1.0):
  """-> dict(out [R, Ho, Wo], stats [8], resp [M]): what the f32 kernel may differ by (the module docstring)."""
  R = tab['shape'][0]
  u, terms = log_prior(tab)
  _, Qabs = _cells(tab)
  M = terms.shape[0]
  dterm = 3.05 * EPS * Qabs + EPS * np.abs(terms) + 2.0 ** -140
  if M == 1:
    du = dterm[0]
  else:
    mx = terms.max(0)
    r = np.exp(terms - u)
    with np.errstate(over='ignore'):
      lip = _lse(terms + dterm, 0) - u
    log_s = u - mx
    du = lip + (r * EPS * np.abs(terms - mx)).sum(0) + E_FN + (M - 1) * EPS + E_FN * np.abs(log_s) + EPS * np.abs(u)
  v = _x(votes, tab, scale)
  F = np.isfinite(v)
  s = 1.0 if votes is None else float(np.float32(scale))
  with np.errstate(invalid='ignore'):
    x = np.where(F, s * v.astype(np.float64), 0.0)
  dx = np.zeros_like(x) if votes is None else EPS * np.abs(x)
  t = x + u
  dt = dx + du + EPS * np.abs(t)
  k = 1 + 2.0 ** -10
  stats = np.zeros(8)
  stats[2] = k * _log_sum_bound(u.reshape(-1), du.reshape(-1), R)
  out = np.zeros(tab['shape'])
  resp = np.zeros(M)
  if not F.any():
    return dict(out=out, stats=stats, resp=resp)
  tF, dtF, uF, duF = t[F], dt[F], u[F], du[F]
  stats[0] = k * _log_sum_bound(tF, dtF, R)
  stats[1] = k * _log_sum_bound(x[F], dx[F], R)
  stats[3] = k * _log_sum_bound(uF, duF, R)
  if _lse(uF) - u.max() < -80:   # the prior's f32 mass on F is in the denormals or gone: -inf is a right answer
    stats[3] = np.inf
  log_z = _lse(tF)
  p = np.exp(tF - log_z)
  with np.errstate(over='ignore', invalid='ignore'):
    rho = np.expm1(dtF + EPS * np.minimum(np.abs(tF - tF.max()), 105.0) + E_FN)
    eta = float((p * rho).sum()) + R * EPS + 1e-13
    Eu = float((p * uF).sum())
    if eta < 0.5:
      stats[4] = k * (float((p * rho * np.abs(uF - Eu)).sum()) + float((p * (1 + rho) * duF).sum())
                      + abs(Eu) * R * EPS + 1e-13 * (1 + abs(Eu))) / (1 - eta)
    else:
      stats[4] = np.inf
    if M > 1:
      for m in range(M):
        tm = terms[m][F]
        rm = np.exp(tm - uF)
        rel = np.expm1(dterm[m][F] + duF + EPS * np.abs(tm - uF) + E_FN + EPS)
        grow = np.where(rm > 0, rm * ((1 + rho) * (1 + rel) - 1), 0.0)
        resp[m] = (k * (float((p * grow).sum()) + float((p * rm).sum()) * (eta + 2 * R * EPS) + 1e-13) / (1 - eta)
                   if eta < 0.5 else np.inf)
  out = np.where(F, k * (dt + stats[0] + EPS * np.abs(t - log_z)), 0.0)
  return dict(out=out, stats=stats, resp=resp)


# ---- the inputs the CPU and GPU tests share (a seed per case) ----------------------------------
def random_votes(shape, seed, spread=4.0):
  """Random votes with -inf patches: a masked rectangle in every rotation, one masked rotation strip, single cells."""
  rng = np.random.default_rng(seed)
  R, Ho, Wo = shape
  v = (rng.standard_normal(shape) * spread).astype(np.float32)
  if Ho * Wo > 1:
    v[:, : max(1, Ho // 4), : max(1, Wo // 3)] = -np.inf
    v[R // 2, Ho // 2:, :] = -np.inf
    v[rng.random(shape) < 0.05] = -np.inf
    v[0, Ho - 1, Wo - 1] = 1.0             # (never all masked)
  return v


def random_table(shape, M, seed, sigma_cells=None, kappa=None, sensor=True, outside=False, cross=True):
  """A table of M components on ``shape`` (cell 0.25 m): centres inside the lattice (one outside it with ``outside``),
  covariances with a cross term (``cross``), a sensor off the grid centre (``sensor``)."""
  rng = np.random.default_rng(seed)
  R, Ho, Wo = shape
  cell = 0.25
  extent = np.array([(Ho + 1) / 2, (Wo + 1) / 2])
  lo = (0 - (extent - 1.5)) * cell + extent * cell / 2
  hi = (np.array([Ho - 1, Wo - 1]) - (extent - 1.5)) * cell + extent * cell / 2
  pos = lo + rng.random((M, 2)) * (hi - lo)
  if outside:
    pos[0] = hi + np.array([3.3, 7.1]) * cell
  cov = np.zeros((M, 2, 2))
  for m in range(M):
    sg = (sigma_cells if sigma_cells is not None else rng.uniform(1.0, 6.0)) * cell
    sa, sb = sg, sg * rng.uniform(0.5, 2.0)
    rho = rng.uniform(-0.7, 0.7) if cross else 0.0
    cov[m] = [[sa * sa, rho * sa * sb], [rho * sa * sb, sb * sb]]
  head = rng.uniform(-np.pi, np.pi, M)
  kap = np.full(M, kappa, np.float64) if kappa is not None else rng.choice([0.0, 2.0, 500.0], M)
  w = rng.uniform(0.2, 1.0, M)
  sq = extent * cell / 2 + (np.array([0.9, -0.6]) if sensor else 0.0)
  return table(shape, cell, pos, cov, head, kap, w, sq)


def fold_votes():
  """[2, 520, 520]: 1057 pixel tiles on 1024 workgroups, so workgroups 0 .. 32 carry their accumulators over a second
  tile; the first tiles are masked, the second-round tiles are live."""
  v = random_votes(FOLD_SHAPE, 77, spread=2.0)
  flat = v.reshape(2, -1)
  flat[:, : 3 * TILE] = -np.inf
  flat[:, MAX_GROUPS * TILE:] += 3.0
  return v
