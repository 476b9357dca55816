"""A vote volume under a road / lane RASTER prior on the map grid (``ops.raster_volume``): the host table, the entry
point that runs it over a ladder of prior strengths, and the fit of the strength against ground truth."""
import numpy as np
import torch

from snap_amd import ops
from snap_amd.models.pose_exhaustive_voting import exhaustive_tfm_to_index
from snap_amd.models.votes.lattice import _check_planes, _host_f64
from snap_amd.models.votes.temper import solve_temperature

RASTER_MAX_STRENGTHS = 8
RASTER_MAX_CONCENTRATION = 700.0   # np.i0 overflows in float64 beyond about 713
RASTER_MAX_OFFSET = 2.0 ** 23      # cells
RASTER_MAX_LOG_PRIOR = 2.0 ** 120  # the largest |lambda g| a cell may reach: far inside f32


def _tap_weights(planes):
  """The four bilinear weights per rotation, f32 [R, 4] for the taps (0,0), (0,1), (1,0), (1,1), formed in f32 exactly
  as the kernel forms them from (f_a, f_b)."""
  fa, fb = planes[:, 0].astype(np.float32), planes[:, 1].astype(np.float32)
  ga, gb = np.float32(1) - fa, np.float32(1) - fb
  return np.stack([ga * gb, ga * fb, fa * gb, fa * fb], -1)


class RasterPrior:
  """The host table of ``raster_prior`` (float64 / the f32 and int32 roundings the kernel reads; no device work):
  ``raster`` f32 [X, Y, 4] = (A, C, S, valid as 1.0 / 0.0), ``offset`` float64 [R, 2] = o_k (in raster index units the
  lattice cell (k, a, b) sits at (a, b) + o_k), ``offsets`` int32 [R, 2] = floor(o_k), ``planes`` f32 [R, 4] = (o_k -
  floor(o_k), cos(h theta_k), sin(h theta_k)), ``outside`` (a float, finite or -inf), ``strengths`` float64 [S] (the
  values of their f32 roundings), ``harmonic`` and ``shape`` = (R, Ho, Wo) of the lattice it was built for.
  ``log_prior(k, a, b)`` evaluates g of cells in float64 from the rounded table."""

  def __init__(self, shape, raster, offset, offsets, planes, outside, strengths, harmonic):
    self.shape = shape
    self.raster, self.offset, self.offsets, self.planes = raster, offset, offsets, planes
    self.outside, self.strengths, self.harmonic = float(outside), strengths, int(harmonic)
    self.num_strengths = int(strengths.size)

  def log_prior(self, k, a, b):
    k, a, b = np.broadcast_arrays(*(np.asarray(v) for v in (k, a, b)))
    X, Y = self.raster.shape[:2]
    w = _tap_weights(self.planes).astype(np.float64)[k]                       # [..., 4]
    cs = self.planes[:, 2:].astype(np.float64)[k]
    xa, yb = a + self.offsets[k, 0].astype(np.int64), b + self.offsets[k, 1].astype(np.int64)
    acc = np.zeros(k.shape + (3,))
    ok = np.ones(k.shape, bool)
    for tap in range(4):
      x, y = xa + (tap >> 1), yb + (tap & 1)
      used = w[..., tap] != 0
      inside = (x >= 0) & (x < X) & (y >= 0) & (y < Y)
      q = self.raster[np.clip(x, 0, X - 1), np.clip(y, 0, Y - 1)].astype(np.float64)
      ok &= ~used | (inside & (q[..., 3] != 0))
      acc += np.where((used & inside)[..., None], w[..., tap, None] * np.nan_to_num(q[..., :3]), 0.0)
    g = acc[..., 0] + cs[..., 0] * acc[..., 1] + cs[..., 1] * acc[..., 2]
    return np.where(ok, g, self.outside)


def _plane(fn, value, name, shape=None):
  v = np.asarray(_host_f64(value) if torch.is_tensor(value) else value, dtype=np.float64)
  if v.ndim != 2 or v.size == 0 or (shape is not None and v.shape != shape):
    raise ValueError(f'{fn}: {name} [X, Y]{"" if shape is None else f" = {list(shape)}"}, got {list(v.shape)}')
  return v


def raster_prior(grid, num_rotations, log_area=None, valid=None, heading=None, concentration=None, harmonic=1,
                 outside=-np.inf, origin=(0.0, 0.0), sensor_q=None, normalise_heading=True, strengths=(1.0,)):
  """A raster prior over position and heading for ``raster_votes`` -> ``RasterPrior`` (host, float64, no device work).

  The rasters live on a map grid of ``grid.cell_size`` whose cell (i, j) has its centre at ((i, j) + 0.5) cell_size +
  ``origin`` (metres, MAP corner frame; the BEV grid itself has origin 0): ``log_area`` [X, Y], the log-prior A of the
  sensor's position (None: 0); ``valid`` [X, Y] bool (None: every cell); ``heading`` [X, Y], the lane direction phi as a
  yaw of m_t_q in radians, with the von Mises ``concentration`` kappa >= 0, a number or [X, Y] (default 1; ``heading``
  None: no heading term).  ``harmonic`` h = 1 for directed lanes, 2 for undirected road axes (phi and phi + pi are then
  the same).  At least one of ``log_area`` and ``heading`` must be given.  ``sensor_q`` [2] (metres) is the point of the
  QUERY corner frame the rasters are read at; default the grid centre c = extent_meters / 2.  ``outside`` is the value
  of g where the raster has no data (off the raster, or an invalid cell): a finite number, or -inf, the cell is
  impossible.  ``strengths``: the ladder lambda_s > 0 of 1 to 8 prior strengths (rounded to f32).

  With alpha_k = 2 pi k / R, theta_k = -alpha_k, e = extent - 1.5 and cell = grid.cell_size, the pose of the index
  (k, a, b) (``exhaustive_indices_to_tfm``) puts the sensor at c + ((a, b) - e) cell + Rot(theta_k) (sensor_q - c), which
  is the raster position (a, b) + o_k with o_k = (c - origin + Rot(theta_k) (sensor_q - c)) / cell - e - 0.5.  The table
  holds n_k = floor(o_k) (int32) and f_k = o_k - n_k in [0, 1) (f32): the bilinear weights are constants of a rotation
  plane, and f_k = 0 (one tap) for the default sensor on an even extent.  The planes are A (with -log I0(kappa) folded
  in under ``normalise_heading``: the heading factor is then a normalised density up to 2 pi), C = kappa cos(h phi)
  and S = kappa sin(h phi), so that g = bilin A + cos(h theta_k) bilin C + sin(h theta_k) bilin S = bilin [A + kappa
  cos(h (theta_k - phi))].

  Raises ValueError for a non-finite A, C or S on a valid cell, kappa < 0 or > 700, a harmonic other than 1 or 2,
  strengths that are not finite numbers > 0 as f32 or more than 8 of them, mismatched raster shapes, an ``outside``
  that is NaN or +inf, an offset beyond 2^23 cells and a max lambda times max |g| that reaches 2^120."""
  fn = 'raster_prior'
  R = int(num_rotations)
  if not 1 <= R <= 64:
    raise ValueError(f'{fn}: 1 <= num_rotations <= 64, got {R}')
  if harmonic not in (1, 2):
    raise ValueError(f'{fn}: harmonic must be 1 (directed lanes) or 2 (road axes), got {harmonic!r}')
  h = int(harmonic)
  if log_area is None and heading is None:
    raise ValueError(f'{fn}: at least one of log_area and heading must be given')
  if heading is None and concentration is not None:
    raise ValueError(f'{fn}: a concentration without a heading')
  lam = np.asarray(strengths, dtype=np.float64).reshape(-1)
  with np.errstate(over='ignore'):
    lam32 = lam.astype(np.float32)
  if not (1 <= lam.size <= RASTER_MAX_STRENGTHS and bool(np.all(np.isfinite(lam32))) and bool(np.all(lam32 > 0))):
    raise ValueError(f'{fn}: strengths must be 1 to {RASTER_MAX_STRENGTHS} finite numbers > 0 as f32, got '
                     f'{lam.tolist()}')
  outside = float(outside)
  if not outside < np.inf:
    raise ValueError(f'{fn}: outside must be a finite number or -inf, got {outside}')
  A = None if log_area is None else _plane(fn, log_area, 'log_area')
  shape = A.shape if A is not None else None
  phi = None if heading is None else _plane(fn, heading, 'heading', shape)
  shape = shape if shape is not None else phi.shape
  ok = np.ones(shape, bool) if valid is None else _plane(fn, valid, 'valid', shape) != 0
  A = np.zeros(shape) if A is None else A.copy()
  C, S = np.zeros(shape), np.zeros(shape)
  if phi is not None:
    kappa = np.asarray(1.0 if concentration is None else
                       (_host_f64(concentration) if torch.is_tensor(concentration) else concentration), np.float64)
    if kappa.ndim not in (0, 2) or (kappa.ndim == 2 and kappa.shape != shape):
      raise ValueError(f'{fn}: concentration a number or {list(shape)}, got {list(kappa.shape)}')
    kappa = np.broadcast_to(kappa, shape)
    bad = ok & ~((kappa >= 0) & (kappa <= RASTER_MAX_CONCENTRATION))     # (a NaN is bad too)
    if bad.any():
      raise ValueError(f'{fn}: 0 <= concentration <= {RASTER_MAX_CONCENTRATION:g} on valid cells, got '
                       f'{kappa[bad].ravel()[:4].tolist()}')
    kv = np.where(ok, kappa, 0.0)
    with np.errstate(invalid='ignore'):
      C, S = kv * np.cos(h * phi), kv * np.sin(h * phi)
    if normalise_heading:
      A = A - np.log(np.i0(kv))
  for name, plane in (('log_area', A), ('the cosine plane', C), ('the sine plane', S)):
    if not np.isfinite(plane[ok]).all():
      raise ValueError(f'{fn}: {name} is not finite on every valid cell')
  planes4 = np.zeros(shape + (4,), np.float32)
  with np.errstate(over='ignore'):
    for i, plane in enumerate((A, C, S)):
      planes4[..., i] = np.where(ok, plane, 0.0).astype(np.float32)
  planes4[..., 3] = ok
  gmax = float(np.abs(planes4[..., :3].astype(np.float64)).sum(-1).max())
  gmax = max(gmax, abs(outside) if np.isfinite(outside) else 0.0)
  if not (np.isfinite(planes4).all() and float(lam32.max()) * gmax < RASTER_MAX_LOG_PRIOR):
    raise ValueError(f'{fn}: the largest strength {float(lam32.max())} times the largest |g| {gmax:.3g} leaves f32 '
                     '(the limit is 2^120)')
  cell = float(grid.cell_size)
  extent = np.asarray(grid.extent, np.float64)[:2]
  Ho, Wo = (int(2 * v - 1) for v in extent)
  c = extent * cell / 2
  e = extent - 1.5
  try:
    s = c if sensor_q is None else np.asarray(_host_f64(sensor_q), np.float64).reshape(2)
    org = np.asarray(_host_f64(origin), np.float64).reshape(2)
  except (TypeError, ValueError):
    raise ValueError(f'{fn}: sensor_q and origin must be [2] numbers') from None
  if not (np.isfinite(s).all() and np.isfinite(org).all()):
    raise ValueError(f'{fn}: sensor_q {s.tolist()} or origin {org.tolist()} is not finite')
  theta = -2 * np.pi * np.arange(R) / R
  snap = lambda v: np.where(np.abs(v) < 2.0 ** -40, 0.0, v)   # (a quarter turn is exact)
  cos, sin = snap(np.cos(theta)), snap(np.sin(theta))
  lever = np.stack([cos * (s - c)[0] - sin * (s - c)[1], sin * (s - c)[0] + cos * (s - c)[1]], -1)   # [R, 2]
  offset = (c - org + lever) / cell - e - 0.5
  if not np.abs(offset).max() <= RASTER_MAX_OFFSET:
    raise ValueError(f'{fn}: an offset of {np.abs(offset).max():.3g} cells; the limit is 2^23')
  n = np.floor(offset)
  f = (offset - n).astype(np.float32)
  carry = f >= 1                                            # (a tiny negative fraction rounds up to 1 in f32)
  n, f = n + carry, np.where(carry, np.float32(0), f)
  planes = np.concatenate([f, snap(np.cos(h * theta))[:, None], snap(np.sin(h * theta))[:, None]], -1)
  return RasterPrior((R, Ho, Wo), np.ascontiguousarray(planes4), offset, np.ascontiguousarray(n.astype(np.int32)),
                     np.ascontiguousarray(planes.astype(np.float32)), outside, lam32.astype(np.float64), h)


def raster_prior_from_logits(logits_areas, area_classes, drivable, grid, num_rotations, floor=1e-3, **kw):
  """``raster_prior`` with A = log(max(the softmax mass of the drivable classes, floor)): ``logits_areas`` [X, Y, n] is
  a ``SemanticNet`` prediction's ``logits_areas`` or any raster of n class logits, ``area_classes`` the n class names
  and ``drivable`` the names (or indices) of the classes a vehicle may stand on; ``floor`` in (0, 1] keeps a pose off
  the predicted road possible.  Host, float64; ``**kw`` goes to ``raster_prior`` (``valid``, ``heading``, ...)."""
  fn = 'raster_prior_from_logits'
  z = np.asarray(_host_f64(logits_areas), np.float64)
  names = list(area_classes)
  if z.ndim != 3 or z.shape[-1] != len(names):
    raise ValueError(f'{fn}: logits_areas [X, Y, {len(names)}], got {list(z.shape)}')
  floor = float(floor)
  if not 0.0 < floor <= 1.0:
    raise ValueError(f'{fn}: 0 < floor <= 1, got {floor}')
  try:
    idx = sorted({d if isinstance(d, (int, np.integer)) else names.index(d) for d in drivable})
  except ValueError:
    raise ValueError(f'{fn}: drivable {list(drivable)} must name classes of {names}') from None
  if not idx or not all(0 <= i < len(names) for i in idx):
    raise ValueError(f'{fn}: drivable must select at least one of the {len(names)} classes, got {list(drivable)}')
  if not np.isfinite(z).all():
    raise ValueError(f'{fn}: logits_areas is not finite')
  z = z - z.max(-1, keepdims=True)
  p = np.exp(z)
  mass = p[..., idx].sum(-1) / p.sum(-1)
  return raster_prior(grid, num_rotations, log_area=np.log(np.maximum(mass, floor)), **kw)


def _gt_linear(m_t_q_gt, grid, num_rotations, shape):
  """The flat index of the cell nearest a ground-truth pose (read on the host), or -1 outside the lattice."""
  if m_t_q_gt is None:
    return -1
  R, Ho, Wo = shape
  gt = _host_f64(exhaustive_tfm_to_index(m_t_q_gt, grid, num_rotations)).reshape(3)
  if not np.isfinite(gt).all():
    return -1
  k, a, b = int(np.rint(gt[0])) % R, int(np.rint(gt[1])), int(np.rint(gt[2]))
  return (k * Ho + a) * Wo + b if 0 <= a < Ho and 0 <= b < Wo else -1


def _check_raster(fn, raster, grid, num_rotations):
  if not isinstance(raster, RasterPrior):
    raise ValueError(f'{fn}: raster must come from raster_prior, got {type(raster).__name__}')
  lattice = (int(num_rotations),) + tuple(int(2 * v - 1) for v in tuple(grid.extent)[:2])
  if raster.shape != lattice:
    raise ValueError(f'{fn}: the raster prior was built for the lattice {raster.shape}, not {lattice}')


def _strengths_on(raster, device):
  from snap_amd.models import base
  return base.device_const('vote_raster_strengths', device, lambda: torch.from_numpy(raster.strengths.copy()),
                           owner=raster)


def raster_votes(votes, raster, grid, num_rotations, temperature=1.0, strength=0, m_t_q_gt=None, device=None):
  """The measurement update with a ``raster_prior`` (``ops.raster_volume``): p_s = softmax(temperature * votes +
  lambda_s g) over the cells F of ``votes`` [R, 2H-1, 2W-1] that are finite and that the raster does not exclude, g the
  raster's interpolated log-prior, at every strength lambda_s of the prior's ladder from ONE visit -> dict of device
  tensors, nothing synchronised: ``votes`` (the normalised log-probabilities at the ladder index ``strength``, -inf =
  impossible: again a vote volume for every other operator); float64 [S]: ``log_z``, ``log_z_prior`` (of lambda_s g
  over the whole lattice), ``expected_log_prior`` = lambda_s E_s[g], ``variance_log_prior`` = lambda_s^2 Var_s[g],
  ``log_evidence`` = log_z - log_z_prior (the frame under the normalised prior), ``log_overlap`` = log_evidence -
  log_z_votes <= 0, ``information_gain`` = KL(p_s || votes alone) >= 0, ``log_prob_gt`` and ``log_prob_gt_slope`` = d
  log_prob_gt / d lambda = g_gt - E_s[g]; ``log_z_votes``: one float64 scalar (of temperature * votes over its finite
  cells); ``strengths`` float64 [S]; ``count`` int32 [4] = (finite cells, NaN / +inf cells, finite cells the raster
  excludes, cells whose mass underflowed at ``strength``); ``table`` [S, 4] and ``stats`` [4]: the op's raw rows.
  ``m_t_q_gt`` (a Transform2D, map corner frame; read on the host) is rounded to its nearest cell; without it, or
  outside the lattice, the two ground-truth rows are NaN; on an excluded or masked cell log_prob_gt is -inf.  ``votes``
  None returns the raster prior itself as a normalised belief, on ``device``."""
  _check_raster('raster_votes', raster, grid, num_rotations)
  if votes is not None:
    _check_planes('raster_votes', votes, num_rotations, 'votes')
    votes = votes.contiguous()
  gt = _gt_linear(m_t_q_gt, grid, num_rotations, raster.shape)
  out, table, stats, count = ops.raster_volume(votes, raster, temperature, write=strength, gt_index=gt, device=device)
  lam = _strengths_on(raster, out.device)
  log_z, log_z_prior, mean, var = table[:, 0], table[:, 1], table[:, 2], table[:, 3]
  return dict(votes=out, log_z=log_z, log_z_prior=log_z_prior, expected_log_prior=lam * mean,
              variance_log_prior=lam * lam * var, log_evidence=log_z - log_z_prior,
              log_overlap=(log_z - log_z_prior) - stats[0], information_gain=(lam * mean - log_z) + stats[0],
              log_prob_gt=(stats[1] + lam * stats[2]) - log_z, log_prob_gt_slope=stats[2] - mean,
              log_z_votes=stats[0], strengths=lam, count=count, table=table, stats=stats)


class RasterStrengthFit:
  """The one-parameter calibration of a raster prior: the strength lambda that minimises the ground-truth NLL of p_s =
  softmax(temperature * votes + lambda g) over a validation set, from ONE visit of every frame.  The ladder is the
  ``raster_prior``'s own ``strengths``, which must increase strictly.  ``add`` evaluates a frame on the whole ladder
  (``ops.raster_volume``) and adds, on the device in float64 and without a synchronisation beyond the read of the ground
  truth, the frame's nll, nll slope E_s[g] - g_gt and Var_s[g] per ladder point and the valid-frame count; a frame whose
  ground truth is invalid (outside the lattice, on a masked or excluded cell) adds nothing.  ``solve`` synchronises
  once."""

  def __init__(self, grid, num_rotations, raster, temperature=1.0):
    _check_raster('RasterStrengthFit', raster, grid, num_rotations)
    if not bool(np.all(np.diff(raster.strengths) > 0)):
      raise ValueError(f'RasterStrengthFit: the strengths must increase strictly, got {raster.strengths.tolist()}')
    self.grid, self.num_rotations, self.raster, self.temperature = grid, int(num_rotations), raster, float(temperature)
    self.strengths = raster.strengths
    self._sums = None                                            # float64 [S, 3] = (nll, slope, var)
    self._frames = None

  def add(self, votes, m_t_q_gt):
    _check_planes('RasterStrengthFit.add', votes, self.num_rotations, 'votes')
    gt = _gt_linear(m_t_q_gt, self.grid, self.num_rotations, self.raster.shape)
    _, table, stats, _ = ops.raster_volume(votes.contiguous(), self.raster, self.temperature, gt_index=gt)
    self.add_table(table, stats)

  def add_table(self, table, stats):
    """The same from a stored ``ops.raster_volume`` table [S, 4] and stats [4] (tensors on any one device)."""
    S = self.strengths.size
    if tuple(table.shape) != (S, 4) or tuple(stats.shape) != (4,):
      raise ValueError(f'RasterStrengthFit.add_table: table [{S}, 4] and stats [4], got {tuple(table.shape)} and '
                       f'{tuple(stats.shape)}')
    table, stats = table.to(torch.float64), stats.to(torch.float64)
    lam = _strengths_on(self.raster, table.device)
    valid = torch.isfinite(stats[1]) & torch.isfinite(stats[2]) & torch.isfinite(table[:, 0]).all()
    row = torch.stack((table[:, 0] - (stats[1] + lam * stats[2]), table[:, 2] - stats[2], table[:, 3]), -1)
    row = torch.where(valid, row, torch.zeros_like(row))
    if self._sums is None:
      self._sums, self._frames = row, valid.to(torch.int64)
    else:
      self._sums = self._sums + row
      self._frames = self._frames + valid.to(torch.int64)

  def solve(self):
    """-> dict(strength, bracket = (lo, hi), bracketed, argmin, nll [S] at the ladder points, slope [S], frames,
    strengths [S]): the NLL is convex in lambda with the slope sum (E_s[g] - g_gt) and the curvature sum Var_s[g], so
    ``solve_temperature``'s bracket and Hermite step apply as they stand.  ``argmin`` is the ladder index of the
    smallest summed NLL (-1 without a frame); ``strength`` the interior stationary point where the slope changes sign
    between neighbours, else the better end of the ladder (``bracketed`` False)."""
    S = self.strengths.size
    if self._sums is None:
      sums, frames = np.zeros((S, 3)), 0
    else:
      packed = torch.cat((self._sums.reshape(-1), self._frames.to(torch.float64).reshape(1))).cpu().numpy()
      sums, frames = packed[:-1].reshape(-1, 3), int(packed[-1])
    out = solve_temperature(self.strengths, sums[:, 0], sums[:, 1], sums[:, 2], frames)
    out['strength'] = out.pop('temperature')
    out['strengths'] = out.pop('temperatures')
    out['slope'] = sums[:, 1].copy()
    out['argmin'] = int(np.argmin(sums[:, 0])) if frames else -1
    return out
