"""A vote volume under a change of MAP frame (``ops.rebase_volume``), and under a position / heading prior in the map
frame (``ops.prior_volume``): the host tables of both and the entry points that run them."""
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.models.pose_exhaustive_voting import exhaustive_tfm_to_index
from snap_amd.models.votes.lattice import _check_planes, _host_f64


def rebase_table(new_t_old, grid, num_rotations):
  """The table of ``ops.rebase_volume`` for a change of MAP frame: ``new_t_old`` is one Transform2D in corner frames, the
  old map frame's pose in the new one, so new_t_q = new_t_old @ old_t_q -> (dk float, A float64 [2, 2], o float64 [2])
  on the host (a transform on the device is read back: one synchronisation).

  In centre frames new_t_old is (phi, sigma) with sigma = tau + (Rot(phi) - I) centre, centre = grid.extent_meters / 2.
  Composing it in FRONT of the pose of the index (r, a, b) and reading the index back (``exhaustive_index_to_tfm`` /
  ``exhaustive_tfm_to_index``) gives r' = (r - phi R / 2 pi) mod R and (a', b') = Rot(phi) ((a, b) - e) + e + sigma /
  cell_size with e = extent - 1.5: the same map for every rotation (the +0.5 cell offsets cancel).  The operator
  gathers, so the table is the inverse: the destination (r', a', b') reads the rotation r' - dk, dk = (-phi R / 2 pi)
  mod R in [0, R), and the plane position A (a', b') + o with A = Rot(-phi), o = e - A (e + sigma / cell_size).
  Float64 throughout; cos phi and sin phi are set to exactly 0 where their magnitude is below 2^-40, so a quarter turn
  is an exact permutation of the lattice; negative zeros are cleared.  The identity gives dk = 0, A = I, o = 0."""
  R = int(num_rotations)
  angle = torch.as_tensor(new_t_old.angle)
  if angle.numel() != 1:
    raise ValueError(f'rebase_table: one transform, got a transform of shape {tuple(angle.shape)}')
  phi = float(angle.detach().to('cpu', torch.float64).reshape(()))
  tau = torch.as_tensor(new_t_old.t).detach().to('cpu', torch.float64).reshape(2).numpy()
  if not (math.isfinite(phi) and np.isfinite(tau).all()):
    raise ValueError(f'rebase_table: the transform ({phi}, {tau.tolist()}) is not finite')
  cos, sin = (0.0 if abs(v) < 2.0 ** -40 else v for v in (math.cos(phi), math.sin(phi)))
  rot = np.array([[cos, -sin], [sin, cos]])
  centre = np.asarray(grid.extent_meters, np.float64)[:2] / 2
  sigma = tau + (rot @ centre - centre)
  e = np.asarray(grid.extent, np.float64)[:2] - 1.5
  A = rot.T + 0.0
  o = (e - A @ (e + sigma / float(grid.cell_size))) + 0.0
  dk = math.fmod((-phi / (2 * math.pi)) * R, R)
  if dk < 0:
    dk += R
  if not dk < R:                                            # (a yaw just above 0 rounds up to R)
    dk = 0.0
  return dk + 0.0, A, o


def rebase_votes(volume, new_t_old, grid, num_rotations, temperature=1.0):
  """Carry a vote volume or belief into another map frame (``ops.rebase_volume`` on ``rebase_table``): ``volume``
  [R, 2H-1, 2W-1] holds log-scores of the poses old_t_q in the OLD map frame; ``new_t_old`` (one Transform2D, corner
  frames) is the old frame's pose in the new one, so every pose becomes new_t_q = new_t_old @ old_t_q -- a composition
  on the map side, where ``fuse_votes`` and the filter's predict step compose on the query side; ``temperature``
  multiplies the volume -> dict of device tensors: ``votes`` [R, 2H-1, 2W-1] (normalised log-probabilities over the
  new frame's lattice; again a vote volume, for every other operator of the family), ``log_z`` (the log-sum-exp of
  temperature * volume), ``mass_kept`` (the share of the distribution that lies inside the new lattice), ``count``
  int32 [4] and ``stats`` float64 [4] (the op's raw rows).  Cells the old lattice did not cover are -inf."""
  _check_planes('rebase_votes', volume, num_rotations, 'volume')
  table = rebase_table(new_t_old, grid, num_rotations)
  out, stats, count = ops.rebase_volume(volume.contiguous(), table, temperature)
  return dict(votes=out, log_z=stats[0], mass_kept=stats[1], count=count, stats=stats)


PRIOR_MAX_COMPONENTS = 8
PRIOR_MAX_QUADRATIC = 2.0 ** 120   # the largest quadratic form 2 q a cell may reach: far inside f32


class PosePrior:
  """The host table of ``pose_prior`` (float64 / the f32 and int32 roundings the kernel reads; no device work):
  ``weights`` [M], ``mu`` [M, R, 2] the components' centres in index units per rotation plane, ``centres`` int32
  [M, R, 2] = rint(mu) and ``planes`` f32 [M, R, 3] = (mu - centres, heading term y), ``comps`` f32 [M, 4] = (Pxx,
  Pxy, Pyy, log w), ``shape`` = (R, Ho, Wo) of the lattice it was built for.  ``log_prior(k, a, b)`` evaluates the
  unnormalised log-prior u of cells in float64 from the rounded table."""

  def __init__(self, shape, weights, mu, centres, planes, comps):
    self.shape = shape
    self.weights, self.mu, self.centres, self.planes, self.comps = weights, mu, centres, planes, comps
    self.num_components = int(comps.shape[0])

  def log_prior(self, k, a, b):
    k, a, b = (np.asarray(v) for v in (k, a, b))
    n = self.centres.astype(np.float64)
    f = self.planes.astype(np.float64)
    P = self.comps.astype(np.float64)
    terms = []
    for m in range(self.num_components):
      da = (a - n[m, k, 0]) - f[m, k, 0]
      db = (b - n[m, k, 1]) - f[m, k, 1]
      q = P[m, 0] * da * da + 2 * P[m, 1] * da * db + P[m, 2] * db * db
      c = (self.comps[m, 3] + self.planes[m, k, 2]).astype(np.float64)   # (one f32 addition, as the kernel forms it)
      terms.append(c - 0.5 * q)
    terms = np.stack(terms)
    mx = terms.max(0)
    return terms[0] if self.num_components == 1 else mx + np.log(np.exp(terms - mx).sum(0))


def _prior_rows(fn, value, tail, name):
  """``value`` as float64 [M, *tail]; a single component may omit the leading dimension."""
  try:
    v = np.asarray(_host_f64(value) if torch.is_tensor(value) else value, dtype=np.float64)
  except (TypeError, ValueError):
    raise ValueError(f'{fn}: {name} must be numbers of shape [M, {", ".join(map(str, tail))}]'.replace(', ]', ']')) from None
  if v.shape == tuple(tail):
    v = v[None]
  if v.ndim != 1 + len(tail) or v.shape[1:] != tuple(tail):
    raise ValueError(f'{fn}: {name} of shape {list(tail)} or [M] + {list(tail)}, got {list(v.shape)}')
  if not np.isfinite(v).all():
    raise ValueError(f'{fn}: {name} is not finite')
  return v


def pose_prior(grid, num_rotations, position=None, covariance=None, heading=None, concentration=None, weights=None,
               sensor_q=None):
  """A mixture prior over position and heading for ``prior_votes`` -> ``PosePrior`` (host, float64, no device work).

  The mixture has M components, 1 <= M <= 8: M is the leading dimension of the arguments given (a single component may
  omit it).  Component m has the weight ``weights[m]`` > 0 (normalised to sum 1; default equal), the position mean
  ``position[m]`` [2] in metres in the MAP corner frame with the symmetric positive-definite ``covariance[m]`` [2, 2]
  in metres^2 (``position`` None: no position term), and the heading mean ``heading[m]`` (the yaw of m_t_q, radians) with
  the von Mises ``concentration[m]`` >= 0 (``heading`` None or concentration 0: no heading term).  At least one of the
  two must be given.  ``sensor_q`` [2] (metres) is the point of the QUERY corner frame the position refers to -- the
  antenna or the camera; default the grid centre c = extent_meters / 2.

  With alpha_k = 2 pi k / R, e = extent - 1.5 and cell = grid.cell_size, the pose of the index (k, a, b)
  (``exhaustive_indices_to_tfm``) puts the sensor at c + ((a, b) - e) cell + Rot(-alpha_k) (sensor_q - c), so component
  m is centred, in plane k, at mu_mk = (g_m - c - Rot(-alpha_k) (sensor_q - c)) / cell + e: one shifted Gaussian per
  rotation (independent of k for the default sensor).  The table holds n = rint(mu) (int32) and f = mu - n in [-0.5,
  0.5] (f32), the precision in cells P = cell^2 Sigma^-1 as (Pxx, Pxy, Pyy) (f32), y_mk = kappa_m (cos(-alpha_k -
  theta_m) - 1) <= 0 (f32) and log w_m (f32).  The unnormalised log-prior of a cell is u = logsumexp_m [log w_m + y_mk
  - (Pxx da^2 + 2 Pxy da db + Pyy db^2) / 2] with (da, db) = (a, b) - mu_mk.

  Raises ValueError for a non-finite input, a covariance that is not symmetric positive definite, M outside 1..8,
  mismatched leading dimensions, weights that are not > 0, a negative concentration, a centre further than 2^23 cells
  from the lattice's origin, and a precision so large that the quadratic form Pxx da^2 + 2 |Pxy da db| + Pyy db^2
  reaches 2^120 at some cell of the lattice (it must stay inside f32 with room for the sums around it)."""
  fn = 'pose_prior'
  R = int(num_rotations)
  if not 1 <= R <= 64:
    raise ValueError(f'{fn}: 1 <= num_rotations <= 64, got {R}')
  if position is None and heading is None:
    raise ValueError(f'{fn}: at least one of position and heading must be given')
  if (position is None) != (covariance is None):
    raise ValueError(f'{fn}: position and covariance go together')
  if heading is None and concentration is not None:
    raise ValueError(f'{fn}: a concentration without a heading')
  rows = {}
  if position is not None:
    rows['position'] = _prior_rows(fn, position, (2,), 'position')
    rows['covariance'] = _prior_rows(fn, covariance, (2, 2), 'covariance')
  if heading is not None:
    rows['heading'] = _prior_rows(fn, heading, (), 'heading')
    rows['concentration'] = _prior_rows(fn, 1.0 if concentration is None else concentration, (), 'concentration')
  if weights is not None:
    rows['weights'] = _prior_rows(fn, weights, (), 'weights')
  sizes = {name: v.shape[0] for name, v in rows.items()}
  M = max(sizes.values())
  if concentration is None and heading is not None:
    rows['concentration'] = np.broadcast_to(rows['concentration'], (sizes['heading'],)).copy()
    sizes['concentration'] = sizes['heading']
  if len(set(sizes.values())) != 1:
    raise ValueError(f'{fn}: mismatched leading dimensions {sizes}')
  if not 1 <= M <= PRIOR_MAX_COMPONENTS:
    raise ValueError(f'{fn}: 1 to {PRIOR_MAX_COMPONENTS} components, got {M}')
  w = rows.get('weights', np.ones(M))
  if not (w > 0).all():
    raise ValueError(f'{fn}: weights must be > 0, got {w.tolist()}')
  w = w / w.sum()
  cell = float(grid.cell_size)
  extent = np.asarray(grid.extent, np.float64)[:2]
  Ho, Wo = (int(2 * v - 1) for v in extent)
  c = extent * cell / 2
  e = extent - 1.5
  s = c if sensor_q is None else _prior_rows(fn, sensor_q, (2,), 'sensor_q')[0]
  alpha = 2 * np.pi * np.arange(R) / R
  cos, sin = np.cos(-alpha), np.sin(-alpha)
  lever = np.stack([cos * (s - c)[0] - sin * (s - c)[1], sin * (s - c)[0] + cos * (s - c)[1]], -1)   # [R, 2]
  mu = np.zeros((M, R, 2))
  P = np.zeros((M, 3))
  if position is not None:
    cov = rows['covariance']
    det = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    if not ((cov[:, 0, 1] == cov[:, 1, 0]).all() and (cov[:, 0, 0] > 0).all() and (det > 0).all()):
      raise ValueError(f'{fn}: covariance must be symmetric positive definite, got {cov.tolist()}')
    mu = (rows['position'][:, None] - c - lever[None]) / cell + e
    P = np.stack([cov[:, 1, 1], -cov[:, 0, 1], cov[:, 0, 0]], -1) / det[:, None] * cell ** 2
    if not (np.isfinite(P).all() and np.abs(mu).max() <= 2.0 ** 23):
      raise ValueError(f'{fn}: a centre beyond 2^23 cells or a precision that is not finite')
    far = np.maximum(np.abs(mu), np.abs(mu - np.array([Ho - 1, Wo - 1]))).max(1) + 0.5   # [M, 2]
    quad = P[:, 0] * far[:, 0] ** 2 + 2 * np.abs(P[:, 1]) * far[:, 0] * far[:, 1] + P[:, 2] * far[:, 1] ** 2
    if not (quad < PRIOR_MAX_QUADRATIC).all():
      raise ValueError(f'{fn}: the precision {P.tolist()} (cells^-2) takes the quadratic form to {quad.max():.3g} on '
                       f'the lattice; the limit is 2^120')
  y = np.zeros((M, R))
  if heading is not None:
    kappa = rows['concentration']
    if not (kappa >= 0).all():
      raise ValueError(f'{fn}: concentration must be >= 0, got {kappa.tolist()}')
    y = kappa[:, None] * (np.cos(-alpha[None] - rows['heading'][:, None]) - 1.0)
  n = np.rint(mu)
  with np.errstate(over='ignore', under='ignore'):
    planes = np.concatenate([mu - n, y[..., None]], -1).astype(np.float32)
    comps = np.concatenate([P, np.log(w)[:, None]], -1).astype(np.float32)
  if not (np.isfinite(planes).all() and np.isfinite(comps).all()):
    raise ValueError(f'{fn}: the table does not fit f32 (concentration {rows.get("concentration")}, precision '
                     f'{P.tolist()})')
  return PosePrior((R, Ho, Wo), w, mu, n.astype(np.int32), np.ascontiguousarray(planes), np.ascontiguousarray(comps))


def prior_votes(votes, prior, grid, num_rotations, temperature=1.0, m_t_q_gt=None, device=None):
  """The measurement update with a ``pose_prior`` (``ops.prior_volume``): p = softmax(temperature * votes + u) over the
  finite cells of ``votes`` [R, 2H-1, 2W-1], u the prior's unnormalised log-density -> dict of device tensors, nothing
  synchronised: ``votes`` (normalised log-probabilities, -inf = impossible: again a vote volume for every other
  operator); float64 scalars ``log_z``, ``log_z_votes`` (of temperature * votes alone), ``log_z_prior`` (of the prior
  over the whole lattice), ``expected_log_prior`` = E_p[u], ``log_evidence`` = log_z - log_z_prior (the frame under the
  normalised prior), ``log_overlap`` = log_evidence - log_z_votes <= 0 (the log overlap of the two normalised
  distributions: the consistency figure a gate thresholds) and ``information_gain`` = KL(p || votes alone) >= 0;
  ``responsibility`` float64 [M]; ``count`` int32 [4] = (finite cells, NaN / +inf cells, cells whose mass underflowed,
  0); ``stats``: the op's raw float64 row.  Without a finite cell log_z and log_evidence are -inf and the other
  figures NaN.  With ``m_t_q_gt`` (a Transform2D, map corner frame; read on the host): ``log_prior_gt`` = u at the cell
  nearest ``exhaustive_tfm_to_index`` of it, from the host table, minus log_z_prior (NaN outside the lattice).
  ``votes`` None returns the prior itself as a normalised belief over the whole lattice, on ``device``."""
  R = int(num_rotations)
  if not isinstance(prior, PosePrior):
    raise ValueError(f'prior_votes: prior must come from pose_prior, got {type(prior).__name__}')
  extent = tuple(int(2 * v - 1) for v in tuple(grid.extent)[:2])
  if prior.shape != (R,) + extent:
    raise ValueError(f'prior_votes: the prior was built for the lattice {prior.shape}, not {(R,) + extent}')
  if votes is not None:
    _check_planes('prior_votes', votes, num_rotations, 'votes')
    votes = votes.contiguous()
  out, resp, stats, count = ops.prior_volume(votes, prior, temperature, device=device)
  res = dict(votes=out, log_z=stats[0], log_z_votes=stats[1], log_z_prior=stats[2], expected_log_prior=stats[4],
             log_evidence=stats[0] - stats[2], log_overlap=(stats[0] - stats[2]) - stats[1],
             information_gain=(stats[4] - stats[0]) + stats[1], responsibility=resp, count=count, stats=stats)
  if m_t_q_gt is not None:
    gt = _host_f64(exhaustive_tfm_to_index(m_t_q_gt, grid, num_rotations)).reshape(3)
    u_gt = float('nan')
    if np.isfinite(gt).all():
      k, a, b = int(np.rint(gt[0])) % R, int(np.rint(gt[1])), int(np.rint(gt[2]))
      if 0 <= a < prior.shape[1] and 0 <= b < prior.shape[2]:
        u_gt = float(prior.log_prior(k, a, b))
    res['log_prior_gt'] = u_gt - stats[2]
  return res
