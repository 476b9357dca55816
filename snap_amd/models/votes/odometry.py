"""The motion between two frames from their votes (``ops.vote_odometry``): candidate increments as integer shifts of
the lattice, their evidence and posterior, and the chain of increments of a whole track."""
import math

import torch

from snap_amd import ops
from snap_amd.models.votes.lattice import _host_transform_f64, _no_motion, _shift_table_f64, _wrap_angle
from snap_amd.utils import geometry


# Limits of ops.vote_odometry's window (vote_odometry.hip).
ODOMETRY_MAX_S = 32


def _increment_shifts(candidates, grid, num_rotations):
  """Host float64 candidates [U] -> (shifts int32 [U, R, 3] (host), Kr, S): ``_shift_table_f64`` rounded with
  floor(x + 0.5), the rotation shift then wrapped into [-R/2, R/2)."""
  R = int(num_rotations)
  dk, da, db = _shift_table_f64(candidates, grid, R)
  k = torch.floor(dk + 0.5)
  k = k - R * torch.floor((k + R / 2) / R)
  rows = torch.stack((k[:, None].expand(-1, R), torch.floor(da + 0.5), torch.floor(db + 0.5)), -1)
  if rows.numel() == 0:
    return rows.to(torch.int32).contiguous(), 0, 0
  if not bool(torch.isfinite(rows).all()) or float(rows.abs().max()) >= 2 ** 30:
    raise ValueError('increment_lattice: a candidate is not a usable number')
  shifts = rows.to(torch.int32).contiguous()
  Kr = int(shifts[..., 0].abs().max())
  S = int(shifts[..., 1:].abs().max())
  if S > ODOMETRY_MAX_S or 2 * Kr + 1 > R:
    raise ValueError(f'increment_lattice: the candidates reach {S} cells and {Kr} rotation bins; the kernel has '
                     f'S <= {ODOMETRY_MAX_S} and 2 Kr + 1 <= R = {R}')
  return shifts, Kr, S


def increment_lattice(grid, num_rotations, range_xy, range_yaw, step_xy=None, step_yaw=None, centre=None):
  """A regular lattice of candidate increments for ``increment_from_votes``: body-frame offsets (yaw, x, y) with
  |x|, |y| <= ``range_xy`` metres in steps of ``step_xy`` (default: one cell) and |yaw| <= ``range_yaw`` radians in
  steps of ``step_yaw`` (default: one rotation bin, 2 pi / R), yaw slowest and y fastest, composed behind ``centre``
  (a Transform2D, e.g. an odometry reading; default: no motion): candidate = centre @ offset -> (candidates
  Transform2D [U] (host, float64: ``cur_t_prev`` of the sequence operators, corner frames), shifts int32 [U, R, 3]
  (host), Kr, S).

  Row (u, r) of ``shifts`` is (dk, da(r), db(r)) of ``motion_taps``' indexing for candidate u (``_shift_table_f64``,
  float64), da and db rounded with floor(x + 0.5), dk rounded the same way and then wrapped into [-R/2, R/2); Kr and
  S are the largest |dk| and |da|, |db|, the window ``ops.vote_odometry`` needs.  So an increment is resolved to ONE
  cell and ONE rotation bin per rotation: two candidates that round to the same rows are indistinguishable, and
  anything finer than a cell comes only from how the per-rotation roundings of (da(r), db(r)) differ across the
  rotations the belief occupies.  A step below one cell or bin therefore buys resolution only for a belief spread over
  several rotations.  Raises ValueError with the numbers when S > 32 or 2 Kr + 1 > R."""
  R = int(num_rotations)
  step_xy = float(grid.cell_size) if step_xy is None else float(step_xy)
  step_yaw = 2 * math.pi / R if step_yaw is None else float(step_yaw)
  if not (step_xy > 0 and step_yaw > 0 and range_xy >= 0 and range_yaw >= 0
          and all(math.isfinite(v) for v in (step_xy, step_yaw, range_xy, range_yaw))):
    raise ValueError(f'increment_lattice: ranges >= 0 and steps > 0, got {range_xy}, {range_yaw}, {step_xy}, {step_yaw}')
  n_xy = int(math.floor(range_xy / step_xy + 1e-9))
  n_yaw = int(math.floor(range_yaw / step_yaw + 1e-9))
  if (2 * n_yaw + 1) * (2 * n_xy + 1) ** 2 > 2 ** 20:
    raise ValueError(f'increment_lattice: {(2 * n_yaw + 1) * (2 * n_xy + 1) ** 2} candidates')
  xy = torch.arange(-n_xy, n_xy + 1, dtype=torch.float64) * step_xy
  yaw = torch.arange(-n_yaw, n_yaw + 1, dtype=torch.float64) * step_yaw
  g = torch.meshgrid(yaw, xy, xy, indexing='ij')
  offset = geometry.Transform2D(g[0].reshape(-1), torch.stack((g[1].reshape(-1), g[2].reshape(-1)), -1))
  if centre is None:
    candidates = offset
  else:
    c = _host_transform_f64(centre)
    if c.angle.numel() != 1:
      raise ValueError(f'increment_lattice: one centre, got a transform of shape {tuple(centre.angle.shape)}')
    n = offset.angle.numel()
    candidates = geometry.Transform2D(c.angle.expand(n), c.t.expand(n, 2)) @ offset
  shifts, Kr, S = _increment_shifts(candidates, grid, R)
  return candidates, shifts, Kr, S


def increment_from_votes(prev, cur, grid, num_rotations, candidates=None, temperature_prev=1.0, temperature_cur=1.0,
                         prior=None, **lattice):
  """The motion between two frames from their votes (``ops.vote_odometry``): ``prev`` [R, 2H-1, 2W-1] is the previous
  frame's pose distribution in log space (its vote volume with ``temperature_prev``, or a filter belief with 1),
  ``cur`` the current frame's votes (``temperature_cur``).  The evidence of a candidate increment ``cur_t_prev``
  (m_t_prev = m_t_cur @ cur_t_prev, corner frames: what ``filter_votes`` and the other sequence operators take) is the
  agreement sum_pose p_cur(pose) p_prev(pose moved by the candidate), each pose moved by the candidate's own integer
  shift at its rotation (``increment_lattice``, which documents the resolution this gives).  ``candidates``: a
  Transform2D [U], or None for ``increment_lattice(grid, num_rotations, **lattice)``.  ``prior``: None (flat), or
  (cur_t_prev, sigma_xy, sigma_yaw): an independent Gaussian log-prior on the candidates' (x, y) in metres and yaw
  (wrapped) about an odometry reading, computed on the host in float64 -- this is how a reading is corrected rather
  than replaced -> dict: ``log_evidence`` f32 [U] (device), ``log_posterior`` float64 [U] (device; normalised over the
  candidates after adding the prior; NaN when no candidate has evidence), ``index`` (int, the MAP candidate; -1 when
  none), ``cur_t_prev`` (the MAP candidate: a host float64 Transform2D of shape (), None when none), ``mean`` float64
  [3] = (yaw, x, y), the yaw a circular mean about the MAP, and ``cov`` float64 [3, 3] in the same order (host),
  ``candidates`` (host float64), ``shifts``, ``log_table`` f32 [2 Kr + 1, R, 2 S + 1, 2 S + 1], ``count`` int32 [6],
  ``stats`` f32 [4] (the op's raw rows).  One host synchronisation (the MAP index is read back)."""
  R = int(num_rotations)
  if prev.dim() != 3 or prev.shape[0] != R or prev.shape != cur.shape:
    raise ValueError(f'increment_from_votes: prev and cur [{R}, Ho, Wo], got {tuple(prev.shape)} and {tuple(cur.shape)}')
  if candidates is None:
    candidates, shifts, Kr, S = increment_lattice(grid, R, **lattice)
  else:
    if lattice:
      raise ValueError(f'increment_from_votes: candidates and lattice arguments {sorted(lattice)} exclude each other')
    candidates = _host_transform_f64(candidates)
    shifts, Kr, S = _increment_shifts(candidates, grid, R)
  U = int(shifts.shape[0])
  if U == 0:
    raise ValueError('increment_from_votes: no candidates')
  dev = prev.device
  shifts_dev = ops.upload_table(shifts.numpy(), dev).view(torch.int32).view(U, R, 3)
  log_table, log_evidence, best, stats, count = ops.vote_odometry(
      prev.contiguous(), cur.contiguous(), Kr, S, shifts_dev, temperature_prev, temperature_cur)
  score = log_evidence.to(torch.float64)
  if prior is not None:
    centre, sigma_xy, sigma_yaw = prior
    c = _host_transform_f64(centre)
    if c.angle.numel() != 1 or not (sigma_xy > 0 and sigma_yaw > 0):
      raise ValueError(f'increment_from_votes: prior (cur_t_prev, sigma_xy > 0, sigma_yaw > 0), got sigmas {sigma_xy}, '
                       f'{sigma_yaw}')
    dxy = candidates.t - c.t
    dyaw = _wrap_angle(candidates.angle - c.angle)
    log_prior = -0.5 * ((dxy ** 2).sum(-1) / float(sigma_xy) ** 2 + dyaw ** 2 / float(sigma_yaw) ** 2)
    score = score + log_prior.to(dev)
  log_posterior = score - torch.logsumexp(score, 0)
  host = log_posterior.cpu()                                 # the one synchronisation
  out = dict(log_evidence=log_evidence, log_posterior=log_posterior, candidates=candidates, shifts=shifts_dev,
             log_table=log_table, count=count, stats=stats)
  if not bool(torch.isfinite(host).any()):
    out.update(index=-1, cur_t_prev=None, mean=torch.full((3,), float('nan'), dtype=torch.float64),
               cov=torch.full((3, 3), float('nan'), dtype=torch.float64))
    return out
  index = int(best[0]) if prior is None else int(torch.nonzero(host == host.max())[0, 0])
  w = torch.exp(host)
  top = candidates[index]
  dev3 = torch.stack((_wrap_angle(candidates.angle - top.angle), candidates.t[:, 0] - top.t[0],
                      candidates.t[:, 1] - top.t[1]), -1)
  mean_dev = (w[:, None] * dev3).sum(0)
  centred = dev3 - mean_dev
  out.update(index=index, cur_t_prev=top,
             mean=torch.stack((top.angle, top.t[0], top.t[1])) + mean_dev,
             cov=(w[:, None, None] * centred[:, :, None] * centred[:, None, :]).sum(0))
  return out


def estimate_increments(volumes, grid, num_rotations, temperature=1.0, details=False, **kw):
  """The increments of a track from its vote volumes alone: ``increment_from_votes`` on every consecutive pair
  (volumes[t - 1], volumes[t]), both with ``temperature``; ``kw`` goes to it (``candidates`` or the lattice's ranges;
  a ``prior`` here is one per call: a list of N entries, entry 0 ignored, or None) -> (increments, q0_t_q):
  ``increments`` is the list [None, cur_t_prev_1, ...] that ``viterbi_track``, ``smooth_track``, ``sample_tracks`` and
  ``fit_motion_noise`` take (entry 0 is None: a track starts from a uniform prior), ``q0_t_q`` the Transform2D [N]
  (host, float64) chain q0_t_qn = q0_t_q(n-1) @ cur_t_prev_n^-1 that ``fuse_votes`` / ``localize_sequence`` take.
  With ``details`` a third entry holds ``increment_from_votes``' dicts (None for frame 0).  Raises ValueError where a
  pair has no candidate with evidence."""
  volumes = list(volumes)
  if not volumes:
    raise ValueError('estimate_increments: no volumes')
  priors = kw.pop('prior', None)
  increments, steps = [None], [None]
  chain = [_no_motion()]
  for t in range(1, len(volumes)):
    step = increment_from_votes(volumes[t - 1], volumes[t], grid, num_rotations, temperature_prev=temperature,
                                temperature_cur=temperature, prior=None if priors is None else priors[t], **kw)
    if step['cur_t_prev'] is None:
      raise ValueError(f'estimate_increments: frames {t - 1} and {t} share no candidate with evidence')
    increments.append(step['cur_t_prev'])
    steps.append(step)
    chain.append(chain[-1] @ step['cur_t_prev'].inv)
  q0_t_q = geometry.Transform2D(torch.stack([c.angle for c in chain]), torch.stack([c.t for c in chain]))
  return (increments, q0_t_q, steps) if details else (increments, q0_t_q)
