"""One vote volume -> what it says about the pose: its peaks, the posterior and its marginals, credible regions, the
Gaussian mixture around the peaks and the expected recall (each one ``snap_amd.ops`` kernel), and the host tables an
evaluation loop builds from them over many frames (coverage, NEES, reliability)."""
import fractions
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.models.pose_exhaustive_voting import exhaustive_index_to_tfm, exhaustive_indices_to_tfm
from snap_amd.models.votes.lattice import _check_planes, _gt_index
from snap_amd.utils import geometry


def poses_from_votes(votes, grid, num_rotations, num_peaks=16, radius_r=1, radius_xy=1):
  """The ``num_peaks`` best distinct poses of a vote volume [R, 2H-1, 2W-1] (``ops.vote_peaks``: non-maximum
  suppression over ``radius_r`` rotations, circular, and ``radius_xy`` cells) -> dict(map_t_query Transform2D [K],
  index int32 [K, 3], score f32 [K], count int32 [2] = (peaks found; NaN votes)).  Best first; rows past
  ``count[0]`` hold index -1, score -inf and a NaN transform."""
  _check_planes('poses_from_votes', votes, num_rotations)
  index, score, count = ops.vote_peaks(votes.contiguous(), num_peaks, radius_r, radius_xy)
  return dict(map_t_query=exhaustive_indices_to_tfm(index, grid, num_rotations), index=index, score=score,
              count=count)


def posterior_from_votes(votes, grid, num_rotations, temperature=1.0, m_t_q_gt=None):
  """The pose distribution p = softmax(temperature * votes) of a vote volume [R, 2H-1, 2W-1] over its finite cells
  (``ops.vote_posterior``; ``temperature`` is the multiplier of the log-scores: exp(learned temperature), or 1) ->
  dict of device tensors, nothing synchronised:

  ``log_prob_xy`` [2H-1, 2W-1] / ``log_prob_r`` [R]: the xy heat map and the yaw histogram, in log space;
  ``log_z``, ``entropy``; ``map_t_query_expected``: ``exhaustive_index_to_tfm`` of the continuous index (circular
  mean rotation index, E[a], E[b]) -- the same +0.5 cell offset and corner-frame conjugation; ``cov_xy`` [2, 2]: the
  covariance of the cell offset in metres^2, rows / columns in the map's (x, y) = index (a, b) order;
  ``yaw_resultant``: the resultant length of the rotation distribution (1 = one rotation, 0 = no preferred one);
  ``count`` int32 [3] = (finite cells, NaN / +inf cells, ground-truth sample valid); ``stats``: the op's raw row.
  With ``m_t_q_gt`` (a Transform2D, map corner frame): ``nll`` = -log p interpolated at ``exhaustive_tfm_to_index``
  of it (computed and read on the device) and ``nll_valid`` (bool; ``nll`` is NaN where it is False: the pose lies
  outside the volume or touches a masked cell)."""
  _check_planes('posterior_from_votes', votes, num_rotations)
  gt = _gt_index(m_t_q_gt, grid, num_rotations, votes.device)
  log_prob_xy, log_prob_r, stats, count = ops.vote_posterior(votes.contiguous(), temperature, gt)
  cell2 = float(grid.cell_size) ** 2
  out = dict(
      log_prob_xy=log_prob_xy, log_prob_r=log_prob_r, log_z=stats[0], entropy=stats[11],
      map_t_query_expected=exhaustive_index_to_tfm(torch.stack((stats[9], stats[2], stats[3])), grid, num_rotations),
      cov_xy=torch.stack((stats[4:6], stats[5:7])) * cell2, yaw_resultant=stats[10], count=count, stats=stats)
  if m_t_q_gt is not None:
    out['nll'] = -stats[12]
    out['nll_valid'] = count[2] != 0
  return out


def _with_posterior(out, votes, grid, num_rotations, posterior):
  """The ``posterior`` argument of the localizing entry points: None or False adds nothing; True, or a dict of keyword
  arguments of ``posterior_from_votes``, adds its result for ``votes`` as ``out['posterior']``."""
  if posterior is not None and posterior is not False:
    kw = {} if posterior is True else dict(posterior)
    out['posterior'] = posterior_from_votes(votes, grid, num_rotations, **kw)


def credible_from_votes(votes, grid, num_rotations, levels=(0.5, 0.9, 0.99), temperature=1.0, m_t_q_gt=None,
                        cell_levels=False):
  """The highest-density credible regions of p = softmax(temperature * votes) over the finite cells of a vote volume
  [R, 2H-1, 2W-1] (``ops.vote_credible``): for every level q of ``levels`` the smallest set of whole tie classes of
  cells that holds at least q of the probability -> dict of device tensors, nothing synchronised:

  ``threshold`` / ``mass`` [L], ``table`` int32 [L, 8], ``level_xy`` uint8 [2H-1, 2W-1], ``level_r`` uint8 [R],
  ``level_cell`` (None unless ``cell_levels``), ``gt_stats``, ``count``: the op's outputs (region l of a level map is
  ``level <= l``); ``area_m2`` [L] = pixels * cell^2, the footprint of the region on the map; ``yaw_span_deg`` [L] =
  rotations * 360 / R; ``volume`` [L] = cells * cell^2 * 2 pi / R (m^2 rad).
  With ``m_t_q_gt`` (a Transform2D, map corner frame; rounded to the nearest cell of ``exhaustive_tfm_to_index`` on the
  device): ``gt_credibility`` = the mass ranked strictly above the true pose's cell (uniform on [0, 1] for a calibrated
  posterior; NaN where invalid), ``gt_level`` (the smallest l whose region holds it, L = none, -1 = invalid),
  ``gt_valid`` (bool: inside the volume, on a contributing cell) and ``covered`` [L] bool."""
  _check_planes('credible_from_votes', votes, num_rotations)
  gt = _gt_index(m_t_q_gt, grid, num_rotations, votes.device)
  levels = tuple(float(q) for q in levels)
  threshold, mass, table, level_xy, level_r, level_cell, gt_stats, count = ops.vote_credible(
      votes.contiguous(), levels, temperature, gt, cell_levels)
  cell2 = float(grid.cell_size) ** 2
  out = dict(
      threshold=threshold, mass=mass, table=table, level_xy=level_xy, level_r=level_r, level_cell=level_cell,
      gt_stats=gt_stats, count=count, area_m2=table[:, 1].to(torch.float32) * cell2,
      yaw_span_deg=table[:, 2].to(torch.float32) * (360.0 / num_rotations),
      volume=table[:, 0].to(torch.float32) * (cell2 * 2 * math.pi / num_rotations))
  if m_t_q_gt is not None:
    out['gt_credibility'] = gt_stats[1]
    out['gt_level'] = count[3]
    out['gt_valid'] = count[2] != 0
    out['covered'] = (count[3] >= 0) & (count[3] <= torch.arange(len(levels), device=votes.device))
  return out


def coverage_table(gt_credibility, levels, valid=None):
  """Host helper of an evaluation loop: the calibration of credible regions over many frames.  ``gt_credibility``: the
  frames' ``credible_from_votes(...)['gt_credibility']`` (any array-like; NaN = invalid), ``valid``: an optional bool
  mask on top -> dict(levels, coverage [L] = the fraction of valid frames with gt_credibility < q (the true pose lay
  inside the q-region), count = the valid frames, mean_abs_error = mean |coverage - q|).  A calibrated posterior has
  coverage = q up to the binomial noise sqrt(q (1 - q) / count)."""
  c = np.asarray(torch.as_tensor(gt_credibility).detach().cpu(), dtype=np.float64).reshape(-1)
  ok = np.isfinite(c)
  if valid is not None:
    ok &= np.asarray(torch.as_tensor(valid).detach().cpu()).reshape(-1).astype(bool)
  q = np.asarray(levels, dtype=np.float64).reshape(-1)
  n = int(ok.sum())
  cov = np.array([float((c[ok] < v).mean()) if n else float('nan') for v in q])
  return dict(levels=q, coverage=cov, count=n, mean_abs_error=float(np.abs(cov - q).mean()) if n else float('nan'))


def _mode_pose_and_jacobian(index_mean, grid, num_rotations):
  """The corner-frame pose at continuous indices [K, 3] = (k, a, b) and its derivative, in float64 on the indices'
  device -> (angle [K], t [K, 2], J [K, 3, 3] = d (angle, tx, ty) / d (k, a, b)).  The pose is
  ``exhaustive_index_to_tfm``'s c @ (-2 pi k / R, ((a, b) - extent + 1.5) cell) @ c^-1 written out with c = (0, centre):
  angle = -2 pi k / R, t = centre + xy_cell - Rot(angle) centre, so the translation depends on k through the rotation
  of the centre: d t / d angle = (sin cx + cos cy, -cos cx + sin cy)."""
  idx = index_mean.to(torch.float64)
  R = int(num_rotations)
  H, W = (float(v) for v in grid.extent)
  cell = float(grid.cell_size)
  cx, cy = (float(v) / 2 for v in grid.extent_meters)
  dphi = -2 * math.pi / R
  angle = idx[:, 0] * dphi
  cos, sin = torch.cos(angle), torch.sin(angle)
  tx = cx + (idx[:, 1] - H + 1.5) * cell - (cos * cx - sin * cy)
  ty = cy + (idx[:, 2] - W + 1.5) * cell - (sin * cx + cos * cy)
  J = torch.zeros((idx.shape[0], 3, 3), dtype=torch.float64, device=idx.device)
  J[:, 0, 0] = dphi
  J[:, 1, 0] = (sin * cx + cos * cy) * dphi
  J[:, 2, 0] = (-cos * cx + sin * cy) * dphi
  J[:, 1, 1] = cell
  J[:, 2, 2] = cell
  return angle, torch.stack((tx, ty), -1), J


def modes_from_votes(votes, grid, num_rotations, peaks=None, num_peaks=16, radius_r=1, radius_xy=1, win_r=None,
                     win_xy=None, temperature=1.0, log_z=None, m_t_q_gt=None):
  """The Gaussian mixture of a vote volume [R, 2H-1, 2W-1]: one component per peak (``ops.vote_modes``) over
  p = softmax(temperature * votes).  ``peaks``: an int32 [K, 3] device table of (r, a, b) rows, or None:
  ``poses_from_votes(num_peaks, radius_r, radius_xy)`` finds them.  The window (``win_r`` rotations, ``win_xy`` cells
  around a peak) defaults to the non-maximum-suppression radii; ``log_z``: the volume's log partition sum (a tensor or
  a number), or None: ``ops.vote_posterior`` computes it -> dict of device tensors, nothing synchronised:

  ``weight`` [K] = exp(log_mass - log_z), the probability a mode owns; ``unassigned`` = 1 - sum weight, the
  probability of the cells outside every window; ``index_mean`` [K, 3], the continuous (k, a, b) index;
  ``map_t_query`` Transform2D [K], the pose at it (``exhaustive_index_to_tfm``'s +0.5 cell offset and corner-frame
  conjugation), NaN for empty modes; ``cov_index`` [K, 3, 3] in index units; ``cov`` [K, 3, 3] in (angle rad, x m, y m)
  of the corner-frame transform, the first-order propagation J Sigma J^T at the mode mean in float64 rounded once (J
  includes the angle-dependence of the corner-frame translation); ``count`` int32 [K, 2] = (owned finite cells, owned
  NaN / +inf cells); ``stats``, the op's raw rows; ``index``, the peak table used.  With ``m_t_q_gt`` (a Transform2D,
  map corner frame): ``nees`` [K], the ground truth's normalised estimation error squared under each mode in index
  units with the lattice's I/12 added to the covariance (chi^2 with 3 degrees of freedom for a consistent mode:
  ``nees_table``)."""
  _check_planes('modes_from_votes', votes, num_rotations)
  votes = votes.contiguous()
  if peaks is None:
    peaks = poses_from_votes(votes, grid, num_rotations, num_peaks, radius_r, radius_xy)['index']
  win_r = radius_r if win_r is None else win_r
  win_xy = radius_xy if win_xy is None else win_xy
  gt = _gt_index(m_t_q_gt, grid, num_rotations, votes.device)
  if log_z is None:
    log_z = ops.vote_posterior(votes, temperature)[2][0]
  stats, count = ops.vote_modes(votes, peaks.contiguous(), win_r, win_xy, temperature, gt)
  log_z = log_z.to(device=votes.device, dtype=torch.float64) if isinstance(log_z, torch.Tensor) else float(log_z)
  weight = torch.exp(stats[:, 0].to(torch.float64) - log_z)
  index_mean = stats[:, 2:5]
  angle, t, J = _mode_pose_and_jacobian(index_mean, grid, num_rotations)
  s = stats.to(torch.float64)
  cov_index = torch.stack((s[:, 5], s[:, 6], s[:, 7], s[:, 6], s[:, 8], s[:, 9], s[:, 7], s[:, 9], s[:, 10]),
                          -1).reshape(-1, 3, 3)
  cov = J @ cov_index @ J.transpose(1, 2)
  out = dict(
      weight=weight.to(torch.float32), unassigned=(1.0 - weight.sum()).to(torch.float32), index_mean=index_mean,
      map_t_query=geometry.Transform2D(angle.to(torch.float32), t.to(torch.float32)),
      cov_index=cov_index.to(torch.float32), cov=cov.to(torch.float32), count=count, stats=stats, index=peaks)
  if m_t_q_gt is not None:
    out['nees'] = stats[:, 11]
  return out


def _modes_of_peaks(out, votes, grid, num_rotations, modes, posterior, peaks):
  """``modes_from_votes`` for an entry point that has run ``poses_from_votes(**peaks)`` into ``out`` and, where
  ``posterior`` asks for it, ``posterior_from_votes`` into ``out['posterior']``."""
  kw = {} if modes is True else dict(modes)
  kw.setdefault('radius_r', peaks.get('radius_r', 1))
  kw.setdefault('radius_xy', peaks.get('radius_xy', 1))
  if 'posterior' in out and 'log_z' not in kw:
    post_kw = {} if posterior is True else posterior
    if float(post_kw.get('temperature', 1.0)) == float(kw.get('temperature', 1.0)):
      kw['log_z'] = out['posterior']['log_z']
  return modes_from_votes(votes, grid, num_rotations, peaks=out['index'], **kw)


def _chi2_3_cdf(x):
  """The chi-square distribution function with 3 degrees of freedom: erf(sqrt(x / 2)) - sqrt(2 x / pi) exp(-x / 2)."""
  return math.erf(math.sqrt(x / 2)) - math.sqrt(2 * x / math.pi) * math.exp(-x / 2)


def chi2_3_quantile(q):
  """The q-quantile (0 <= q < 1) of the chi-square distribution with 3 degrees of freedom, by bisection on the closed
  form of its distribution function in float64."""
  q = float(q)
  if not 0.0 <= q < 1.0:
    raise ValueError(f'chi2_3_quantile: level {q} outside [0, 1)')
  lo, hi = 0.0, 1.0
  while _chi2_3_cdf(hi) < q:
    hi *= 2
  for _ in range(200):
    mid = 0.5 * (lo + hi)
    if mid == lo or mid == hi:
      break
    if _chi2_3_cdf(mid) < q:
      lo = mid
    else:
      hi = mid
  return 0.5 * (lo + hi)


def nees_table(nees, levels=(0.5, 0.9, 0.99), valid=None):
  """Host helper of an evaluation loop, the Gaussian counterpart of ``coverage_table``: the consistency of the modes'
  covariances over many frames.  ``nees``: the frames' ``modes_from_votes(...)['nees']`` of the mode that is judged
  (any array-like; NaN = invalid), ``valid``: an optional bool mask on top -> dict(levels, quantile [L] = the chi^2_3
  quantiles of the levels, coverage [L] = the fraction of valid samples with nees below the quantile, count = the
  valid samples, mean_abs_error = mean |coverage - q|).  A consistent covariance has coverage = q up to the binomial
  noise sqrt(q (1 - q) / count); a coverage below q means covariances that are too small."""
  c = np.asarray(torch.as_tensor(nees).detach().cpu(), dtype=np.float64).reshape(-1)
  ok = np.isfinite(c)
  if valid is not None:
    ok &= np.asarray(torch.as_tensor(valid).detach().cpu()).reshape(-1).astype(bool)
  q = np.asarray(levels, dtype=np.float64).reshape(-1)
  quant = np.array([chi2_3_quantile(v) for v in q])
  n = int(ok.sum())
  cov = np.array([float((c[ok] < v).mean()) if n else float('nan') for v in quant])
  return dict(levels=q, quantile=quant, coverage=cov, count=n,
              mean_abs_error=float(np.abs(cov - q).mean()) if n else float('nan'))


RECALL_THRESHOLDS = ((0.5, 1), (1, 2), (2, 4))             # (metres, degrees): the reference's joint recall pairs


def recall_thresholds(thresholds, grid, num_rotations):
  """(metres, degrees) pairs -> (rho2, half_r), int32 arrays [L] of ``ops.vote_recall``: the squared xy radius in cells
  and the rotation half-width in bins of the lattice poses STRICTLY within the thresholds of a lattice pose, as the
  reference's recall tests dt < t and dr < t: d^2 < (t / cell)^2 for an integer d^2 is d^2 <= ceil((t / cell)^2) - 1,
  and |dr| 360 / R < t_deg is |dr| <= ceil(t_deg R / 360) - 1.  Exact rational arithmetic on the numbers' shortest
  decimal forms (0.25 is 1/4, 0.2 is 1/5), so a threshold that is a whole number of cells is excluded as it should
  be.  ValueError for a pair outside the op's limits (1 to 8 pairs, 0 <= rho2 <= 1024, 0 <= half_r <= 4,
  2 half_r + 1 <= R)."""
  frac = lambda v: fractions.Fraction(repr(float(v)))
  R = int(num_rotations)
  pairs = [tuple(p) for p in thresholds]
  if not 1 <= len(pairs) <= 8 or any(len(p) != 2 for p in pairs):
    raise ValueError(f'recall_thresholds: 1 to 8 (metres, degrees) pairs, got {thresholds}')
  cell = frac(grid.cell_size)
  rho2, half_r = [], []
  for t_m, t_deg in pairs:
    if not (math.isfinite(t_m) and math.isfinite(t_deg) and t_m > 0 and t_deg > 0):
      raise ValueError(f'recall_thresholds: thresholds must be finite numbers > 0, got ({t_m}, {t_deg})')
    q = math.ceil((frac(t_m) / cell) ** 2) - 1
    h = math.ceil(frac(t_deg) * R / 360) - 1
    if q > 1024 or h > 4 or 2 * h + 1 > R:
      raise ValueError(f'recall_thresholds: ({t_m} m, {t_deg} deg) is rho2={q}, half_r={h} on a {grid.cell_size} m, '
                       f'{R}-rotation lattice: outside rho2 <= 1024, half_r <= 4, 2 half_r + 1 <= R')
    rho2.append(q)
    half_r.append(h)
  return np.asarray(rho2, dtype=np.int32), np.asarray(half_r, dtype=np.int32)


def recall_from_votes(votes, grid, num_rotations, thresholds=RECALL_THRESHOLDS, temperature=1.0, peaks=None,
                      m_t_q_gt=None, maps=False):
  """The expected recall under p = softmax(temperature * votes) of a vote volume [R, 2H-1, 2W-1]
  (``ops.vote_recall``): for every (metres, degrees) pair of ``thresholds`` (``recall_thresholds``) the probability
  that the pose lies strictly within the pair of a lattice pose -> dict of device tensors, nothing synchronised:

  ``best_index`` int32 [L, 3] and ``map_t_query`` Transform2D [L]: per pair the lattice pose whose threshold ball
  carries the most probability, i.e. the estimate that maximises the expected recall at that pair
  (``exhaustive_indices_to_tfm``; NaN without a finite vote); ``best_recall`` [L]: that probability;
  ``thresholds_cells`` int32 [L, 2] = (rho2, half_r) (host); ``log_z``; ``count`` int32 [4] = (finite cells, NaN / +inf
  cells, ground truth valid, 0).  With ``peaks`` (an int32 [K, 3] device table, ``poses_from_votes(...)['index']``):
  ``peak_recall`` [K, L], the probability that each candidate is within the thresholds (0 for a -1 row).  With
  ``m_t_q_gt`` (a Transform2D, map corner frame; rounded to the nearest cell of ``exhaustive_tfm_to_index`` on the
  device): ``gt_recall`` [L], the probability within the thresholds of the true pose, a smooth counterpart of the
  hit / miss metric (NaN where the truth lies outside the volume).  With ``maps``: ``maps`` [L, R, 2H-1, 2W-1], the log
  of that probability for every lattice pose."""
  _check_planes('recall_from_votes', votes, num_rotations)
  rho2, half_r = recall_thresholds(thresholds, grid, num_rotations)
  gt = _gt_index(m_t_q_gt, grid, num_rotations, votes.device)
  best_index, best_lm, centre_lm, gt_lm, stats, count, lm_maps = ops.vote_recall(
      votes.contiguous(), rho2.tolist(), half_r.tolist(), None if peaks is None else peaks.contiguous(), temperature,
      gt, maps)
  out = dict(best_index=best_index, map_t_query=exhaustive_indices_to_tfm(best_index, grid, num_rotations),
             best_recall=torch.exp(best_lm), thresholds_cells=np.stack([rho2, half_r], -1), log_z=stats[0],
             count=count)
  if peaks is not None:
    out['peak_recall'] = torch.exp(centre_lm)
  if m_t_q_gt is not None:
    out['gt_recall'] = torch.exp(gt_lm)
  if maps:
    out['maps'] = lm_maps
  return out


def recall_table(pred_recall, hit, bins=10, valid=None):
  """Host helper of an evaluation loop, the reliability table that goes with ``recall_from_votes(...)['peak_recall']``:
  ``pred_recall``: the predicted probabilities that the judged poses are within a threshold, ``hit``: whether they
  were (any array-likes of one shape; a NaN prediction = invalid), ``valid``: an optional bool mask on top ->
  dict(edges [bins + 1], count [bins], mean_pred [bins], hit_rate [bins] (NaN for an empty bin), total = the valid
  samples, ece = sum count / total |mean_pred - hit_rate|, NaN without samples).  ``bins`` equal bins on [0, 1], a
  prediction of exactly 1 in the last; float64.  A calibrated predictor has hit_rate = mean_pred up to the binomial
  noise sqrt(p (1 - p) / count)."""
  p = np.asarray(torch.as_tensor(pred_recall).detach().cpu(), dtype=np.float64).reshape(-1)
  h = np.asarray(torch.as_tensor(hit).detach().cpu()).reshape(-1).astype(np.float64)
  bins = int(bins)
  if bins < 1 or p.shape != h.shape:
    raise ValueError(f'recall_table: bins >= 1 and one hit per prediction, got bins={bins}, {p.size} and {h.size}')
  ok = np.isfinite(p)
  if valid is not None:
    ok &= np.asarray(torch.as_tensor(valid).detach().cpu()).reshape(-1).astype(bool)
  p, h = p[ok], h[ok]
  which = np.clip(np.floor(p * bins).astype(np.int64), 0, bins - 1)
  count = np.bincount(which, minlength=bins)
  with np.errstate(invalid='ignore'):
    mean_pred = np.bincount(which, weights=p, minlength=bins) / count
    hit_rate = np.bincount(which, weights=h, minlength=bins) / count
  n = int(count.sum())
  full = count > 0
  ece = float((count[full] * np.abs(mean_pred[full] - hit_rate[full])).sum() / n) if n else float('nan')
  return dict(edges=np.linspace(0.0, 1.0, bins + 1), count=count, mean_pred=mean_pred, hit_rate=hit_rate, total=n,
              ece=ece)
