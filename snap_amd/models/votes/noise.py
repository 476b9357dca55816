"""EM (Baum-Welch) fit of the filter's motion noise to a track: the expected log-likelihood of a candidate noise under
the tap posteriors of ``track_statistics``, the grid-search M-step, and the loop around filter, smoother and both."""
import math

import numpy as np
import torch

from snap_amd.models.votes.lattice import _host_f64, _no_motion
from snap_amd.models.votes.motion import FILTER_MAX_TAPS_K, FILTER_MAX_TAPS_XY, _motion_axes
from snap_amd.models.votes.sequence import filter_votes, smooth_track, track_statistics


# ``fit_motion_noise``: the default multiplicative candidate grid of the M-step, the range ``uniform_mix`` is kept in,
# and the smallest standard deviation (index units) a candidate is clipped to.
NOISE_CANDIDATES = (0.5, 0.7, 0.85, 1.0, 1.2, 1.5, 2.0)
NOISE_UNIFORM_MIX_RANGE = (1e-6, 0.5)
NOISE_MIN_SIGMA_INDEX = 1e-3


def _expected_log_taps(hist, first, taps, taps_first):
  """sum hist * log(taps) with both tables [M, T] aligned by absolute offset (entry t of row m of ``hist`` is the
  offset first[m] + t); 0 log 0 = 0; -inf where ``hist`` has mass on an offset the candidate gives no tap."""
  total = 0.0
  for m in range(hist.shape[0]):
    for t in np.nonzero(hist[m] > 0)[0]:
      j = int(first[m]) + int(t) - int(taps_first[m])
      w = taps[m, j] if 0 <= j < taps.shape[1] else 0.0
      if not w > 0:
        return -math.inf
      total += hist[m, t] * math.log(w)
  return total


def motion_noise_objective(stats_list, increments, grid, num_rotations, sigma_xy, sigma_yaw, truncate=3.0,
                           support='candidate'):
  """The expected complete-data log-likelihood of the stay branch for a candidate noise, float64 on the host:
  sum over the steps, axes, rows and taps of hist * log w, with ``hist`` the tap posteriors of ``track_statistics``
  (``stats_list[t]`` goes with ``increments[t + 1]``) and w the taps ``motion_taps`` builds for the candidate
  ``sigma_xy`` / ``sigma_yaw`` before their f32 rounding, matched to the histograms by absolute offset.  0 log 0 = 0;
  -inf when the candidate gives a zero tap where a histogram has mass.  The sum separates: ``sigma_yaw`` only enters
  through ``hist_k``, ``sigma_xy`` through ``hist_a`` and ``hist_b``.

  ``support``: 'candidate' = the candidate's own tables, cut at ``truncate`` standard deviations; every histogram has
  some mass on its outermost taps, so any candidate narrow enough to lose a tap is at -inf.  'tables' = the
  candidate's Gaussian cut at the reach rho = (T - 2) / 2 of the tables the histograms were taken with, per axis and
  step (``truncate`` is then not used): the candidates of one E-step are compared on one support, and a narrower one
  is finite as long as its outermost taps stay above the kernel's smallest tap, 2^-20."""
  stats_list, increments = list(stats_list), list(increments)
  if len(stats_list) + 1 != len(increments):
    raise ValueError(f'motion_noise_objective: {len(stats_list)} steps need {len(stats_list) + 1} increments, got '
                     f'{len(increments)}')
  if support not in ('candidate', 'tables'):
    raise ValueError(f"motion_noise_objective: support 'candidate' or 'tables', got {support!r}")
  R = int(num_rotations)
  index_sigma = (float(sigma_yaw) * R / (2 * math.pi), float(sigma_xy) / float(grid.cell_size),
                 float(sigma_xy) / float(grid.cell_size))
  total = 0.0
  for st, inc in zip(stats_list, increments[1:]):
    used = st['taps']
    cut = truncate
    if support == 'tables':                                 # ceil(cut * sigma) = rho, half a unit away from both sides
      reach = [(int(used[i].shape[-1]) - 2) // 2 for i in (0, 2, 3)]
      cut = tuple((rho - 0.5) / s if rho > 0 and s > 0 else 0.0 for rho, s in zip(reach, index_sigma))
    axes = _motion_axes(inc if inc is not None else _no_motion(), grid, R, sigma_xy, sigma_yaw, cut)
    off = _host_f64(used[4]).astype(np.int64)
    for hist, first, (w, l) in ((_host_f64(st['hist_k'])[None], np.array([int(used[1])]), axes[0]),
                                (_host_f64(st['hist_a']), off[:, 0], axes[1]),
                                (_host_f64(st['hist_b']), off[:, 1], axes[2])):
      total += _expected_log_taps(hist, first, w, l)
      if total == -math.inf:
        return total
  return total


def _noise_candidates(value, factors, lo, hi):
  """The candidate grid of one parameter: value * factors clipped to [lo, hi], the current value always among them
  -> (sorted list without repeats)."""
  c = {min(max(float(value) * float(f), lo), hi) for f in factors}
  c.add(float(value))
  return sorted(c)


def noise_m_step(stats_list, increments, grid, num_rotations, sigma_xy, sigma_yaw, truncate=3.0,
                 candidates=NOISE_CANDIDATES):
  """The M-step of ``fit_motion_noise`` on the tap posteriors of one E-step: a one-dimensional search per parameter
  over value * ``candidates`` (the current value always included; clipped so that ``motion_taps`` never raises: at
  least ``NOISE_MIN_SIGMA_INDEX`` index units, at most what the kernel's tables hold at ``truncate``), the objective
  ``motion_noise_objective(support='tables')`` (it separates over the two parameters; on the candidates' own support
  every narrower candidate that loses a tap would be at -inf and a standard deviation could never come down past a
  truncation step), the lowest candidate among equals; ``uniform_mix``
  becomes the mean jump share clamped to ``NOISE_UNIFORM_MIX_RANGE`` -> dict: ``sigma_xy``, ``sigma_yaw``,
  ``uniform_mix`` (the new values), ``jump`` (the mean jump share), ``candidates`` and ``objective`` (dicts with the
  lists for 'sigma_xy' and 'sigma_yaw') and ``current`` (the objective at the current values per parameter)."""
  R = int(num_rotations)
  cell, bin_k = float(grid.cell_size), 2 * math.pi / R
  # the largest sigma (index units) whose ceil(truncate * sigma) still fits the table, a hair inside
  reach = lambda max_taps: ((max_taps - 2) // 2) / truncate * (1 - 1e-12) if truncate > 0 else 1e6
  grids_ = dict(sigma_xy=_noise_candidates(sigma_xy, candidates, NOISE_MIN_SIGMA_INDEX * cell,
                                           max(reach(FILTER_MAX_TAPS_XY) * cell, float(sigma_xy))),
                sigma_yaw=_noise_candidates(sigma_yaw, candidates, NOISE_MIN_SIGMA_INDEX * bin_k,
                                            max(reach(FILTER_MAX_TAPS_K) * bin_k, float(sigma_yaw))))
  out = dict(candidates=grids_, objective={}, current={})
  for name in ('sigma_xy', 'sigma_yaw'):
    value = lambda c: motion_noise_objective(stats_list, increments, grid, R, c if name == 'sigma_xy' else sigma_xy,
                                             c if name == 'sigma_yaw' else sigma_yaw, truncate, support='tables')
    obj = [value(c) for c in grids_[name]]
    out['objective'][name] = obj
    out['current'][name] = obj[grids_[name].index(float(sigma_xy if name == 'sigma_xy' else sigma_yaw))]
    out[name] = grids_[name][int(np.argmax(obj))]           # (the first, i.e. lowest, among equals)
  jump = float(np.mean([float(_host_f64(st['jump'])) for st in stats_list])) if stats_list else 0.0
  out['jump'] = jump
  out['uniform_mix'] = min(max(jump, NOISE_UNIFORM_MIX_RANGE[0]), NOISE_UNIFORM_MIX_RANGE[1])
  return out


def fit_motion_noise(volumes, increments, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                     temperature=1.0, truncate=3.0, iterations=5, candidates=NOISE_CANDIDATES):
  """EM (Baum-Welch) fit of the filter's motion noise to one track: ``volumes`` the N vote volumes, ``increments``
  the N odometry increments (entry 0 ignored; None = no motion), ``sigma_xy`` / ``sigma_yaw`` / ``uniform_mix`` the
  starting values.  Each iteration runs the filter forward (``filter_votes``), ``smooth_track`` and
  ``track_statistics`` with the current values (the E-step) and then ``noise_m_step`` -> (dict ``sigma_xy``,
  ``sigma_yaw``, ``uniform_mix``: the fitted values; list with one record per iteration: the values the iteration ran
  with, ``log_evidence`` (the track's total under them, a float), ``jump`` (the mean jump share) and ``m_step``
  (``noise_m_step``'s dict)).  The log-evidence of the LAST M-step's values is not evaluated: run the filter once more
  to see it.

  This is a generalised EM: the M-step treats the filter's renormalisation of the mass that leaves the volume (the
  factor sum p / S of its transition kernel, which depends on the noise) as a constant, and searches a grid rather
  than solving for the maximum, so an iteration need not increase the log-evidence when much mass leaves the volume;
  the per-iteration record shows whether it did.  One host synchronisation per step and iteration."""
  volumes, increments = list(volumes), list(increments)
  if len(volumes) < 2 or len(volumes) != len(increments):
    raise ValueError(f'fit_motion_noise: {len(volumes)} volumes (at least 2) and {len(increments)} increments')
  cur = dict(sigma_xy=float(sigma_xy), sigma_yaw=float(sigma_yaw), uniform_mix=float(uniform_mix))
  records = []
  for _ in range(int(iterations)):
    beliefs, evidence, belief = [], [], None
    for votes, inc in zip(volumes, increments):
      if belief is not None and inc is None:
        inc = _no_motion()
      step = filter_votes(belief, votes, inc, grid, num_rotations, cur['sigma_xy'], cur['sigma_yaw'], temperature,
                          cur['uniform_mix'], truncate)
      belief = step['belief']
      beliefs.append(belief)
      evidence.append(step['log_evidence'])
    smoothed = smooth_track(beliefs, increments, grid, num_rotations, cur['sigma_xy'], cur['sigma_yaw'],
                            cur['uniform_mix'], truncate)
    stats = track_statistics(beliefs, smoothed, increments, grid, num_rotations, cur['sigma_xy'], cur['sigma_yaw'],
                             cur['uniform_mix'], truncate)
    m = noise_m_step(stats, increments, grid, num_rotations, cur['sigma_xy'], cur['sigma_yaw'], truncate, candidates)
    records.append(dict(cur, log_evidence=float(torch.stack(evidence).double().sum()), jump=m['jump'], m_step=m))
    cur = dict(sigma_xy=m['sigma_xy'], sigma_yaw=m['sigma_yaw'], uniform_mix=m['uniform_mix'])
  return cur, records
