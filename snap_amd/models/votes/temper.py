"""A vote volume's statistics over a ladder of temperatures from one visit (``ops.temper_volume``), and the calibration
of the temperature against ground truth built on them."""
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.models.votes.lattice import _check_planes, _gt_index


def _ladder_f32(fn, temperatures):
  """A temperature ladder as the float64 values of its f32 roundings (what the kernel multiplies by): 1 to 16 finite
  numbers > 0, strictly increasing after the rounding, else ValueError."""
  t = np.asarray(temperatures, dtype=np.float64).reshape(-1)
  with np.errstate(over='ignore'):
    t32 = t.astype(np.float32)
  if not (1 <= t32.size <= 16 and bool(np.all(np.isfinite(t32))) and bool(np.all(t32 > 0))
          and bool(np.all(np.diff(t32) > 0))):
    raise ValueError(f'{fn}: temperatures must be 1 to 16 finite numbers > 0, strictly increasing as f32, got '
                     f'{t.tolist()}')
  return t32.astype(np.float64)


def temperature_ladder(lo, hi, num):
  """A geometric ladder of ``num`` temperatures from ``lo`` to ``hi`` (both included; ``num`` = 1: ``lo`` alone) as a
  float64 numpy array whose f32 roundings increase strictly; ValueError where they do not (``lo`` and ``hi`` too close
  for ``num`` steps of f32), or where 0 < lo <= hi < inf and 1 <= num <= 16 does not hold."""
  lo, hi, num = float(lo), float(hi), int(num)
  if not (1 <= num <= 16 and 0.0 < lo <= hi < math.inf and (num == 1 or lo < hi)):
    raise ValueError(f'temperature_ladder: 0 < lo < hi < inf and 1 <= num <= 16, got lo={lo} hi={hi} num={num}')
  if num == 1:
    t = np.array([lo], dtype=np.float64)
  else:
    t = lo * (hi / lo) ** (np.arange(num, dtype=np.float64) / (num - 1))
    t[0], t[-1] = lo, hi
  _ladder_f32('temperature_ladder', t)
  return t


def temper_votes(votes, grid, num_rotations, temperatures, m_t_q_gt=None):
  """The statistics of p_s = softmax(s * votes) of a vote volume [R, 2H-1, 2W-1] at every temperature s of a ladder,
  from one visit of the volume (``ops.temper_volume``; ``temperatures``: 1 to 16 host numbers, strictly increasing as
  f32, e.g. ``temperature_ladder``) -> dict of device tensors, float64 [S] unless noted, nothing synchronised:

  ``log_z``; ``mean_vote`` = E_s[v] = d log_z / d s; ``var_vote`` = Var_s[v] = d2 log_z / d s2; ``entropy`` and
  ``log_p_max`` (the log-probability of the best cell): the frame's "entropy and confidence against temperature" curve;
  ``count`` int32 [4] = (finite cells, NaN / +inf cells, ground-truth sample valid, 0); ``table`` [S, 8] and ``stats``
  [4], the op's raw rows.  With ``m_t_q_gt`` (a Transform2D, map corner frame; sampled at ``exhaustive_tfm_to_index`` of
  it by ``posterior_from_votes``' rule): ``log_prob_gt`` = -nll at every temperature, ``nll_slope`` = d nll / d s =
  E_s[v] - v_gt and ``valid_gt`` (bool; both are NaN where it is False); without it they are NaN and False."""
  _check_planes('temper_votes', votes, num_rotations)
  gt = _gt_index(m_t_q_gt, grid, num_rotations, votes.device)
  table, stats, count = ops.temper_volume(votes.contiguous(), _ladder_f32('temper_votes', temperatures), gt)
  return dict(log_z=table[:, 0], mean_vote=table[:, 1], var_vote=table[:, 2], entropy=table[:, 3],
              log_p_max=table[:, 4], log_prob_gt=table[:, 5], nll_slope=table[:, 6], valid_gt=count[2] != 0,
              count=count, table=table, stats=stats)


def _hermite_root(a, b, g0, g1, d0, d1):
  """The root in [a, b] of the cubic Hermite interpolant of a function with values g0 <= 0 <= g1 and derivatives d0, d1
  at a and b, by bisection on the interpolant (it changes sign on [a, b] whatever the derivatives); the midpoint of the
  bracket where the interpolant is not finite."""
  h = b - a
  def p(t):
    t2, t3 = t * t, t * t * t
    return ((2 * t3 - 3 * t2 + 1) * g0 + (t3 - 2 * t2 + t) * h * d0 + (-2 * t3 + 3 * t2) * g1 + (t3 - t2) * h * d1)
  if not all(math.isfinite(x) for x in (g0, g1, d0, d1)):
    return a + 0.5 * h
  lo, hi = 0.0, 1.0
  for _ in range(64):
    mid = 0.5 * (lo + hi)
    if p(mid) < 0.0:
      lo = mid
    else:
      hi = mid
  x = a + 0.5 * (lo + hi) * h
  return x if a <= x <= b else a + 0.5 * h


def solve_temperature(temperatures, nll, slope, var, frames):
  """The host half of ``TemperatureFit.solve``, on float64 numpy rows over the ladder: the summed ground-truth ``nll``,
  its derivative ``slope`` = sum (E_s[v] - v_gt) and second derivative ``var`` = sum Var_s[v] >= 0, over ``frames``
  valid frames.  The NLL is convex in s, so its minimiser lies where the slope changes sign: the bracket is the pair
  of neighbouring ladder points with slope < 0 on the left and >= 0 on the right, and the estimate the root of the
  cubic Hermite interpolant of the slope on it (values and derivatives at both ends; ``_hermite_root``).  Without a
  sign change on the ladder ``bracketed`` is False, ``temperature`` the end of the ladder with the smaller NLL and the
  bracket that point twice; without a frame ``temperature`` is NaN."""
  t = np.asarray(temperatures, dtype=np.float64).reshape(-1)
  nll, g, var = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (nll, slope, var))
  frames = int(frames)
  out = dict(nll=nll.copy(), frames=frames, temperatures=t.copy())
  if frames == 0 or not np.all(np.isfinite(g)):
    return dict(out, temperature=float('nan'), bracket=(float('nan'), float('nan')), bracketed=False)
  up = np.flatnonzero(g >= 0.0)
  if up.size and up[0] > 0:
    l = int(up[0]) - 1
    root = _hermite_root(t[l], t[l + 1], g[l], g[l + 1], var[l], var[l + 1])
    return dict(out, temperature=float(root), bracket=(float(t[l]), float(t[l + 1])), bracketed=True)
  if up.size and g[0] == 0.0:                                    # the first ladder point is the minimiser
    return dict(out, temperature=float(t[0]), bracket=(float(t[0]), float(t[0])), bracketed=True)
  end = 0 if nll[0] <= nll[-1] else t.size - 1
  return dict(out, temperature=float(t[end]), bracket=(float(t[end]), float(t[end])), bracketed=False)


class TemperatureFit:
  """The one-parameter calibration of the exhaustive path: the temperature s that minimises the ground-truth NLL of
  p_s = softmax(s * votes) over a validation set, from ONE visit of every frame.  ``add`` evaluates a frame on the whole
  ladder (``ops.temper_volume``) and adds, on the device in float64 and without a synchronisation, the frame's nll,
  nll slope E_s[v] - v_gt and Var_s[v] per ladder point and the valid-frame count; a frame whose ground truth is
  invalid (outside the volume, on a masked cell) adds nothing.  ``solve`` synchronises once."""

  def __init__(self, grid, num_rotations, temperatures):
    self.grid, self.num_rotations = grid, int(num_rotations)
    self.temperatures = _ladder_f32('TemperatureFit', temperatures)
    self._sums = None                                            # float64 [S, 3] = (nll, slope, var), where the tables live
    self._frames = None

  def add(self, votes, m_t_q_gt):
    _check_planes('TemperatureFit.add', votes, self.num_rotations)
    gt = _gt_index(m_t_q_gt, self.grid, self.num_rotations, votes.device)
    table, _, count = ops.temper_volume(votes.contiguous(), self.temperatures, gt)
    self.add_table(table, count)

  def add_table(self, table, count):
    """The same from a stored ``ops.temper_volume`` table [S, 8] and count [4] (tensors on any one device)."""
    if tuple(table.shape) != (self.temperatures.size, 8) or tuple(count.shape) != (4,):
      raise ValueError(f'TemperatureFit.add_table: table [{self.temperatures.size}, 8] and count [4], got '
                       f'{tuple(table.shape)} and {tuple(count.shape)}')
    table = table.to(torch.float64)
    valid = count[2] != 0
    row = torch.stack((-table[:, 5], table[:, 6], table[:, 2]), -1)
    row = torch.where(valid, row, torch.zeros_like(row))
    if self._sums is None:
      self._sums, self._frames = row, valid.to(torch.int64)
    else:
      self._sums = self._sums + row
      self._frames = self._frames + valid.to(torch.int64)

  def solve(self):
    """-> dict(temperature, bracket = (lo, hi), bracketed, nll [S] at the ladder points, frames, temperatures [S]):
    ``solve_temperature`` on the sums."""
    if self._sums is None:
      zero = np.zeros(self.temperatures.size)
      return solve_temperature(self.temperatures, zero, zero, zero, 0)
    packed = torch.cat((self._sums.reshape(-1), self._frames.to(torch.float64).reshape(1))).cpu().numpy()
    sums = packed[:-1].reshape(-1, 3)
    return solve_temperature(self.temperatures, sums[:, 0], sums[:, 1], sums[:, 2], int(packed[-1]))


def fit_temperature(volumes, m_t_q_gts, grid, num_rotations, lo, hi, num=16, rounds=3):
  """``TemperatureFit`` for volumes held in memory: round 1 on ``temperature_ladder(lo, hi, num)``, every further round
  on a fresh ladder over the previous round's bracket, which so shrinks by ``num`` - 1 per round in the exponent (the
  curvature is not trusted: the Hermite estimate is only read off the last bracket).  It stops early where a round does
  not bracket the minimiser or the bracket no longer holds ``num`` distinct f32 temperatures -> the last round's
  ``solve()`` dict plus ``brackets``, the list of every round's bracket."""
  volumes, m_t_q_gts = list(volumes), list(m_t_q_gts)
  if len(volumes) != len(m_t_q_gts):
    raise ValueError(f'fit_temperature: {len(volumes)} volumes for {len(m_t_q_gts)} ground truths')
  brackets, out = [], None
  for _ in range(int(rounds)):
    try:
      ladder = temperature_ladder(lo, hi, num)
    except ValueError:
      if out is None:
        raise
      break
    fit = TemperatureFit(grid, num_rotations, ladder)
    for votes, gt in zip(volumes, m_t_q_gts):
      fit.add(votes, gt)
    out = fit.solve()
    brackets.append(out['bracket'])
    lo, hi = out['bracket']
    if not out['bracketed'] or not lo < hi:
      break
  if out is None:
    raise ValueError(f'fit_temperature: rounds must be >= 1, got {rounds}')
  return dict(out, brackets=brackets)
