"""An odometry increment and its noise -> the tap tables of the sequence kernels' predict step, in linear form
(``ops.vote_filter`` and its backward companions) and in log form (``ops.vote_viterbi``), and the one-tap tables of a
step without motion."""
import functools
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.models.votes.lattice import _shift_table_f64
from snap_amd.utils import geometry


# Limits of ops.vote_filter's tap tables (vote_filter.hip) and the smallest non-zero tap it is specified for.
FILTER_MAX_TAPS_K = 16
FILTER_MAX_TAPS_XY = 32
FILTER_MIN_TAP = 2.0 ** -20


def _axis_taps(centre, sigma, truncate, max_taps, what):
  """One axis of ``motion_taps``: centres [M] float64 (index units) and the standard deviation ``sigma`` (index
  units) -> (taps float64 [M, T], first offsets int64 [M]), T = 2 rho + 2 with rho = ceil(truncate * sigma)."""
  if not (sigma >= 0 and math.isfinite(sigma)) or not (truncate >= 0 and math.isfinite(truncate)):
    raise ValueError(f'motion_taps: {what}: sigma {sigma} (index units), truncate {truncate}')
  if not np.isfinite(centre).all() or np.abs(centre).max(initial=0.0) >= 2 ** 30:
    raise ValueError(f'motion_taps: {what}: shift {centre} (index units) is not a usable number')
  rho = int(math.ceil(truncate * sigma))
  T = 2 * rho + 2
  if T > max_taps:
    raise ValueError(f'motion_taps: {what}: ceil({truncate} * {sigma:.4g}) = {rho} index units needs {T} taps, '
                     f'the kernel has {max_taps}')
  i = np.arange(-rho, rho + 1, dtype=np.float64)
  g = np.exp(-i * i / (2 * sigma * sigma)) if rho > 0 else np.ones(1)
  g = g / g.sum()
  l = np.floor(centre)
  f = centre - l                                            # in [0, 1)
  w = np.zeros((len(centre), T))
  w[:, :T - 1] += (1 - f)[:, None] * g[None]
  w[:, 1:] += f[:, None] * g[None]
  w[w < FILTER_MIN_TAP] = 0.0
  w = w / w.sum(-1, keepdims=True)
  return w, l.astype(np.int64) - rho


def _motion_axes(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate):
  """The float64 host half of ``motion_taps``: one increment -> ((taps_k [1, Tk], lk [1]), (taps_a [R, Ta], la [R]),
  (taps_b [R, Tb], lb [R])), taps float64 and first offsets int64 (``_axis_taps`` per axis).  ``truncate``: one number,
  or one per axis (rotation, rows, columns)."""
  R = int(num_rotations)
  tr_k, tr_a, tr_b = truncate if isinstance(truncate, (tuple, list)) else (truncate,) * 3
  angle = torch.as_tensor(cur_t_prev.angle)
  if angle.numel() != 1:
    raise ValueError(f'motion_taps: one increment, got a transform of shape {tuple(angle.shape)}')
  host = geometry.Transform2D(angle.detach().to('cpu', torch.float64), torch.as_tensor(cur_t_prev.t).detach().to(
      'cpu', torch.float64))
  dk, da, db = (v.numpy() for v in _shift_table_f64(host, grid, R))
  cell = float(grid.cell_size)
  return (_axis_taps(dk, float(sigma_yaw) * R / (2 * math.pi), tr_k, FILTER_MAX_TAPS_K, 'rotation'),
          _axis_taps(da[0], float(sigma_xy) / cell, tr_a, FILTER_MAX_TAPS_XY, 'rows'),
          _axis_taps(db[0], float(sigma_xy) / cell, tr_b, FILTER_MAX_TAPS_XY, 'columns'))


def motion_taps(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate=3.0, device=None):
  """The tap tables of ``ops.vote_filter``'s predict step for one odometry increment: ``cur_t_prev`` is a Transform2D
  in corner frames, the previous frame's pose in the current frame's coordinates, so m_t_prev = m_t_cur @ cur_t_prev;
  ``sigma_xy`` (metres) and ``sigma_yaw`` (radians) are the increment's standard deviations ->
  (taps_k f32 [Tk], lk int, taps_a f32 [R, Ta], taps_b f32 [R, Tb], offsets int32 [R, 2] = (la, lb)) on ``device``
  (default: the transform's).

  The current pose (r, a, b) has its previous pose at the continuous index (r + dk, a + da(r), b + db(r)): row r of
  ``sequence_shift_table(cur_t_prev)`` before its rounding, float64.  Per axis, with the centre c = l + f,
  l = floor(c): w_j = (1 - f) g(j - l) + f g(j - l - 1) for j = l - rho .. l + rho + 1, g the Gaussian of the axis'
  standard deviation in index units (sigma_xy / cell_size, sigma_yaw R / 2 pi) sampled at the integers -rho .. rho,
  rho = ceil(truncate * sigma), normalised to sum 1 (a delta for sigma = 0): linear-interpolation transport followed
  by a blur.  The taps' mean is c exactly, they are continuous in sigma at 0, and with sigma = 0 they are
  ``ops.vote_fuse``'s own split (1 - f, f).  Entries below 2^-20 are set to 0 and the row renormalised, in float64;
  rounded to f32 once.  Built on the host (a transform on the device is read back: one synchronisation); raises
  ValueError where rho is beyond the kernel's tables (Tk <= 16, Ta, Tb <= 32)."""
  return _motion_tables(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device, log=False)


def motion_log_taps(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate=3.0, device=None):
  """``motion_taps``' tables for ``ops.vote_viterbi``: the same arguments, the same float64 construction and the same
  rounding of every tap w to f32, then float32(log(float64(w))), -inf for w = 0 -> (ltaps_k f32 [Tk], lk int, ltaps_a
  f32 [R, Ta], ltaps_b f32 [R, Tb], offsets int32 [R, 2]) on ``device``; the offsets are ``motion_taps``' own.  Every
  entry is -inf or a finite number <= 0.  Built on the host, one upload."""
  return _motion_tables(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device, log=True)


def _motion_tables(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device, log):
  """``motion_taps`` (``log`` False) and ``motion_log_taps`` (True): ``_motion_axes``' float64 tables rounded to f32
  once -- for ``log`` then float32(log(float64(w))), -inf for w = 0 -- and uploaded with the int32 offsets in one
  table."""
  R = int(num_rotations)
  if device is None:
    device = torch.as_tensor(cur_t_prev.angle).device
  (wk, lk), (wa, la), (wb, lb) = _motion_axes(cur_t_prev, grid, R, sigma_xy, sigma_yaw, truncate)
  # one upload: the three f32 tables, then the int32 offsets
  f32 = np.concatenate([wk.reshape(-1), wa.reshape(-1), wb.reshape(-1)]).astype(np.float32)
  if log:
    with np.errstate(divide='ignore'):
      f32 = np.log(f32.astype(np.float64)).astype(np.float32)
  off = np.stack([la, lb], -1).astype(np.int32)
  blob = ops.upload_table(np.concatenate([f32.view(np.uint8), off.reshape(-1).view(np.uint8)]), device)
  tab = blob[:f32.nbytes].view(torch.float32)
  nk, na = wk.size, wa.size
  return (tab[:nk], int(lk[0]), tab[nk:nk + na].view(R, -1), tab[nk + na:].view(R, -1),
          blob[f32.nbytes:].view(torch.int32).view(R, 2))


@functools.lru_cache(maxsize=32)
def _still_tables(fill, R, device):
  """One tap of value ``fill`` at offset 0 on every axis: the tables of a call without a predict step."""
  dev = torch.device(device)
  tap = torch.full((R, 1), fill, dtype=torch.float32, device=dev)
  return (torch.full((1,), fill, dtype=torch.float32, device=dev), 0, tap, tap.clone(),
          torch.zeros((R, 2), dtype=torch.int32, device=dev))


_still_taps = functools.partial(_still_tables, 1.0)       # weight 1: ``vote_filter``'s
_still_log_taps = functools.partial(_still_tables, 0.0)   # log-weight 0: ``vote_viterbi``'s
