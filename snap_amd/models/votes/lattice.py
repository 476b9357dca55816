"""The index lattice of a vote volume, as every module of the package reads it: the plane checks, a ground-truth pose
as an index, linear indices as (r, a, b), the shift table of a relative pose, and the small host conversions."""
import math

import numpy as np
import torch

from snap_amd.models.pose_exhaustive_voting import exhaustive_tfm_to_index
from snap_amd.utils import geometry


def _check_planes(fn, volume, num_rotations, name=None):
  """``volume`` holds one plane per rotation; with ``name`` (the track operators' wording) it is also [R, Ho, Wo]."""
  if name is None:
    if volume.shape[0] != num_rotations:
      raise ValueError(f'{fn}: {volume.shape[0]} vote planes for {num_rotations} rotations')
  elif volume.dim() != 3 or volume.shape[0] != num_rotations:
    raise ValueError(f'{fn}: {name} [{num_rotations}, Ho, Wo], got {tuple(volume.shape)}')


def _gt_index(m_t_q_gt, grid, num_rotations, device):
  """A ground-truth pose (or None) -> its ``exhaustive_tfm_to_index`` as f32 [3] on ``device`` (or None)."""
  if m_t_q_gt is None:
    return None
  gt = exhaustive_tfm_to_index(m_t_q_gt, grid, num_rotations).to(device=device, dtype=torch.float32)
  return gt.reshape(3).contiguous()


def _linear_to_indices(linear, shape):
  """Linear lattice indices int32 [...] -> (r, a, b) int32 [..., 3]; -1 rows where the index is negative."""
  P, Wo = shape[1] * shape[2], shape[2]
  lin = linear.long()
  indices = torch.stack([lin // P, (lin % P) // Wo, lin % Wo], -1).to(torch.int32)
  return torch.where((linear >= 0)[..., None], indices, indices.new_full((), -1))


def _shift_table_f64(q0_t_q, grid, num_rotations):
  """The float64 quantities of ``sequence_shift_table`` before their rounding: (dk [N] in [0, R), da [N, R],
  db [N, R]) on the transform's device."""
  R = int(num_rotations)
  phi = torch.as_tensor(q0_t_q.angle).to(torch.float64).reshape(-1)
  tau = torch.as_tensor(q0_t_q.t).to(torch.float64).reshape(-1, 2)
  dev = phi.device
  cx, cy = (float(v) / 2 for v in grid.extent_meters)
  cos, sin = torch.cos(phi), torch.sin(phi)
  rho_x = tau[:, 0] + (cos * cx - sin * cy - cx)
  rho_y = tau[:, 1] + (sin * cx + cos * cy - cy)
  theta = torch.arange(R, device=dev, dtype=torch.float64) * (2 * math.pi / R)
  ct, st = torch.cos(theta)[None], torch.sin(theta)[None]
  da = (ct * rho_x[:, None] + st * rho_y[:, None]) / grid.cell_size
  db = (-st * rho_x[:, None] + ct * rho_y[:, None]) / grid.cell_size
  dk = torch.remainder(-phi * (R / (2 * math.pi)), R)
  return dk, da, db


def sequence_shift_table(q0_t_q, grid, num_rotations):
  """The shift table of ``ops.vote_fuse`` for a sequence of query frames with known relative motion: ``q0_t_q`` is a
  Transform2D [N] in corner frames, frame n's pose in the anchor frame's coordinates, so m_t_qn = m_t_q0 @ q0_t_qn
  (an identity for the anchor itself) -> f32 [N, R, 3] on the transform's device.

  Row (n, r) = (dk, da, db): where the anchor pose has the index (r, a, b), frame n has the continuous index
  (r + dk, a + da, b + db).  In centre frames q0_t_qn is (phi_n, rho_n) with rho_n = tau_n + (Rot(phi_n) - I) center,
  center = grid.extent_meters / 2; composing it behind the anchor's (-2 pi r / R, xy_cell) and reading the index back
  (``exhaustive_index_to_tfm`` / ``exhaustive_tfm_to_index``) gives dk = -phi_n R / (2 pi) wrapped into [0, R) and
  (da, db) = Rot(-2 pi r / R) rho_n / cell_size: the +0.5 cell offsets cancel, and nothing depends on (a, b).
  Computed in float64 and rounded to f32 once; an identity transform gives an all-zero row."""
  dk, da, db = _shift_table_f64(q0_t_q, grid, num_rotations)
  R = int(num_rotations)
  dk = dk.to(torch.float32)
  dk = torch.where(dk >= R, torch.zeros_like(dk), dk)             # (a yaw just above 0 rounds up to R)
  return (torch.stack((dk[:, None].expand(-1, R), da.to(torch.float32), db.to(torch.float32)), -1) + 0.0).contiguous()


def _host_f64(x):
  return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


def _host_transform_f64(tfm):
  """A Transform2D of any shape -> the same as float64 host tensors, flattened to [U]."""
  angle = torch.as_tensor(tfm.angle).detach().to('cpu', torch.float64).reshape(-1)
  t = torch.as_tensor(tfm.t).detach().to('cpu', torch.float64).reshape(-1, 2)
  return geometry.Transform2D(angle, t)


def _wrap_angle(x):
  return x - 2 * math.pi * torch.floor((x + math.pi) / (2 * math.pi))


def _no_motion():
  return geometry.Transform2D(torch.zeros((), dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
