"""Vote peaks -> continuous poses: the refinement lattice around every peak and its scoring on the two planes
themselves (``ops.plane_align_score``)."""
import functools
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.utils import geometry


def _bin_cos_sin(R):
  """float64 (cos, sin) of the R bin angles 2 pi r / R -> [R, 2].  The angle is reduced to a quarter turn first
  (4 r = q R + rem: 2 pi r / R = (q + rem / R) pi / 2) and the quarter turns are applied as sign swaps, so whole
  quarter turns are exactly (+-1, 0) / (0, +-1)."""
  r = np.arange(R)
  q, rem = np.divmod(4 * r, R)
  base = (np.pi / 2) * (rem / R)
  cb, sb = np.cos(base), np.sin(base)
  cos = np.choose(q, [cb, -sb, -cb, sb])
  sin = np.choose(q, [sb, cb, -sb, -cb])
  return np.stack([cos, sin], -1) + 0.0                   # (+ 0.0: no negative zeros)


@functools.lru_cache(maxsize=16)
def _refine_constants(R, steps_r, range_r, steps_xy, range_xy, device):
  """Device constants of ``refine_lattice``, float64, uploaded once per (rotations, lattice, device): (cos, sin) of
  the R bin angles [R, 2]; (dk, cos, sin of 2 pi dk / R) of the rotation offsets [steps_r, 3]; the cell offsets
  [steps_xy]."""
  dk = np.linspace(-range_r, range_r, steps_r)
  delta = 2 * np.pi * dk / R
  off = np.stack([dk, np.cos(delta), np.sin(delta)], -1)
  dxy = np.linspace(-range_xy, range_xy, steps_xy)
  return (torch.tensor(_bin_cos_sin(R), device=device), torch.tensor(off, device=device),
          torch.tensor(dxy, device=device))


def _refine_lattice_f64(index, grid, num_rotations, q_hw, steps_r, range_r, steps_xy, range_xy):
  """The lattice of ``refine_lattice`` before its rounding: float64 tensors [K, steps_r, steps_xy, steps_xy] on
  ``index``'s device -> (k, a, b, cos, sin, tx, ty) with (cos, sin, tx, ty) the map <- query transform in corner
  frames, translations in cells, and ``empty`` [K]."""
  index = torch.as_tensor(index)
  if index.dim() != 2 or index.shape[-1] != 3:
    raise ValueError(f'refine_lattice: index [K, 3], got {tuple(index.shape)}')
  R, steps_r, steps_xy = int(num_rotations), int(steps_r), int(steps_xy)
  H, W = (int(v) for v in grid.extent)
  if tuple(int(v) for v in q_hw) != (H, W):
    # exhaustive_index_to_tfm reads the shift and the rotation centre off the one extent of `grid`
    raise ValueError(f'refine_lattice: query plane {tuple(q_hw)} on a grid of extent {(H, W)}')
  if steps_r < 1 or steps_xy < 1:
    raise ValueError(f'refine_lattice: steps_r={steps_r} steps_xy={steps_xy}')
  rot, off, dxy = _refine_constants(R, steps_r, float(range_r), steps_xy, float(range_xy), str(index.device))
  empty = index[:, 0] < 0
  idx = index.to(torch.float64)
  row = rot[index[:, 0].long().clamp(0, R - 1)]
  shape = (index.shape[0], steps_r, steps_xy, steps_xy)
  cr, sr = row[:, 0, None], row[:, 1, None]
  cd, sd = off[None, :, 1], off[None, :, 2]
  cos_t = (cr * cd - sr * sd)[:, :, None, None].expand(shape)      # cos / sin of theta = 2 pi (r + dk) / R
  sin_t = (sr * cd + cr * sd)[:, :, None, None].expand(shape)
  k = (idx[:, 0, None] + off[None, :, 0])[:, :, None, None].expand(shape)
  a = (idx[:, 1, None] + dxy[None])[:, None, :, None].expand(shape)
  b = (idx[:, 2, None] + dxy[None])[:, None, None, :].expand(shape)
  # m_t_q = c @ (-theta, xy_cell) @ c^-1 with c = (0, centre): rotation -theta, t = centre + xy_cell - Rot centre
  c, s = cos_t, -sin_t
  cx, cy = H / 2, W / 2
  tx = cx + (a - H + 1 + 0.5) - (c * cx - s * cy)
  ty = cy + (b - W + 1 + 0.5) - (s * cx + c * cy)
  return (k, a, b, c, s, tx, ty), empty


def refine_lattice(index, grid, num_rotations, q_hw, steps_r=11, range_r=0.5, steps_xy=9, range_xy=1.0):
  """The refinement lattice around vote peaks: ``index`` int32 [K, 3] = (r, a, b) rows (``ops.vote_peaks``; any
  device; a row of -1 = no peak), ``q_hw`` the query plane's extent (= ``grid.extent``) ->

  * the continuous indices f32 [K, L, 3], L = steps_r * steps_xy^2: (r + dk, a + da, b + db) with dk on
    linspace(-range_r, range_r, steps_r) and da, db on linspace(-range_xy, range_xy, steps_xy); rotation slowest,
    then a, then b;
  * the pose table f32 [K * L, 4] = (cos, sin, tx, ty) of ``ops.plane_align_score``: ``exhaustive_index_to_tfm`` of
    the continuous index (the same +0.5 cell offset and corner-frame conjugation), translations in cells.

  Nothing is left to a device's transcendentals: cos / sin of the R bin angles and of the steps_r offsets are float64
  host tables, combined on the device by the angle-addition formulas in float64; everything is rounded to f32 once.
  Rows of a -1 peak are NaN."""
  (k, a, b, c, s, tx, ty), empty = _refine_lattice_f64(index, grid, num_rotations, q_hw, steps_r, range_r, steps_xy,
                                                      range_xy)
  K = k.shape[0]
  nan = torch.full((), float('nan'), device=k.device)
  cont = torch.stack((k, a, b), -1).to(torch.float32).reshape(K, -1, 3)
  poses = torch.stack((c, s, tx, ty), -1).to(torch.float32).reshape(K, -1, 4)
  cont = torch.where(empty[:, None, None], nan, cont)
  poses = torch.where(empty[:, None, None], nan, poses)
  return cont.contiguous(), poses.reshape(-1, 4).contiguous()


def refine_poses(plane_q, plane_map, index, grid, num_rotations, conf_q=None, min_overlap=0.05, **lattice):
  """Metric poses from vote peaks: scores the ``refine_lattice(**lattice)`` of every peak of ``index`` (int32
  [K, 3]) on the two planes themselves (``ops.plane_align_score``: the vote's own correlation and normaliser at
  continuous poses, threshold ``min_overlap`` * query cells) and keeps the best lattice pose per peak -> dict of
  device tensors, nothing synchronised: ``index`` f32 [K, 3] (continuous), ``score`` f32 [K], ``overlap`` int32
  [K], ``map_t_query`` Transform2D [K], ``lattice_scores`` f32 [K, steps_r, steps_xy, steps_xy].  The argmax has
  ``ops.argmax_rows``' order (the first maximum wins; an all -inf row gives lattice index 0).  A -1 peak gives
  score -inf, overlap 0, a NaN index and a NaN transform.  ``conf_q`` multiplies the query features, as in
  ``exhaustive_pose_voting``."""
  fq = plane_q.features
  if conf_q is not None:
    fq = fq * conf_q[..., None]
  dev = fq.device
  H, W = fq.shape[:2]
  index = torch.as_tensor(index).to(dev)
  kw = dict(steps_r=11, range_r=0.5, steps_xy=9, range_xy=1.0)
  unknown = set(lattice) - set(kw)
  if unknown:
    raise TypeError(f'refine_poses: unexpected keyword arguments {sorted(unknown)}')
  kw.update(lattice)
  (k, a, b, c, s, tx, ty), empty = _refine_lattice_f64(index, grid, num_rotations, (H, W), **kw)
  K, L = k.shape[0], k[0].numel()
  nan = torch.full((), float('nan'), device=dev)
  poses = torch.stack((c, s, tx, ty), -1).to(torch.float32).reshape(K, L, 4)
  poses = torch.where(empty[:, None, None], nan, poses).reshape(-1, 4).contiguous()
  thr = -1.0 if min_overlap is None else min_overlap * H * W
  score, overlap = ops.plane_align_score(fq.contiguous(), plane_q.valid.contiguous(), plane_map.features.contiguous(),
                                         plane_map.valid.contiguous(), poses, thr)
  score = score.reshape(K, L)
  best = ops.argmax_rows(score).long()[:, None]
  pick = lambda t: t.reshape(K, L).gather(1, best)[:, 0]
  cont = torch.stack([pick(v) for v in (k, a, b)], -1).to(torch.float32)
  angle = (pick(k) * (-2 * math.pi / int(num_rotations))).to(torch.float32)
  t = (torch.stack([pick(tx), pick(ty)], -1) * float(grid.cell_size)).to(torch.float32)
  return dict(
      index=torch.where(empty[:, None], nan, cont), score=pick(score), overlap=pick(overlap),
      map_t_query=geometry.Transform2D(torch.where(empty, nan, angle), torch.where(empty[:, None], nan, t)),
      lattice_scores=score.reshape(K, kw['steps_r'], kw['steps_xy'], kw['steps_xy']))
