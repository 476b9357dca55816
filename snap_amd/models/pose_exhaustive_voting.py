"""Exhaustive (x, y, theta) pose voting (``snap/models/pose_exhaustive_voting.py``).

``template_matching`` has two formulations of the same correlation:

* ``method='fft'`` (voting_fft.hip; the default where the geometry fits): FFT products of the
  templates and the edge-padded map, channel pairs packed as complex numbers, the overlap count the
  same way and rounded to the nearest integer -- ~1e-3 of the direct form's multiply-adds, scores
  within ~1e-6 (relative to the largest score) of the direct sum, the -inf mask identical;
* ``method='direct'``: the dense contraction (2*R*(2H-1)(2W-1)*H*W*D flop) on the MFMA conv engine
  with the R rotated templates as an (H x W x D) -> R filter bank over the edge-padded map -- the
  reference's own formulation (``jax.scipy.signal.convolve``, :86-91) and the checker of the other.

Rotation, padding and the -inf / normalise pass are small HIP kernels (voting.hip).
"""
import fractions
import functools
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.models import types
from snap_amd.utils import geometry


def get_grid_center_transform(grid, device=None):
  """corner_t_center (pose_exhaustive_voting.py:31-34)."""
  center = torch.tensor((np.asarray(grid.extent_meters) / 2).astype(np.float32), device=device)
  return geometry.Transform2D(torch.zeros((), device=device), center)


def _template_transforms(num_rotations, grid, device):
  """templates_t_grid = corner_t_center @ rot(theta) @ corner_t_center^-1 (:44-50)."""
  angles = torch.tensor(
      np.linspace(0, np.pi * 2, num_rotations, endpoint=False).astype(np.float32)
  )
  c = get_grid_center_transform(grid)
  n = len(angles)
  corner = geometry.Transform2D(c.angle.expand(n), c.t.expand(n, 2))
  rot = geometry.Transform2D(angles, torch.zeros(n, 2))
  t = corner @ rot @ corner.inv
  tfm = torch.stack([torch.cos(t.angle), torch.sin(t.angle), t.t[:, 0], t.t[:, 1]], -1)
  return tfm.to(device=device, dtype=torch.float32).contiguous()


def sample_query_templates(features, valid, num_rotations, grid, _engine=False):
  """Rotate a BEV by ``num_rotations`` angles (pose_exhaustive_voting.py:37-69)."""
  if num_rotations % 4 != 0:
    raise ValueError('num_rotations must be divisible by 4')
  if features.shape[0] != features.shape[1]:
    raise ValueError('the rot90 completion requires a square BEV')
  tfm = _template_transforms(num_rotations, grid, features.device)
  H, W = features.shape[:2]
  out = ops.rotate_templates(
      features.contiguous(), valid.contiguous(), tfm[: num_rotations // 4].contiguous(),
      num_rotations, grid.cell_size,
      want_tw=_engine and not _stacked(num_rotations, (H, W)),   # (the stacked path reads `templates`)
  )
  if _engine:
    return out
  return out[0], out[1]


# Shift-stacking factor of the correlation GEMM (0 / 1 = plain direct form).  With R = 36 templates
# the GEMM has 36 output columns -- 56 % of a 64-wide MFMA tile; stacking the S x S shifted copies
# of every template as extra filters (and striding the correlation by S) gives R S^2 = 576 columns
# = 9 full tiles for 2.4 % more multiply-adds: the same products, summed in the same k order.
STACK_SHIFT = 4
STACK_MIN_CELLS = 64 * 64      # below this the plain form is already launch-bound
# 'auto': the frequency-domain form from FFT_MIN_CELLS map cells on (below, the direct form is a
# handful of launch-bound kernels), 'fft' / 'direct': forced.  Per call: the ``method`` argument.
# Two behaviours of the frequency-domain form differ from the direct form and are why 'direct' stays
# selectable: (1) the transforms are GLOBAL -- one NaN / Inf anywhere in the map features (valid cell or
# not: the reference does not mask them out of the scores either) or in the query plane makes every
# score of every rotation NaN, where the direct form poisons only the placements that overlap the bad
# cell; (2) its workspace grows with R * D * N^2 (0.9 GB of first-axis spectra at R = 36, 256^2, D = 32):
# 'auto' falls back to the direct form beyond FFT_WORKSPACE_BUDGET bytes.
VOTING_METHOD = 'auto'
FFT_MIN_CELLS = 64 * 64
FFT_WORKSPACE_BUDGET = 16 << 30


def _use_fft(method, R, q_hw, D, m_hw):
  method = method or VOTING_METHOD
  if method not in ('auto', 'fft', 'direct'):
    raise ValueError(f'voting method {method!r}: expected auto | fft | direct')
  if method == 'direct':
    return False
  ok = ops.voting_fft_supported(R, q_hw[0], q_hw[1], D, m_hw[0], m_hw[1])
  if method == 'fft':
    if not ok:
      raise ValueError(f'voting method fft: map {m_hw} is beyond the transform sizes of voting_fft.hip')
    return True
  return (ok and m_hw[0] * m_hw[1] >= FFT_MIN_CELLS
          and ops.voting_fft_workspace_bytes(R, q_hw[0], q_hw[1], D, m_hw[0], m_hw[1]) <= FFT_WORKSPACE_BUDGET)


def _stacked(R, q_hw):
  S = STACK_SHIFT
  return S > 1 and q_hw[0] * q_hw[1] >= STACK_MIN_CELLS and (R * S * S) % 4 == 0


def _correlate(mp, tw, R, q_hw, templates=None):
  """``tw`` [H,W,D,R] and / or ``templates`` [R,H,W,D]: the same filter bank in two layouts."""
  H, W = q_hw
  S = STACK_SHIFT
  Ho, Wo = mp.shape[0] - H + 1, mp.shape[1] - W + 1
  if not _stacked(R, q_hw):
    if tw is None:
      tw = templates.permute(1, 2, 3, 0).contiguous()
    return ops.conv2d(mp[None], tw)[0]                  # [Ho, Wo, R]
  A4, B4 = -(-Ho // S), -(-Wo // S)
  pb = max(0, S * (A4 - 1) + (H + S - 1) - mp.shape[0])  # zero rows only cropped outputs can see
  pr = max(0, S * (B4 - 1) + (W + S - 1) - mp.shape[1])
  tws_shape = (H + S - 1, W + S - 1, mp.shape[-1], R * S * S)
  presplit = (ops.precision() == 'bf16x3' and ops.USE_PRESPLIT_VOTING and mp.shape[-1] % 16 == 0
              and (R * S * S) % 192 == 0
              and ops.conv2d_presplit_supported((1,) + tuple(mp.shape), tws_shape, S, ((0, pb), (0, pr))))
  tws = None
  if presplit and templates is not None and ops.FUSED_TEMPLATE_PACK:
    # the bank goes straight into the engine's weight image (no f32 bank, no pack pass)
    tws = ops.pack_stacked_templates_split(templates, S)
  if tws is None:
    tws = ops.stack_templates(templates, S, 'rhwd') if templates is not None else ops.stack_templates(tw, S)
  if presplit:
    # the correlation as ONE large GEMM on the pre-split engine: the map is split into its two
    # bf16 parts once (instead of once per tap and column tile inside the K loop), both operands
    # travel by LDS-DMA, 256 x 192 tiles (R S^2 = 576 = three column tiles); same products, same
    # k order, same bits as the split engine's im2col body.  Template banks beyond the engine's
    # 32-bit offsets (matching_dim 64 at 256^2, queries of ~360^2 cells) keep the plain-input
    # launch below, which drops to the f32 engine where the split weight image does not fit
    raw4 = ops.conv2d(ops.presplit(mp[None]), tws, stride=S, padding=((0, pb), (0, pr)), ps_tile=3)[0]
  else:
    raw4 = ops.conv2d(mp[None], tws, stride=S, padding=((0, pb), (0, pr)))[0]   # [A4, B4, R*S*S]
  del tws
  raw = raw4.reshape(A4, B4, R, S, S).permute(0, 3, 1, 4, 2).reshape(A4 * S, B4 * S, R)
  return raw[:Ho, :Wo].contiguous()


def _overlap_count(mvp, cw, R, q_hw):
  """cnt[a, b, r] = sum_ij cw[i, j, r] * mvp[a+i, b+j]  (pose_exhaustive_voting.py:93-101).

  Plain form: a 1-channel correlation on the f32 engine's scalar path.  Large maps with
  W % 32 == 0: the template columns are folded into 32 input channels (j = 32 t + c) and the
  output columns into 32 images (b = 32 bq + br), X[br][row, col, c] = mvp[row, 32 col + br + c],
  which makes it a KH x (W/32) conv with Cin = 32 -- run on the bf16 engine.  EXACT: both
  operands are 0 / 1 (exact in bf16), every product is 0 / 1 and the f32 accumulator counts at
  most H W < 2^24 of them, so the result is the same integers."""
  H, W = q_hw
  if not _stacked(R, q_hw) or W % 32:
    return ops.conv2d(mvp[None, :, :, None].contiguous(), cw)[0]
  Hp, Wp = mvp.shape
  Ho, Wo = Hp - H + 1, Wp - W + 1
  nbq = -(-Wo // 32)                       # output column groups
  ncol = nbq + W // 32 - 1                 # decimated columns a group can touch
  need = 32 * (ncol - 1) + 31 + 31 + 1     # widest index + 1
  mv = torch.nn.functional.pad(mvp, (0, max(0, need - Wp)))
  win = mv.unfold(1, 32, 1)[:, :32 * ncol]                       # win[row, s, c] = mv[row, s + c]
  # (0 / 1 are exact in bf16: the folded image is written in the engine's element type, and the launch
  #  moves both operands by LDS-DMA -- conv_bf16_xh_kernel -- instead of converting f32 in its loop)
  X = win.reshape(Hp, ncol, 32, 32).permute(2, 0, 1, 3).to(torch.bfloat16).contiguous()   # [br, row, col, c]
  wq = cw.reshape(H, W // 32, 32, R)                               # [i, t, c, r], j = 32 t + c
  out = ops.conv2d(X, wq, math='bf16')                             # [32, Ho, nbq, R]
  return out.permute(1, 2, 0, 3).reshape(Ho, nbq * 32, R)[:, :Wo].contiguous()


def _match(tw, cw, tcount, R, q_hw, m, m_valid, min_overlap, templates=None):
  H, W = q_hw
  mp, mvp = ops.pad_map(m.contiguous(), m_valid.contiguous())
  raw = _correlate(mp, tw, R, q_hw, templates)          # [Ho, Wo, R]
  cnt = None
  if min_overlap is not None:
    cnt = _overlap_count(mvp, cw, R, q_hw)
  thr = 0.0 if min_overlap is None else min_overlap * H * W
  return ops.template_finalize(raw, cnt, tcount, R, thr, use_overlap=min_overlap is not None)


def template_matching(q, q_valid, m, m_valid, do_padding=True, min_overlap=0.05, method=None):
  """pose_exhaustive_voting.py:72-104 with explicit templates q [R,H,W,D]."""
  R, H, W, D = q.shape
  if do_padding and _use_fft(method, R, (H, W), D, tuple(m.shape[:2])):
    tcount = q_valid.sum((-1, -2)).to(torch.float32)
    thr = 0.0 if min_overlap is None else min_overlap * H * W
    return ops.voting_fft(q.contiguous(), q_valid.contiguous(), m.contiguous(), m_valid.contiguous(), tcount,
                          thr, use_overlap=min_overlap is not None)
  cw = q_valid.flip(1, 2).permute(1, 2, 0).to(torch.float32)[:, :, None, :].contiguous()
  tcount = q_valid.sum((-1, -2)).to(torch.float32)
  if not do_padding:
    # :82-86: no edge padding and jax.scipy.signal.convolve(mode='full') == the same
    # cross-correlation over the map extended by ZEROS.  The reference's overlap test pads the
    # validity mask regardless of do_padding (:93-96), which gives it a [4H-3, 4W-3] count
    # against [2H-1, 2W-1] scores: only min_overlap=None is a working combination there.
    if min_overlap is not None:
      raise ValueError('template_matching(do_padding=False) needs min_overlap=None '
                       '(the reference\'s shapes disagree otherwise)')
    mp = torch.nn.functional.pad(m, (0, 0, W - 1, W - 1, H - 1, H - 1)).contiguous()
    raw = _correlate(mp, None, R, (H, W), q.contiguous())
    return ops.template_finalize(raw, None, tcount, R, 0.0, use_overlap=False)
  return _match(None, cw, tcount, R, (H, W), m, m_valid, min_overlap, templates=q.contiguous())


def exhaustive_pose_voting(plane_q, plane_map, num_rotations, grid, conf_q=None, method=None):
  """pose_exhaustive_voting.py:107-124 -> scores [R, 2H-1, 2W-1]."""
  feats_q = plane_q.features
  if conf_q is not None:
    feats_q = feats_q * conf_q[..., None]
  H, W = feats_q.shape[:2]
  fft = _use_fft(method, num_rotations, (H, W), feats_q.shape[-1], tuple(plane_map.features.shape[:2]))
  if fft:
    # sample_query_templates runs INSIDE the first transform (rows interpolated on the fly, rot90
    # quadrants as index maps): the [R, H, W, D] template tensor is never written
    if num_rotations % 4 != 0:
      raise ValueError('num_rotations must be divisible by 4')
    if H != W:
      raise ValueError('the rot90 completion requires a square BEV')
    tfm = _template_transforms(num_rotations, grid, feats_q.device)[: num_rotations // 4].contiguous()
    return ops.voting_fft_rotated(feats_q.contiguous(), plane_q.valid.contiguous(), tfm, grid.cell_size,
                                  plane_map.features.contiguous(), plane_map.valid.contiguous(),
                                  num_rotations, 0.05)
  templates, tvalid, tw, cw, tcount = sample_query_templates(
      feats_q, plane_q.valid, num_rotations, grid, _engine=True
  )
  return _match(tw, cw, tcount, num_rotations, (H, W), plane_map.features, plane_map.valid, 0.05,
                templates=templates)


def exhaustive_index_to_tfm(index, grid, num_rotations):
  """pose_exhaustive_voting.py:127-137 (keeps the reference's +0.5 cell offset)."""
  index = torch.as_tensor(index)
  dev = index.device
  extent = torch.tensor(grid.extent, device=dev)
  xy_cell = ((index[1:] - extent + 1 + 0.5) * grid.cell_size).to(torch.float32)
  angle = (index[0] * 2 * math.pi / num_rotations).to(torch.float32)
  m_t_q_center = geometry.Transform2D(-angle, xy_cell)
  c = get_grid_center_transform(grid, dev)
  return c @ m_t_q_center @ c.inv


def exhaustive_tfm_to_index(m_t_q_corner, grid, num_rotations):
  """pose_exhaustive_voting.py:140-149."""
  dev = m_t_q_corner.t.device
  c = get_grid_center_transform(grid, dev)
  m_t_q_center = c.inv @ m_t_q_corner @ c
  k = (-m_t_q_center.angle / (math.pi * 2) % 1) * num_rotations
  ij = (m_t_q_center.t / grid.cell_size) + torch.tensor(grid.extent, device=dev) - 1.5
  return torch.cat([k[..., None], ij], -1)


@functools.lru_cache(maxsize=16)
def _index_to_tfm_constants(R, extent, cell_size, device):
  """Device constants of ``exhaustive_indices_to_tfm``, uploaded once per (rotations, grid, device): the [R, 3]
  table (-angle, cos, sin) computed on the host in f32, the extent, the grid centre in metres, a NaN."""
  neg_angle = -(np.arange(R) * 2 * np.pi / R).astype(np.float32)
  table = torch.tensor(np.stack([neg_angle, np.cos(neg_angle), np.sin(neg_angle)], -1), device=device)
  center = torch.tensor((np.asarray(extent) * cell_size / 2).astype(np.float32), device=device)
  return table, torch.tensor(extent, device=device), center, torch.full((), float('nan'), device=device)


def exhaustive_indices_to_tfm(indices, grid, num_rotations):
  """``exhaustive_index_to_tfm`` for ``indices`` [K, 3] = (r, a, b) rows -> Transform2D [K]: the same +0.5 cell
  offset and the same corner-frame conjugation c @ (-angle, xy_cell) @ c^-1, written out with c.angle = 0.

  The list of poses must not depend on where it is evaluated, so nothing here is left to a device's
  transcendentals: the cell offsets and the R angles are rounded to f32 from float64 (as the numpy restatement
  oracle/voting.py does), cos / sin come from an R-entry host table gathered by ``r``, and the rest is f32
  multiplies and adds in a fixed order.  A row of -1 (no peak: ``ops.vote_peaks`` past its found count) gives
  a NaN transform, not a plausible-looking pose."""
  indices = torch.as_tensor(indices)
  if indices.dim() != 2 or indices.shape[-1] != 3:
    raise ValueError(f'exhaustive_indices_to_tfm: indices [K, 3], got {tuple(indices.shape)}')
  dev = indices.device
  R = int(num_rotations)
  table, extent, center, nan = _index_to_tfm_constants(R, tuple(grid.extent), float(grid.cell_size), str(dev))
  empty = indices[:, 0] < 0
  row = table[indices[:, 0].long().clamp(0, R - 1)]
  xy_cell = ((indices[:, 1:].to(torch.float64) - extent + 1 + 0.5) * grid.cell_size).to(torch.float32)
  t = center + xy_cell                                     # c @ m_t_q_center
  bx, by = -center[0], -center[1]                          # c^-1 = (-0, -center)
  cos, sin = row[:, 1], row[:, 2]
  t = t + torch.stack([cos * bx + (-sin) * by, sin * bx + cos * by], -1)
  angle = 0.0 + row[:, 0]
  return geometry.Transform2D(torch.where(empty, nan, angle), torch.where(empty[:, None], nan, t))


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


def localize_exhaustive(plane_q, plane_map, num_rotations, grid, conf_q=None, method=None, posterior=None,
                        refine=None, credible=None, modes=None, recall=None, prior=None, **peaks):
  """``exhaustive_pose_voting`` followed by ``poses_from_votes(**peaks)``: the dict of the latter plus ``votes``.
  ``['map_t_query'][0]`` is the single best pose.  ``posterior``: True, or a dict of keyword arguments of
  ``posterior_from_votes`` (``temperature``, ``m_t_q_gt``), adds its result as ``['posterior']``.  ``refine``: True,
  or a dict of keyword arguments of ``refine_poses`` (``min_overlap``, the lattice), adds the peaks refined to
  continuous poses on the two planes as ``['refined']``.  ``credible``: True, or a dict of keyword arguments of
  ``credible_from_votes`` (``levels``, ``temperature``, ``m_t_q_gt``, ``cell_levels``), adds its result as
  ``['credible']``.  ``modes``: True, or a dict of keyword arguments of ``modes_from_votes`` (``win_r``, ``win_xy``,
  ``temperature``, ``m_t_q_gt``), adds the mixture around the peaks already found as ``['modes']`` (the window defaults
  to the peaks' radii; the posterior's ``log_z`` is reused where both have the same temperature).  ``recall``: True, or
  a dict of keyword arguments of ``recall_from_votes`` (``thresholds``, ``temperature``, ``m_t_q_gt``, ``maps``), adds
  its result for the peaks already found as ``['recall']``.  ``prior``: a ``pose_prior`` (or a dict of keyword
  arguments of ``prior_votes`` with it under ``'prior'``: ``temperature``, ``m_t_q_gt``); the frame's votes then go
  through ``prior_votes`` BEFORE the peaks and everything else are taken: ``votes`` is the normalised product,
  ``votes_frame`` the raw volume and ``['prior']`` the dict of ``prior_votes``."""
  votes = exhaustive_pose_voting(plane_q, plane_map, num_rotations, grid, conf_q=conf_q, method=method)
  fused = None
  if prior is not None:
    kw = dict(prior) if isinstance(prior, dict) else dict(prior=prior)
    fused = prior_votes(votes, kw.pop('prior'), grid, num_rotations, **kw)
    frame, votes = votes, fused['votes']
  out = poses_from_votes(votes, grid, num_rotations, **peaks)
  out['votes'] = votes
  if fused is not None:
    out['votes_frame'] = frame
    out['prior'] = fused
  if posterior is not None and posterior is not False:
    kw = {} if posterior is True else dict(posterior)
    out['posterior'] = posterior_from_votes(votes, grid, num_rotations, **kw)
  if refine is not None and refine is not False:
    kw = {} if refine is True else dict(refine)
    out['refined'] = refine_poses(plane_q, plane_map, out['index'], grid, num_rotations, conf_q=conf_q, **kw)
  if credible is not None and credible is not False:
    kw = {} if credible is True else dict(credible)
    out['credible'] = credible_from_votes(votes, grid, num_rotations, **kw)
  if modes is not None and modes is not False:
    out['modes'] = _modes_of_peaks(out, votes, grid, num_rotations, modes, posterior, peaks)
  if recall is not None and recall is not False:
    kw = {} if recall is True else dict(recall)
    out['recall'] = recall_from_votes(votes, grid, num_rotations, peaks=out['index'], **kw)
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


def fuse_votes(volumes, q0_t_q, grid, num_rotations, weights=None):
  """Fuse the vote volumes of N query frames with known relative motion into the anchor frame's volume
  (``ops.vote_fuse`` on ``sequence_shift_table``).  ``volumes``: f32 [N, R, 2H-1, 2W-1] or a list of N volumes;
  ``q0_t_q``: Transform2D [N], corner frames, m_t_qn = m_t_q0 @ q0_t_qn; ``weights``: None or N per-frame factors
  (a sequence of numbers or a tensor) -> (fused [R, 2H-1, 2W-1], count int32 [2] = (finite cells, NaN cells)).  The
  fused score exists only where every frame sees the pose (-inf elsewhere): it is again a vote volume, for
  ``poses_from_votes`` and ``posterior_from_votes``."""
  if not isinstance(volumes, torch.Tensor):
    volumes = torch.stack(list(volumes))
  if volumes.dim() != 4 or volumes.shape[1] != num_rotations:
    raise ValueError(f'fuse_votes: volumes [N, {num_rotations}, Ho, Wo], got {tuple(volumes.shape)}')
  shifts = sequence_shift_table(q0_t_q, grid, num_rotations)
  if shifts.shape[0] != volumes.shape[0]:
    raise ValueError(f'fuse_votes: {volumes.shape[0]} volumes for {shifts.shape[0]} relative poses')
  if weights is not None:
    weights = torch.as_tensor(weights, dtype=torch.float32).to(volumes.device).contiguous()
  return ops.vote_fuse(volumes.contiguous(), shifts.to(volumes.device), weights)


def localize_sequence(planes_q, plane_map, num_rotations, grid, q0_t_q, conf_q=None, method=None, weights=None,
                      posterior=None, modes=None, **peaks):
  """Sequence localization: ``exhaustive_pose_voting`` per query frame, ``fuse_votes`` with the frames' relative
  poses ``q0_t_q`` (Transform2D [N], corner frames, the anchor first as an identity), then
  ``poses_from_votes(fused, **peaks)``: the dict of ``localize_exhaustive`` with ``votes`` = the fused volume, plus
  ``votes_frames`` [N, R, 2H-1, 2W-1], ``count_fused`` (``fuse_votes``' count) and ``map_t_query_frames``, a
  Transform2D [K, N] = peak k composed with q0_t_qn (NaN past the found count).  ``conf_q``: None or one confidence
  per frame; ``posterior`` and ``modes`` as in ``localize_exhaustive``, on the fused volume."""
  planes_q = list(planes_q)
  conf_q = [None] * len(planes_q) if conf_q is None else list(conf_q)
  if len(conf_q) != len(planes_q):
    raise ValueError(f'localize_sequence: {len(conf_q)} confidences for {len(planes_q)} frames')
  frames = torch.stack([exhaustive_pose_voting(pq, plane_map, num_rotations, grid, conf_q=cq, method=method)
                        for pq, cq in zip(planes_q, conf_q)])
  fused, count_fused = fuse_votes(frames, q0_t_q, grid, num_rotations, weights)
  out = poses_from_votes(fused, grid, num_rotations, **peaks)
  out['votes'] = fused
  out['votes_frames'] = frames
  out['count_fused'] = count_fused
  rel = q0_t_q.to(device=fused.device, dtype=torch.float32)
  out['map_t_query_frames'] = out['map_t_query'].unsqueeze(-1) @ rel.unsqueeze(0)
  if posterior is not None and posterior is not False:
    kw = {} if posterior is True else dict(posterior)
    out['posterior'] = posterior_from_votes(fused, grid, num_rotations, **kw)
  if modes is not None and modes is not False:
    out['modes'] = _modes_of_peaks(out, fused, grid, num_rotations, modes, posterior, peaks)
  return out


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


def filter_votes(belief, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0,
                 uniform_mix=1e-3, truncate=3.0):
  """One step of the recursive pose filter (``ops.vote_filter`` on ``motion_taps``): ``belief`` [R, 2H-1, 2W-1] is the
  log-space belief after the previous frame, or None to start a track (a uniform prior; ``cur_t_prev`` is then
  ignored); ``votes`` the new frame's volume; ``cur_t_prev`` the odometry increment (Transform2D, corner frames,
  m_t_prev = m_t_cur @ cur_t_prev) with standard deviations ``sigma_xy`` (metres) / ``sigma_yaw`` (radians);
  ``temperature`` multiplies the votes; ``uniform_mix`` is the share of a uniform distribution mixed into the
  predicted prior (the track can recover from a pose it had ruled out) -> dict of device tensors: ``belief``
  [R, 2H-1, 2W-1] (normalised log-probabilities, -inf = impossible: a vote volume for ``poses_from_votes`` /
  ``posterior_from_votes`` / ``refine_poses``), ``log_evidence`` (of the frame under the predicted prior),
  ``mass_kept`` (the share of the previous belief that stayed inside the volume), ``count`` int32 [4] and ``stats``
  f32 [4] (the op's raw rows)."""
  _check_planes('filter_votes', votes, num_rotations, 'votes')
  if belief is None:
    taps = _still_taps(int(num_rotations), str(votes.device))
  else:
    taps = motion_taps(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device=votes.device)
    belief = belief.contiguous()
  out, stats, count = ops.vote_filter(belief, votes.contiguous(), taps, temperature, uniform_mix)
  return dict(belief=out, log_evidence=stats[0], mass_kept=stats[1], count=count, stats=stats)


def _no_motion():
  return geometry.Transform2D(torch.zeros((), dtype=torch.float64), torch.zeros(2, dtype=torch.float64))


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


def smooth_votes(belief, smoothed_next, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                 truncate=3.0):
  """One backward step of the smoother that goes with ``filter_votes`` (``ops.vote_smooth`` on ``motion_taps``):
  ``belief`` [R, 2H-1, 2W-1] is the filter's belief after frame t, ``smoothed_next`` the smoothed belief of frame
  t + 1 (for the last frame of a track: its filtered belief), ``next_t_cur`` the increment the filter was given at
  frame t + 1 (its ``cur_t_prev``) and the noise parameters that step's: ``motion_taps`` is deterministic on the host,
  so the tables are the filter's bit for bit -> dict of device tensors: ``smoothed`` [R, 2H-1, 2W-1] (normalised
  log-probabilities of p(x_t | all frames)), ``log_norm`` (0 up to rounding where beliefs and increment belong
  together), ``mass_kept`` (the filter's, of that step), ``count`` int32 [4] and ``stats`` f32 [4] (the op's raw rows)."""
  _check_planes('smooth_votes', belief, num_rotations, 'belief')
  taps = motion_taps(next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device=belief.device)
  out, stats, count = ops.vote_smooth(belief.contiguous(), smoothed_next.contiguous(), taps, uniform_mix)
  return dict(smoothed=out, log_norm=stats[0], mass_kept=stats[1], count=count, stats=stats)


def smooth_track(beliefs, increments, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3, truncate=3.0,
                 details=False):
  """The backward recursion over a track: ``beliefs`` are the N filtered beliefs (``filter_votes`` in frame order),
  ``increments`` the N increments the filter was given (entry 0 is ignored: a track starts from a uniform prior;
  None = no motion) -> the list of the N smoothed volumes, p(x_t | frames 0 .. N-1); the last is ``beliefs[-1]``
  itself.  With ``details`` the list holds ``smooth_votes``' dicts (None for the last frame)."""
  beliefs, increments = list(beliefs), list(increments)
  if not beliefs or len(beliefs) != len(increments):
    raise ValueError(f'smooth_track: {len(beliefs)} beliefs and {len(increments)} increments')
  smoothed, steps = [None] * len(beliefs), [None] * len(beliefs)
  smoothed[-1] = beliefs[-1]
  for t in range(len(beliefs) - 2, -1, -1):
    inc = increments[t + 1] if increments[t + 1] is not None else _no_motion()
    steps[t] = smooth_votes(beliefs[t], smoothed[t + 1], inc, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix,
                            truncate)
    smoothed[t] = steps[t]['smoothed']
  return steps if details else smoothed


# ``fit_motion_noise``: the default multiplicative candidate grid of the M-step, the range ``uniform_mix`` is kept in,
# and the smallest standard deviation (index units) a candidate is clipped to.
NOISE_CANDIDATES = (0.5, 0.7, 0.85, 1.0, 1.2, 1.5, 2.0)
NOISE_UNIFORM_MIX_RANGE = (1e-6, 0.5)
NOISE_MIN_SIGMA_INDEX = 1e-3


def pair_statistics(belief, smoothed_next, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                    truncate=3.0):
  """The tap posteriors of one filter step given all frames (``ops.vote_pairs`` on ``motion_taps``): arguments as
  ``smooth_votes`` -> dict of device tensors: ``hist_k`` float64 [Tk], ``hist_a`` [R, Ta], ``hist_b`` [R, Tb] (the
  posterior mass of the stay branch by tap, per axis; entry t of a row belongs to the offset first + t of that row's
  table), ``stay`` and ``jump`` (they sum to 1: ``jump`` is the share of the step's posterior that went through the
  uniform mix, i.e. the track was lost and re-acquired), ``log_norm`` (0 up to rounding where the arguments belong
  together), ``mass_kept``, ``count`` int32 [4], ``stats`` float64 [4], and ``taps``, the tuple used."""
  _check_planes('pair_statistics', belief, num_rotations, 'belief')
  taps = motion_taps(next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device=belief.device)
  hist_k, hist_a, hist_b, stats, count = ops.vote_pairs(belief.contiguous(), smoothed_next.contiguous(), taps,
                                                        uniform_mix)
  return dict(hist_k=hist_k, hist_a=hist_a, hist_b=hist_b, stay=stats[0], jump=stats[1], log_norm=stats[2],
              mass_kept=stats[3], count=count, stats=stats, taps=taps)


def track_statistics(beliefs, smoothed, increments, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                     truncate=3.0):
  """``pair_statistics`` of every step of a track: ``beliefs`` the N filtered beliefs, ``smoothed`` the N smoothed
  volumes (``smooth_track``), ``increments`` the N increments the filter was given (entry 0 ignored; None = no motion)
  -> the list of the N - 1 dicts, entry t for the step from frame t to frame t + 1."""
  beliefs, smoothed, increments = list(beliefs), list(smoothed), list(increments)
  if not beliefs or len(beliefs) != len(increments) or len(beliefs) != len(smoothed):
    raise ValueError(f'track_statistics: {len(beliefs)} beliefs, {len(smoothed)} smoothed volumes and '
                     f'{len(increments)} increments')
  return [pair_statistics(beliefs[t], smoothed[t + 1], increments[t + 1] if increments[t + 1] is not None
                          else _no_motion(), grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix, truncate)
          for t in range(len(beliefs) - 1)]


def _host_f64(x):
  return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


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


# Limits of ops.vote_odometry's window (vote_odometry.hip).
ODOMETRY_MAX_S = 32


def _host_transform_f64(tfm):
  """A Transform2D of any shape -> the same as float64 host tensors, flattened to [U]."""
  angle = torch.as_tensor(tfm.angle).detach().to('cpu', torch.float64).reshape(-1)
  t = torch.as_tensor(tfm.t).detach().to('cpu', torch.float64).reshape(-1, 2)
  return geometry.Transform2D(angle, t)


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


def _wrap_angle(x):
  return x - 2 * math.pi * torch.floor((x + math.pi) / (2 * math.pi))


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


class VoteFilter:
  """A track: the recursive pose filter of one vehicle on one map lattice.  Holds the grid, the number of rotations,
  the odometry noise (``sigma_xy`` metres, ``sigma_yaw`` radians per step), ``temperature``, ``uniform_mix``,
  ``truncate`` (``filter_votes``) and the current ``belief`` (None before the first frame and after ``reset()``).
  With ``keep_history`` every step's ``(belief, cur_t_prev)`` is appended to ``history`` (one volume per frame stays
  allocated) for ``smooth()``."""

  def __init__(self, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0, uniform_mix=1e-3, truncate=3.0,
               keep_history=False):
    self.grid = grid
    self.num_rotations = int(num_rotations)
    self.sigma_xy = float(sigma_xy)
    self.sigma_yaw = float(sigma_yaw)
    self.temperature = float(temperature)
    self.uniform_mix = float(uniform_mix)
    self.truncate = float(truncate)
    self.belief = None
    if keep_history:
      self.history = []

  def reset(self):
    """Drop the belief (and the history): the next ``step`` starts a track from a uniform prior."""
    self.belief = None
    if hasattr(self, 'history'):
      self.history = []

  def step(self, votes, cur_t_prev=None):
    """One filter step with the new frame's ``votes`` -> ``filter_votes``' dict; the belief is kept.  ``cur_t_prev``:
    the odometry increment since the previous step (ignored by the first step of a track); None = no motion (the
    belief is only diffused)."""
    if self.belief is not None and cur_t_prev is None:
      cur_t_prev = _no_motion()
    out = filter_votes(self.belief, votes, cur_t_prev, self.grid, self.num_rotations, self.sigma_xy, self.sigma_yaw,
                       self.temperature, self.uniform_mix, self.truncate)
    self.belief = out['belief']
    if hasattr(self, 'history'):
      self.history.append((out['belief'], cur_t_prev))
    return out

  def localize(self, plane_q, plane_map, cur_t_prev=None, conf_q=None, method=None, posterior=None, **peaks):
    """``exhaustive_pose_voting`` of the new frame, ``step``, then ``poses_from_votes(belief, **peaks)``: the dict of
    ``localize_exhaustive`` with ``votes`` = the belief, plus ``votes_frame`` (the frame's own votes),
    ``log_evidence`` and ``mass_kept``.  ``posterior`` as in ``localize_exhaustive``, on the belief."""
    frame = exhaustive_pose_voting(plane_q, plane_map, self.num_rotations, self.grid, conf_q=conf_q, method=method)
    step = self.step(frame, cur_t_prev)
    out = poses_from_votes(step['belief'], self.grid, self.num_rotations, **peaks)
    out['votes'] = step['belief']
    out['votes_frame'] = frame
    out['log_evidence'] = step['log_evidence']
    out['mass_kept'] = step['mass_kept']
    if posterior is not None and posterior is not False:
      kw = {} if posterior is True else dict(posterior)
      out['posterior'] = posterior_from_votes(step['belief'], self.grid, self.num_rotations, **kw)
    return out

  def credible(self, levels=(0.5, 0.9, 0.99), m_t_q_gt=None, cell_levels=False):
    """``credible_from_votes`` of the belief the filter holds (log-space and normalised, so the temperature is 1) ->
    its dict.  Raises ValueError before the first step."""
    if self.belief is None:
      raise ValueError('VoteFilter.credible: no belief (at least one step)')
    return credible_from_votes(self.belief, self.grid, self.num_rotations, levels=levels, temperature=1.0,
                               m_t_q_gt=m_t_q_gt, cell_levels=cell_levels)

  def modes(self, **kw):
    """``modes_from_votes(**kw)`` of the belief the filter holds (log-space and normalised, so the temperature is 1 and
    log_z is 0) -> its dict.  Raises ValueError before the first step."""
    if self.belief is None:
      raise ValueError('VoteFilter.modes: no belief (at least one step)')
    return modes_from_votes(self.belief, self.grid, self.num_rotations, temperature=1.0, log_z=0.0, **kw)

  def recall(self, **kw):
    """``recall_from_votes(**kw)`` of the belief the filter holds (log-space and normalised, so the temperature is 1)
    -> its dict.  Raises ValueError before the first step."""
    if self.belief is None:
      raise ValueError('VoteFilter.recall: no belief (at least one step)')
    return recall_from_votes(self.belief, self.grid, self.num_rotations, temperature=1.0, **kw)

  def rebase(self, new_t_old, drop_history=False):
    """Carry the belief the filter holds into another map frame (the vehicle drives onto the neighbouring map tile, or
    the map is re-anchored): ``rebase_votes(belief, new_t_old)`` with temperature 1 (the belief is log-space and
    normalised) -> its dict; the belief is replaced, so the track goes on where ``reset()`` would restart it from a
    uniform prior.  Cells the old lattice did not cover come out -inf; the next ``step``'s ``uniform_mix`` re-opens
    them.  The stored beliefs of a history are in the OLD frame and the smoother cannot mix frames: with a non-empty
    history this raises ValueError unless ``drop_history`` is true, which restarts the history empty.  Raises
    ValueError before the first step."""
    if self.belief is None:
      raise ValueError('VoteFilter.rebase: no belief (at least one step)')
    if getattr(self, 'history', None) and not drop_history:
      raise ValueError(f'VoteFilter.rebase: the {len(self.history)} stored beliefs are in the old map frame; '
                       'drop_history=True restarts the history')
    out = rebase_votes(self.belief, new_t_old, self.grid, self.num_rotations, temperature=1.0)
    self.belief = out['votes']
    if hasattr(self, 'history'):
      self.history = []
    return out

  def apply_prior(self, prior):
    """The measurement update of the belief the filter holds with a ``pose_prior`` (a GNSS fix, a compass):
    ``prior_votes(belief, prior)`` with temperature 1 (the belief is log-space and normalised) -> its dict; the belief
    is replaced.  With a history the belief of its last entry is replaced as well and that entry's ``cur_t_prev`` kept:
    a frame's stored belief is p(x_t | everything up to t), which now includes the fix.  ``step(votes)`` followed by
    ``apply_prior`` is the prior-times-votes start of a track.  Raises ValueError before the first step."""
    if self.belief is None:
      raise ValueError('VoteFilter.apply_prior: no belief (at least one step)')
    out = prior_votes(self.belief, prior, self.grid, self.num_rotations, temperature=1.0)
    self.belief = out['votes']
    if getattr(self, 'history', None):
      self.history[-1] = (out['votes'], self.history[-1][1])
    return out

  def estimate_increment(self, votes, **kw):
    """``increment_from_votes(belief, votes, **kw)``: the increment since the previous step from the belief the filter
    holds (log-space and normalised, so its temperature is 1) and the new frame's ``votes`` (the filter's
    temperature) -> its dict.  Nothing is stepped.  Raises ValueError before the first step."""
    if self.belief is None:
      raise ValueError('VoteFilter.estimate_increment: no belief (at least one step)')
    return increment_from_votes(self.belief, votes, self.grid, self.num_rotations, temperature_prev=1.0,
                                temperature_cur=self.temperature, **kw)

  def step_estimated(self, votes, **kw):
    """``step`` with the increment taken from the votes themselves: ``estimate_increment(votes, **kw)``, then
    ``step(votes, cur_t_prev=the MAP candidate)`` -> ``step``'s dict plus ``increment`` (``estimate_increment``'s dict;
    None for the first step of a track, which needs no increment).  Raises ValueError where no candidate has
    evidence."""
    if self.belief is None:
      out = self.step(votes)
      out['increment'] = None
      return out
    inc = self.estimate_increment(votes, **kw)
    if inc['cur_t_prev'] is None:
      raise ValueError('VoteFilter.step_estimated: no candidate increment has evidence')
    out = self.step(votes, cur_t_prev=inc['cur_t_prev'])
    out['increment'] = inc
    return out

  def smooth(self, posterior=None, **peaks):
    """The backward recursion over the history (``smooth_track``; each step's taps are rebuilt by ``motion_taps``) ->
    one dict per frame: ``poses_from_votes(smoothed, **peaks)`` plus ``votes`` (the smoothed volume; the last frame's
    is the filter's belief itself), ``log_norm`` (None for the last frame) and, with ``posterior`` as in
    ``localize_exhaustive``, ``posterior``.  Raises ValueError without a history."""
    if not getattr(self, 'history', None):
      raise ValueError('VoteFilter.smooth: no history (keep_history=True and at least one step)')
    beliefs, increments = zip(*self.history)
    steps = smooth_track(beliefs, increments, self.grid, self.num_rotations, self.sigma_xy, self.sigma_yaw,
                         self.uniform_mix, self.truncate, details=True)
    frames = []
    for belief, step in zip(beliefs, steps):
      votes = belief if step is None else step['smoothed']
      out = poses_from_votes(votes, self.grid, self.num_rotations, **peaks)
      out['votes'] = votes
      out['log_norm'] = None if step is None else step['log_norm']
      if posterior is not None and posterior is not False:
        kw = {} if posterior is True else dict(posterior)
        out['posterior'] = posterior_from_votes(votes, self.grid, self.num_rotations, **kw)
      frames.append(out)
    return frames

  def fit_noise(self, volumes=None, iterations=5, candidates=NOISE_CANDIDATES, apply=False):
    """``fit_motion_noise`` on the history's increments, starting from this filter's ``sigma_xy``, ``sigma_yaw`` and
    ``uniform_mix``.  The history keeps the beliefs, not the frames' own vote volumes, so ``volumes`` (the volumes the
    steps were given, ``localize``'s ``votes_frame``, in frame order) is required -> ``fit_motion_noise``'s pair (the
    fitted values, the per-iteration records).  The filter's parameters are left alone unless ``apply`` is true; the
    belief and the history are never touched (they were computed with the old values).  Raises ValueError without a
    history of at least two steps or when the volumes do not match it."""
    if len(getattr(self, 'history', None) or []) < 2:
      raise ValueError('VoteFilter.fit_noise: no history (keep_history=True and at least two steps)')
    if volumes is None or len(volumes) != len(self.history):
      raise ValueError(f'VoteFilter.fit_noise: the {len(self.history)} vote volumes the steps were given are needed '
                       '(the history keeps beliefs only)')
    increments = [h[1] for h in self.history]
    fitted, records = fit_motion_noise(volumes, increments, self.grid, self.num_rotations, self.sigma_xy,
                                       self.sigma_yaw, self.uniform_mix, self.temperature, self.truncate, iterations,
                                       candidates)
    if apply:
      self.sigma_xy, self.sigma_yaw, self.uniform_mix = fitted['sigma_xy'], fitted['sigma_yaw'], fitted['uniform_mix']
    return fitted, records

  def sample(self, num, seed):
    """``num`` whole tracks drawn from the joint posterior of the history's frames (``sample_tracks``: forward-filter /
    backward-sample on the stored beliefs; each step's taps are rebuilt by ``motion_taps``) -> its dict.  Raises
    ValueError without a history."""
    if not getattr(self, 'history', None):
      raise ValueError('VoteFilter.sample: no history (keep_history=True and at least one step)')
    beliefs, increments = zip(*self.history)
    return sample_tracks(beliefs, increments, self.grid, self.num_rotations, self.sigma_xy, self.sigma_yaw, num, seed,
                         self.uniform_mix, self.truncate)


def _linear_to_indices(linear, shape):
  """Linear lattice indices int32 [...] -> (r, a, b) int32 [..., 3]; -1 rows where the index is negative."""
  P, Wo = shape[1] * shape[2], shape[2]
  lin = linear.long()
  indices = torch.stack([lin // P, (lin % P) // Wo, lin % Wo], -1).to(torch.int32)
  return torch.where((linear >= 0)[..., None], indices, indices.new_full((), -1))


def sample_votes(votes, grid, num_rotations, num, seed, stream=0, temperature=1.0):
  """``num`` poses drawn from the pose distribution of a vote volume or a belief (``ops.vote_sample``): ``votes``
  [R, 2H-1, 2W-1]; ``seed`` (64 bits) and ``stream`` (int32; the frame number, say) key the Philox draws, so the same
  arguments give the same poses; ``temperature`` multiplies the votes -> dict of device tensors: ``linear`` int32
  [num] (the linear lattice index, -1 when no cell has mass), ``indices`` int32 [num, 3] = (r, a, b), ``m_t_q``
  (``exhaustive_indices_to_tfm`` of the indices: Transform2D [num], the cells' centre poses, no sub-cell jitter),
  ``log_prob`` f32 [num] (of the drawn cells), ``count`` int32 [2] and ``stats`` f32 [2] (the op's raw rows)."""
  _check_planes('sample_votes', votes, num_rotations, 'votes')
  linear, log_prob, stats, count = ops.vote_sample(votes.contiguous(), num, seed, stream, temperature)
  indices = _linear_to_indices(linear, votes.shape)
  return dict(linear=linear, indices=indices, m_t_q=exhaustive_indices_to_tfm(indices, grid, num_rotations),
              log_prob=log_prob, count=count, stats=stats)


def sample_back(belief, nxt, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, seed, stream, uniform_mix=1e-3,
                truncate=3.0):
  """One backward step of forward-filter / backward-sample (``ops.vote_sample_back`` on ``motion_taps``): ``belief``
  [R, 2H-1, 2W-1] is the filter's belief after frame t, ``nxt`` int32 [B] the chains' linear indices at frame t + 1,
  ``next_t_cur`` the increment the filter was given at frame t + 1 and the noise parameters that step's (as in
  ``smooth_votes``: the tables are the filter's bit for bit) -> dict of device tensors: ``linear`` int32 [B] (the
  chains' cells at frame t, -1 = none), ``jumped`` int32 [B] (1: the step was the uniform jump, 0: transported, -1: no
  predecessor), ``mass_kept``, ``count`` int32 [3] and ``stats`` f32 [2] (the op's raw rows)."""
  _check_planes('sample_back', belief, num_rotations, 'belief')
  taps = motion_taps(next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device=belief.device)
  prev, jumped, stats, count = ops.vote_sample_back(belief.contiguous(), nxt.contiguous(), taps, uniform_mix, seed,
                                                    stream)
  return dict(linear=prev, jumped=jumped, mass_kept=stats[0], count=count, stats=stats)


def sample_tracks(beliefs, increments, grid, num_rotations, sigma_xy, sigma_yaw, num, seed, uniform_mix=1e-3,
                  truncate=3.0):
  """``num`` whole tracks drawn from p(x_0 .. x_{N-1} | all frames) by forward-filter / backward-sample: ``beliefs``
  are the N filtered beliefs (``filter_votes`` in frame order), ``increments`` the N increments the filter was given
  (entry 0 is ignored; None = no motion).  ``sample_votes`` on the last belief with stream N - 1, then ``sample_back``
  down to frame 0 with stream t -> dict of device tensors with ``VoteViterbi.path(end=...)``'s shapes: ``linear`` int32
  [N, num], ``indices`` int32 [N, num, 3] (-1 where a track has no pose), ``m_t_q`` (Transform2D [N * num],
  frame-major) and ``jumps`` bool [N, num] (the step into frame t was the uniform jump; frame 0: False)."""
  beliefs, increments = list(beliefs), list(increments)
  if not beliefs or len(beliefs) != len(increments):
    raise ValueError(f'sample_tracks: {len(beliefs)} beliefs and {len(increments)} increments')
  N = len(beliefs)
  cur = sample_votes(beliefs[-1], grid, num_rotations, num, seed, N - 1)['linear']
  linear, jumps = [cur], []
  for t in range(N - 2, -1, -1):
    inc = increments[t + 1] if increments[t + 1] is not None else _no_motion()
    step = sample_back(beliefs[t], cur, inc, grid, num_rotations, sigma_xy, sigma_yaw, seed, t, uniform_mix, truncate)
    jumps.append(step['jumped'] == 1)
    cur = step['linear']
    linear.append(cur)
  jumps.append(torch.zeros_like(cur, dtype=torch.bool))
  linear = torch.stack(linear[::-1])
  indices = _linear_to_indices(linear, beliefs[-1].shape)
  return dict(linear=linear, indices=indices,
              m_t_q=exhaustive_indices_to_tfm(indices.reshape(-1, 3), grid, num_rotations),
              jumps=torch.stack(jumps[::-1]))


def motion_log_taps(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate=3.0, device=None):
  """``motion_taps``' tables for ``ops.vote_viterbi``: the same arguments, the same float64 construction and the same
  rounding of every tap w to f32, then float32(log(float64(w))), -inf for w = 0 -> (ltaps_k f32 [Tk], lk int, ltaps_a
  f32 [R, Ta], ltaps_b f32 [R, Tb], offsets int32 [R, 2]) on ``device``; the offsets are ``motion_taps``' own.  Every
  entry is -inf or a finite number <= 0.  Built on the host, one upload."""
  return _motion_tables(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device, log=True)


def _viterbi_log_weights(uniform_mix, n):
  """(log_stay, log_jump) = (float32(log1p(-eps)), float32(log(eps) - log(n))) as Python floats; -inf at eps = 1 / 0."""
  eps = float(uniform_mix)
  if not 0.0 <= eps <= 1.0:
    raise ValueError(f'viterbi_votes: uniform_mix must lie in [0, 1], got {uniform_mix}')
  with np.errstate(divide='ignore'):
    return float(np.float32(np.log1p(-np.float64(eps)))), float(np.float32(np.log(np.float64(eps)) - math.log(n)))


def viterbi_votes(score, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0,
                  uniform_mix=1e-3, truncate=3.0):
  """One forward step of the most-likely-track recursion (``ops.vote_viterbi`` on ``motion_log_taps``), the max-product
  companion of ``filter_votes`` with the same arguments: ``score`` [R, 2H-1, 2W-1] is the previous step's ``score``
  (the log score of the best path into every pose), or None to start a track (``cur_t_prev`` is then ignored) -> dict
  of device tensors: ``score`` [R, 2H-1, 2W-1] (a vote volume for ``poses_from_votes``), ``back`` int32 [R, 2H-1, 2W-1]
  (the linear index of every pose's best predecessor, -1 = none), ``peak_prev`` (M, the maximum of the previous score,
  which the step subtracted: the sum of these over a track restores the path's total), ``top`` (the largest score),
  ``count`` int32 [6] and ``stats`` f32 [2] (the op's raw rows); and what the step was run with, for
  ``VoteViterbi.path``: ``log_taps`` (the table tuple) and ``log_weights`` = (log_stay, log_jump) as Python floats.
  The transition is max((1 - eps) T, eps / n): log_stay = float32(log1p(-eps)), log_jump = float32(log(eps) - log(n)),
  eps = ``uniform_mix``."""
  _check_planes('viterbi_votes', votes, num_rotations, 'votes')
  log_stay, log_jump = _viterbi_log_weights(uniform_mix, votes.numel())
  if score is None:
    taps = _still_log_taps(int(num_rotations), str(votes.device))
  else:
    taps = motion_log_taps(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device=votes.device)
    score = score.contiguous()
  out, back, stats, count = ops.vote_viterbi(score, votes.contiguous(), taps, temperature, log_stay, log_jump)
  return dict(score=out, back=back, peak_prev=stats[0], top=stats[1], count=count, stats=stats, log_taps=taps,
              log_weights=(log_stay, log_jump))


def _entered_by_jump(cur, prev, best_prev, log_taps, shape, log_stay, log_jump):
  """Whether the step into the cells ``cur`` int32 [B] (their predecessors ``prev`` = back[cur]) was the uniform jump,
  from the step's tables alone, on the device -> bool [B].  A jump has prev == J (``best_prev``, the previous frame's
  best cell).  So has a transported step out of J, which the kernel takes iff log_stay + m2 >= log_jump, and then m2
  is the f32 value of the tap triple that leads from ``cur`` to J (d = 0 there): fl(ltb + fl(lta + ltk)), the largest
  over the rotation taps that reach J's plane.  f32 addition is monotone, so that triple's stay >= log_jump also
  implies that the kernel did not jump: the rule below is the kernel's decision exactly."""
  ltk, lk, lta, ltb, off = log_taps
  R, Ho, Wo = shape
  P = Ho * Wo
  x, j = cur.clamp(min=0).long(), best_prev.clamp(min=0).long()
  r, a, b = x // P, (x % P) // Wo, x % Wo
  kj, aj, bj = j // P, (j % P) // Wo, j % Wo
  ta, tb = aj - a - off[r, 0].long(), bj - b - off[r, 1].long()
  inside = (ta >= 0) & (ta < lta.shape[1]) & (tb >= 0) & (tb < ltb.shape[1])
  planes = torch.remainder(r[:, None] + lk + torch.arange(ltk.shape[0], device=cur.device)[None], R)
  m0 = torch.where(planes == kj, ltk[None], ltk.new_full((), -math.inf)).max(-1).values
  m2 = ltb[r, tb.clamp(0, ltb.shape[1] - 1)] + (lta[r, ta.clamp(0, lta.shape[1] - 1)] + m0)
  transported = inside & (m2.new_tensor(log_stay) + m2 >= log_jump)
  return (cur >= 0) & (best_prev >= 0) & (prev == best_prev) & ~transported


def viterbi_track(volumes, increments, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0, uniform_mix=1e-3,
                  truncate=3.0):
  """The jointly most likely pose sequence of a track: ``volumes`` are the N frames' vote volumes [R, 2H-1, 2W-1],
  ``increments`` the N odometry increments as ``VoteFilter.step`` takes them (entry 0 is ignored; None = no motion).
  ``viterbi_votes`` over the frames, then the back-pointers from the last frame's best pose (``ops.vote_backstep``)
  -> ``VoteViterbi.path()``'s dict: ``indices`` int32 [N, 3] = (r, a, b), ``linear`` int32 [N], ``m_t_q``
  (``exhaustive_indices_to_tfm`` of the indices), ``log_score`` (float64 scalar: the last ``top`` plus the steps'
  ``peak_prev`` for t >= 1) and ``jumps`` bool [N] (the step into frame t was the uniform jump), all on the device.
  One int32 volume per frame is held until the trace is done."""
  volumes, increments = list(volumes), list(increments)
  if not volumes or len(volumes) != len(increments):
    raise ValueError(f'viterbi_track: {len(volumes)} volumes and {len(increments)} increments')
  for v in volumes:
    if not isinstance(v, torch.Tensor) or v.dim() != 3 or v.shape != volumes[0].shape or v.shape[0] != num_rotations:
      raise ValueError(f'viterbi_track: every volume [{num_rotations}, Ho, Wo] of one shape, got '
                       f'{[tuple(getattr(u, "shape", ())) for u in volumes]}')
  track = VoteViterbi(grid, num_rotations, sigma_xy, sigma_yaw, temperature, uniform_mix, truncate)
  for v, inc in zip(volumes, increments):
    track.step(v, inc)
  return track.path()


class VoteViterbi:
  """A track's most likely pose sequence (the max-product companion of ``VoteFilter``, same arguments): ``step`` runs
  ``viterbi_votes`` on each new frame and keeps the current ``score`` (None before the first frame and after
  ``reset()``); ``path`` follows the back-pointers from the current best pose.  Every step's ``back`` is appended to
  ``history``: one int32 volume per frame stays allocated until ``reset()``."""

  def __init__(self, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0, uniform_mix=1e-3, truncate=3.0):
    self.grid = grid
    self.num_rotations = int(num_rotations)
    self.sigma_xy = float(sigma_xy)
    self.sigma_yaw = float(sigma_yaw)
    self.temperature = float(temperature)
    self.uniform_mix = float(uniform_mix)
    if not 0.0 <= self.uniform_mix <= 1.0:
      raise ValueError(f'VoteViterbi: uniform_mix must lie in [0, 1], got {uniform_mix}')
    self.truncate = float(truncate)
    self.score = None
    self.history = []

  def reset(self):
    """Drop the score and the back-pointers: the next ``step`` starts a track."""
    self.score = None
    self.history = []

  def step(self, votes, cur_t_prev=None):
    """One forward step with the new frame's ``votes`` -> ``viterbi_votes``' dict; ``score`` is kept and ``back``
    appended.  ``cur_t_prev`` as in ``VoteFilter.step``."""
    if self.score is not None:
      if tuple(votes.shape) != tuple(self.score.shape):
        raise ValueError(f'VoteViterbi.step: votes {tuple(votes.shape)} on a track of {tuple(self.score.shape)}')
      if cur_t_prev is None:
        cur_t_prev = _no_motion()
    out = viterbi_votes(self.score, votes, cur_t_prev, self.grid, self.num_rotations, self.sigma_xy, self.sigma_yaw,
                        self.temperature, self.uniform_mix, self.truncate)
    self.score = out['score']
    self.history.append(out)
    return out

  def path(self, end=None):
    """The back-pointers followed from the last frame to the first -> dict of device tensors: ``linear`` int32 [N],
    ``indices`` int32 [N, 3] = (r, a, b) (-1 where there is no path), ``m_t_q`` (``exhaustive_indices_to_tfm`` of the
    indices: Transform2D [N]), ``log_score`` (float64: the end pose's score plus the steps' ``peak_prev`` for t >= 1)
    and ``jumps`` bool [N] (the step into frame t was the uniform jump; frame 0: False).  ``end``: None = the current
    best pose (``count[5]``), or an int32 device tensor of B linear indices of the last frame (``vote_peaks`` of the
    score, say) to trace B alternatives at once: ``linear`` [N, B], ``indices`` [N, B, 3], ``jumps`` [N, B],
    ``log_score`` [B], ``m_t_q`` Transform2D [N * B] (frame-major).  No host synchronisation."""
    if not self.history:
      raise ValueError('VoteViterbi.path: no step yet')
    last = self.history[-1]
    single = end is None
    if single:
      cur = last['count'][5:6]
    else:
      if (not isinstance(end, torch.Tensor) or end.dtype != torch.int32 or end.dim() != 1 or end.numel() < 1
          or end.device != self.score.device):
        raise ValueError(f'VoteViterbi.path: end int32 [B] on {self.score.device}, got '
                         f'{(end.dtype, tuple(end.shape), end.device) if isinstance(end, torch.Tensor) else type(end)}')
      cur = end.contiguous()
    shape = tuple(self.score.shape)
    n = self.score.numel()
    flat = self.score.reshape(-1)
    known = (cur >= 0) & (cur < n)
    end_score = torch.where(known, flat[cur.clamp(0, n - 1).long()], flat.new_full((), -math.inf))
    log_score = end_score.double()
    linear, jumps = [cur], []
    for step in reversed(self.history[1:]):
      prev = ops.vote_backstep(step['back'], cur)
      jumps.append(_entered_by_jump(cur, prev, step['count'][4], step['log_taps'], shape, *step['log_weights']))
      log_score = log_score + step['peak_prev'].double()
      linear.append(prev)
      cur = prev
    jumps.append(torch.zeros_like(cur, dtype=torch.bool))
    linear = torch.stack(linear[::-1])                       # [N, B]
    jumps = torch.stack(jumps[::-1])
    P = shape[1] * shape[2]
    lin = linear.long()
    indices = torch.stack([lin // P, (lin % P) // shape[2], lin % shape[2]], -1).to(torch.int32)
    indices = torch.where((linear >= 0)[..., None], indices, indices.new_full((), -1))
    m_t_q = exhaustive_indices_to_tfm(indices.reshape(-1, 3), self.grid, self.num_rotations)
    if single:
      linear, jumps, indices, log_score = linear[:, 0], jumps[:, 0], indices[:, 0], log_score[0]
    return dict(indices=indices, linear=linear, m_t_q=m_t_q, log_score=log_score, jumps=jumps)

  def localize(self, plane_q, plane_map, cur_t_prev=None, conf_q=None, method=None, **peaks):
    """``exhaustive_pose_voting`` of the new frame, ``step``, then ``poses_from_votes(score, **peaks)``: the dict of
    ``localize_exhaustive`` with ``votes`` = the current score volume, plus ``votes_frame`` (the frame's own votes),
    ``back``, ``peak_prev`` and ``top``."""
    frame = exhaustive_pose_voting(plane_q, plane_map, self.num_rotations, self.grid, conf_q=conf_q, method=method)
    step = self.step(frame, cur_t_prev)
    out = poses_from_votes(step['score'], self.grid, self.num_rotations, **peaks)
    out['votes'] = step['score']
    out['votes_frame'] = frame
    out['back'] = step['back']
    out['peak_prev'] = step['peak_prev']
    out['top'] = step['top']
    return out
