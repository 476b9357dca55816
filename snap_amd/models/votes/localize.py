"""Voting followed by the analysis of the volume: the one-frame and the fused-sequence localizers."""
import torch

from snap_amd.models.pose_exhaustive_voting import exhaustive_pose_voting
from snap_amd.models.votes.analysis import (_modes_of_peaks, _with_posterior, credible_from_votes, poses_from_votes,
                                            recall_from_votes)
from snap_amd.models.votes.frames import prior_votes
from snap_amd.models.votes.raster import raster_votes
from snap_amd.models.votes.refine import refine_poses
from snap_amd.models.votes.sequence import fuse_votes


def localize_exhaustive(plane_q, plane_map, num_rotations, grid, conf_q=None, method=None, posterior=None,
                        refine=None, credible=None, modes=None, recall=None, prior=None, raster=None, **peaks):
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
  ``votes_frame`` the raw volume and ``['prior']`` the dict of ``prior_votes``.  ``raster``: a ``raster_prior`` (or a
  dict of keyword arguments of ``raster_votes`` with it under ``'raster'``: ``temperature``, ``strength``,
  ``m_t_q_gt``); the votes (the product with ``prior``, where both are given) go through ``raster_votes`` before the
  peaks are taken: ``votes`` is the normalised product, ``votes_frame`` the raw volume and ``['raster']`` the dict of
  ``raster_votes``."""
  votes = exhaustive_pose_voting(plane_q, plane_map, num_rotations, grid, conf_q=conf_q, method=method)
  fused = None
  if prior is not None:
    kw = dict(prior) if isinstance(prior, dict) else dict(prior=prior)
    fused = prior_votes(votes, kw.pop('prior'), grid, num_rotations, **kw)
    frame, votes = votes, fused['votes']
  rastered = None
  if raster is not None:
    kw = dict(raster) if isinstance(raster, dict) else dict(raster=raster)
    rastered = raster_votes(votes, kw.pop('raster'), grid, num_rotations, **kw)
    frame, votes = (votes if fused is None else frame), rastered['votes']
  out = poses_from_votes(votes, grid, num_rotations, **peaks)
  out['votes'] = votes
  if fused is not None:
    out['votes_frame'] = frame
    out['prior'] = fused
  if rastered is not None:
    out['votes_frame'] = frame
    out['raster'] = rastered
  _with_posterior(out, votes, grid, num_rotations, posterior)
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
  _with_posterior(out, fused, grid, num_rotations, posterior)
  if modes is not None and modes is not False:
    out['modes'] = _modes_of_peaks(out, fused, grid, num_rotations, modes, posterior, peaks)
  return out
