"""Reference chain of OccupancyNet (snap/models/occupancy_net.py) for the tests (TEST INFRASTRUCTURE).

Composed from the numpy oracle -- ``oracle.lift.streetview_encoder``, ``oracle.grids.interpolate_nd``,
``oracle.encoder.mlp``, ``oracle.bev.log_sigmoid`` -- plus restatements of the ray sampler
(occupancy_net.py:34-60) and the loss / metrics (:131-166).  ``sample_rays_f32`` is ALSO the host
restatement of occupancy.hip's point arithmetic (same f32 expressions, no contraction): the kernel's
sample points must equal it bitwise.  ``occupancy_ray_features`` / ``occupancy_head`` /
``occupancy_head_supported`` are numpy twins of the ``snap_amd.ops`` entry points for CPU tests.
"""
import numpy as np
import torch

from oracle import bev as o_bev
from oracle import encoder as o_enc
from oracle import grids as o_grids
from oracle import lift as o_lift

f32 = np.float32


def sample_rays_f32(hits, origins, mask, num_samples, margin):
  """hits / origins [..., N, 3], mask [..., N] -> (points [..., S*N, 3], labels, valid), sample-major."""
  hits = np.asarray(hits, f32)
  origins = np.asarray(origins, f32)
  S = int(num_samples)
  d = hits - origins
  dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
  with np.errstate(invalid='ignore', divide='ignore'):
    d = d * ((dist - f32(margin)) / np.where(dist < 1, f32(1), dist))
  if S > 2:
    steps = np.arange(S - 1, dtype=f32) / f32(S - 2)
  else:
    steps = np.zeros(S - 1, f32)
  neg = steps.reshape(-1, *([1] * d.ndim)) * d[None] + origins[None]
  samples = np.concatenate([hits[None], neg], 0).astype(f32)              # [S, ..., N, 3]
  lead = hits.shape[:-2]
  N = hits.shape[-2]
  points = np.moveaxis(samples, 0, -3).reshape(*lead, S * N, 3)
  labels = np.zeros((S, N), bool)
  labels[0] = True
  labels = np.broadcast_to(labels.reshape(S * N), (*lead, S * N)).copy()
  valid = np.broadcast_to(np.asarray(mask, bool)[..., None, :], (*lead, S, N)).reshape(*lead, S * N).copy()
  return points, labels, valid


def interpolate_volume(volume, volume_valid, points, cell_size):
  """Per scene interpolate_nd(volume[b], points[b] / cell_size, valid[b]) -> (features [B, P, D], valid)."""
  feats, valid = [], []
  for b in range(len(volume)):
    idx = (np.asarray(points[b], f32) / f32(cell_size)).astype(volume.dtype)
    f, v = o_grids.interpolate_nd(volume[b], idx, None if volume_valid is None else volume_valid[b])
    feats.append(f)
    valid.append(v)
  return np.stack(feats), np.stack(valid)


def mlp(params, layers, x):
  return o_enc.mlp(params, {'layers': tuple(layers), 'apply_input_activation': False}, x)


def occupancy_net(params, config, grid, data):
  """occupancy_net.py:79-125 on numpy inputs (``data`` = the map scene of ``helpers.scene_to_oracle``
  plus ``lidar_rays`` / ``occupancy_queries`` as numpy)."""
  X, Y, Z = grid.extent
  idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij'), -1)
  xyz = ((idx + 0.5) * grid.cell_size).astype(f32)
  B = len(data['images'])
  sv = dict(data)
  sv['xyz_query'] = np.broadcast_to(xyz, (B, *xyz.shape)).copy()
  pred = o_lift.streetview_encoder(params['streetview_encoder'], config['streetview_encoder'], sv)
  vol = pred['feature_volume']
  queries = data.get('occupancy_queries')
  if queries is None:
    rays = data['lidar_rays']
    pts, labels, valid = sample_rays_f32(rays['points'], rays['origins'], rays['mask'],
                                         config['num_samples_per_ray'], config['ray_margin'])
    pred['ray_samples'] = dict(points=pts, labels=labels, valid=valid)
    queries = pts
  feats, valid = interpolate_volume(vol['features'], vol['valid'], queries, grid.cell_size)
  logits = mlp(params['mlp_out'], config['occupancy_mlp']['layers'], feats)[..., 0].astype(f32)
  pred['occupancy'] = dict(values=1 / (1 + np.exp(-logits)), valid=valid, logits=logits)
  return pred


def masked_mean(x, mask, axis):
  """layers.py:31-34."""
  div = np.sum(np.where(mask.any(axis, keepdims=True), mask, True), axis)
  return np.sum(x * mask, axis) / div


def loss_metrics(logits, labels, occ_valid, ray_valid):
  """occupancy_net.py:131-166 -> (losses, metrics), per example."""
  logits = np.asarray(logits, np.float64)
  mask = occ_valid & ray_valid
  bce = -np.where(labels, o_bev.log_sigmoid(logits), o_bev.log_sigmoid(-logits))
  bce = (masked_mean(bce, mask & labels, 1) + masked_mean(bce, mask & ~labels, 1)) / 2
  correct = (logits > 0) == labels
  metrics = {
      'occupancy/accuracy': masked_mean(correct, mask, 1),
      'occupancy/recall': masked_mean(correct, mask & labels, 1),
      'occupancy/precision': masked_mean(correct, mask & ~labels, 1),
  }
  return {'occupancy_bce': bce, 'total': bce}, metrics


# -- numpy twins of the snap_amd.ops entry points (CPU tests of the module) ------------------------
def _np(t):
  return None if t is None else t.detach().cpu().numpy()


def _points(rays, points, num_samples, margin):
  if rays is not None:
    hits, origins, mask = (_np(t) for t in rays)
    return sample_rays_f32(hits, origins, mask.astype(bool), num_samples, margin)
  return _np(points).astype(f32), None, None


def occupancy_ray_features(volume, volume_valid, cell_size, *, rays=None, points=None, num_samples=1, margin=0.0,
                           want_samples=True):
  pts, labels, rvalid = _points(rays, points, num_samples, margin)
  vv = None if volume_valid is None else _np(volume_valid).astype(bool)
  feats, valid = interpolate_volume(_np(volume).astype(f32), vv, pts, cell_size)
  samples = None
  if rays is not None and want_samples:
    samples = (torch.from_numpy(pts), torch.from_numpy(labels), torch.from_numpy(rvalid))
  return (torch.from_numpy(np.ascontiguousarray(feats.reshape(-1, feats.shape[-1]))), torch.from_numpy(valid),
          samples)


def occupancy_head_supported(D, hidden):
  hidden = tuple(hidden)
  ok = lambda w: 0 < w <= 256 and w % 32 == 0
  return len(hidden) in (1, 2) and ok(D) and all(ok(h) for h in hidden)


def occupancy_head(volume, volume_valid, cell_size, mlp_params, *, rays=None, points=None, num_samples=1,
                   margin=0.0, want_samples=True):
  feats, valid, samples = occupancy_ray_features(volume, volume_valid, cell_size, rays=rays, points=points,
                                                 num_samples=num_samples, margin=margin, want_samples=want_samples)
  params = {f'Dense_{i}': {'kernel': _np(k), 'bias': _np(b)} for i, (k, b) in enumerate(mlp_params)}
  logits = mlp(params, [k.shape[1] for k, _ in mlp_params], feats.numpy())[..., 0].astype(f32)
  return torch.from_numpy(logits.reshape(valid.shape)), valid, samples


TWINS = ('occupancy_ray_features', 'occupancy_head', 'occupancy_head_supported')
