"""Reference chain of OccupancyNet (snap/models/occupancy_net.py) for the tests (TEST INFRASTRUCTURE).

Composed from the numpy oracle -- ``oracle.lift.streetview_encoder``, ``oracle.grids.interpolate_nd``,
``oracle.encoder.mlp``, ``oracle.bev.log_sigmoid`` -- plus restatements of the ray sampler
(occupancy_net.py:34-60) and the loss / metrics (:131-166).  ``sample_rays_f32`` is ALSO the host
restatement of occupancy.hip's point arithmetic (same f32 expressions, no contraction): the kernel's
sample points must equal it bitwise.  ``occupancy_ray_features`` / ``occupancy_head`` /
``occupancy_head_supported`` are numpy twins of the ``snap_amd.ops`` entry points for CPU tests.

``fmaf32`` / ``gather_f32`` / ``head_f32`` restate the rest of occupancy.hip EXACTLY: the build has no
contraction (every f32 expression is one IEEE operation) and the f32 MFMA is a k-ordered ``fmaf`` chain
from its C input, so the fused head's logits are reproduced bit for bit on the host.
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


def fmaf32(a, b, c):
  """Vectorised f32 fused multiply-add, ONE rounding (C's fmaf; Python 3.10 has no math.fma).  The f32
  product is exact in float64; TwoSum gives s + e = a*b + c exactly; rounding s to odd (step one float64
  ulp toward e when e != 0 and s is even) keeps the sticky bit, and 53 >= 24 + 2 makes the final cast to
  f32 correctly rounded (ties to even, signed zeros, subnormals and overflow to +-inf included)."""
  a, b, c = (np.asarray(v, f32) for v in (a, b, c))
  with np.errstate(invalid='ignore', over='ignore'):
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = np.asarray(p + c64)
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = np.isfinite(s) & (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def _tap_base(lo, size):
  """occ_taps' il = (int)fminf(fmaxf(lo, -1), size): floor(c) clamped to [-1, size] (NaN -> -1) before
  the conversion (as int64)."""
  return np.fmin(np.fmax(lo, f32(-1)), f32(size)).astype(np.int64)


def gather_f32(volume, volume_valid, points, cell):
  """occupancy.hip's occ_taps / occ_taps_ok / occ_blend4 in numpy f32, the same expressions in the same
  order: volume [B, X, Y, Z, D], volume_valid [B, X, Y, Z] or None, points [B, P, 3] -> (features
  [B, P, D] f32, valid [B, P]).  Only the 8 taps of each point are read (a lazily zeroed volume stays
  untouched)."""
  points = np.asarray(points, f32)
  B, X, Y, Z, D = volume.shape
  size = (X, Y, Z)
  cell = f32(cell)
  idx, w = [], []
  inb = np.ones(points.shape[:-1], bool)
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    for t in range(3):
      p = points[..., t] / cell
      inb &= (p >= f32(0)) & (p < f32(size[t]))
      c = p - f32(0.5)
      lo = np.floor(c)
      whi = c - lo
      w.append((f32(1) - whi, whi))
      il = _tap_base(lo, size[t])
      idx.append((np.clip(il, 0, size[t] - 1), np.clip(il + 1, 0, size[t] - 1)))
    bidx = np.arange(B).reshape(B, *([1] * (points.ndim - 2)))
    bidx = np.broadcast_to(bidx, points.shape[:-1])
    acc = None
    ok = np.ones(points.shape[:-1], bool)
    for corner in range(8):
      bits = [(corner >> (2 - t)) & 1 for t in range(3)]
      wc = (w[0][bits[0]] * w[1][bits[1]]) * w[2][bits[2]]
      ix, iy, iz = (idx[t][bits[t]] for t in range(3))
      contrib = wc[..., None] * np.asarray(volume[bidx, ix, iy, iz], f32)
      acc = contrib if acc is None else acc + contrib
      if volume_valid is not None:
        ok &= np.asarray(volume_valid[bidx, ix, iy, iz], bool)
  return acc.astype(f32), inb & ok


def _snap_relu(v):
  return np.where(v < 0, f32(0), v).astype(f32)                # keeps -0.0 and NaN


def _fmaf_chain(x, w, acc=None):
  """acc = fmaf(x[:, k], w[k, :], acc) for k ascending, from +0.0: x [R, K], w [K, N] -> [R, N]."""
  x, w = np.asarray(x, f32), np.asarray(w, f32)
  if acc is None:
    acc = np.zeros((x.shape[0], w.shape[1]), f32)
  for k in range(x.shape[1]):
    acc = fmaf32(x[:, k, None], w[None, k, :], acc)
  return acc


def head_f32(feats, mlp):
  """The fused head's arithmetic on feature rows feats [R, D]: mlp = [(kernel [in, out], bias [out]),
  ...] with one or two hidden layers and a width-1 last layer -> logits [R] f32.  Hidden layer:
  relu(fmaf chain over k from +0.0, + bias).  Output, one hidden layer: fmaf chain over k from +0.0,
  then + bo.  Two hidden layers: per 32-column tile ct of the second, partial[ct] = fmaf chain over
  the tile's columns (ascending) from +0.0; acc = partial[0] + partial[1] + ... (ct order), + bo."""
  mlp = [(np.asarray(k, f32), np.asarray(b, f32)) for k, b in mlp]
  if len(mlp) not in (2, 3) or mlp[-1][0].shape[1] != 1:
    raise ValueError('head_f32: one or two hidden layers and a width-1 output layer')
  x = np.asarray(feats, f32)
  for k, b in mlp[:-1]:
    x = _snap_relu(_fmaf_chain(x, k) + b)
  wo, bo = mlp[-1]
  if len(mlp) == 2:
    acc = _fmaf_chain(x, wo)[:, 0]
  else:
    n = x.shape[1]
    partial = [_fmaf_chain(x[:, ct:ct + 32], wo[ct:ct + 32])[:, 0] for ct in range(0, n, 32)]
    acc = partial[0]
    for part in partial[1:]:
      acc = acc + part
  return (acc + bo[0]).astype(f32)


def head_layout(D, h1):
  """The LDS layout snap_occupancy_head_f32 instantiates for (D, first hidden width): 'small'
  (D, h1 <= 128), 'wide_a' (D > 128, h1 <= 128) or 'wide_ah' (h1 > 128)."""
  if D <= 128 and h1 <= 128:
    return 'small'
  return 'wide_a' if h1 <= 128 else 'wide_ah'


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
