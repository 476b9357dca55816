"""Per-point occupancy from the StreetView feature volume (``snap/models/occupancy_net.py``).

``OccupancyNet`` = ``StreetViewEncoder`` on the meta grid's voxel centres (no BEV mapper, z offset
or vertical pooling) -> query points (lidar-ray samples, or ``data['occupancy_queries']``) ->
trilinear interpolation of the volume -> ``MLP(occupancy_mlp)`` -> logits.  The query chain is
occupancy.hip: ONE fused launch (``ops.occupancy_head``) when nothing needs gradients, or the
producer (``ops.occupancy_ray_features``: samples + interpolated rows) followed by the MLP on the
Dense engine.  ``OccupancyNetModel`` carries the balanced BCE loss and the metrics (:131-166).

The encoder is frozen in the reference's training config (train_occupancy.py:29).  A model built with
``train_encoder=True`` also trains it through the head: when an encoder parameter requires grad, the
encoder runs under autograd (its own VJPs) and the query chain is ``ag.occupancy_ray_features`` (the
deterministic gather VJP into the volume, occupancy.hip) followed by the Dense chain.  Without
``train_encoder`` such a forward raises, as before (freeze it:
``trainer.train_step(..., freeze_params_reg_exp='streetview_encoder/')``).
"""
import torch

from snap_amd import autograd as ag
from snap_amd import ops
from snap_amd.configs import defaults as default_configs
from snap_amd.models import base
from snap_amd.models import layers
from snap_amd.models import streetview_encoder
from snap_amd.models import types
from snap_amd.models.semantic_net import masked_mean

F32_CLASS = ('f32', 'bf16x3', 'bf16x6')


def sample_queries_from_rays(hits, origins, valid, num_samples, margin):
  """occupancy_net.py:34-60, batched over the leading axes: hits / origins [..., N, 3], valid [..., N]
  -> LidarRaySamples(points [..., S*N, 3], labels, valid), sample-major (element k * N + n).  Sample 0
  is the hit (label True); samples 1..S-1 are origin + linspace(0, 1, S-1) * dir (label False) with
  dir = (hit - origin) * (|d| - margin) / max(|d|, 1) -- the reference's clip(min=1), kept.  The same
  f32 expressions as occupancy.hip (which produces these points inside the query kernels)."""
  S = int(num_samples)
  d = hits - origins
  dist = torch.sqrt((d[..., 0:1] * d[..., 0:1] + d[..., 1:2] * d[..., 1:2]) + d[..., 2:3] * d[..., 2:3])
  d = d * ((dist - margin) / torch.where(dist < 1, torch.ones_like(dist), dist))
  if S > 2:
    steps = torch.arange(S - 1, dtype=hits.dtype, device=hits.device) / torch.tensor(
        S - 2, dtype=hits.dtype, device=hits.device)
  else:
    steps = torch.zeros(S - 1, dtype=hits.dtype, device=hits.device)
  neg = steps.reshape(-1, *([1] * d.dim())) * d.unsqueeze(0) + origins.unsqueeze(0)     # [S-1, ..., N, 3]
  samples = torch.cat([hits.unsqueeze(0), neg], 0)                                    # [S, ..., N, 3]
  lead = hits.shape[:-2]
  N = hits.shape[-2]
  samples = samples.movedim(0, -3).reshape(*lead, S * N, 3)
  labels = torch.zeros((S, N), dtype=torch.bool, device=hits.device)
  labels[0] = True
  labels = labels.reshape(S * N).expand(*lead, S * N)
  valid = valid.to(torch.bool).unsqueeze(-2).expand(*lead, S, N).reshape(*lead, S * N)
  return types.LidarRaySamples(points=samples, labels=labels, valid=valid)


def dense_chain(mlp, x):
  """MLP(occupancy_mlp) on the Dense engine in force (layers.py:55-78: ReLU between layers): ``mlp`` =
  [(kernel [in, out], bias [out]), ...], x [M, in] -> [M, out_last].  The engine writes column quads, so a
  layer whose width is not a multiple of 4 (the width-1 logit layer) runs on zero-padded kernel / bias
  columns and is sliced back: the kept columns are the same products (each column its own k-ordered
  chain); under autograd the padding is differentiated through (``ag.dense``)."""
  n = len(mlp)
  for i, (k, b) in enumerate(mlp):
    pad = (-k.shape[1]) % 4
    if pad:
      k = torch.nn.functional.pad(k, (0, pad))
      b = torch.nn.functional.pad(b, (0, pad))
    fn = ag.dense if base.needs_grad(x, k, b) else ops.dense
    x = fn(x, k, b, relu=i + 1 < n)
    if pad:
      x = x[..., :k.shape[1] - pad]
  return x


class OccupancyNet(base.Module):
  """occupancy_net.py:66-125.  ``train_encoder``: an encoder parameter that requires grad is trained
  through the occupancy head (the gather's VJP) instead of raising."""

  def __init__(self, config, grid, dtype=torch.float32, train_encoder=False):
    self.config = config
    self.grid = grid
    self.dtype = dtype
    self.train_encoder = bool(train_encoder)
    self.streetview_encoder = streetview_encoder.StreetViewEncoder(config.streetview_encoder, dtype)
    self.feature_dim = int(config.streetview_encoder.feature_dim)
    self.mlp_out = layers.MLP(config.occupancy_mlp, in_dim=self.feature_dim)
    widths = tuple(int(w) for w in config.occupancy_mlp.layers)
    if widths[-1] != 1:
      raise ValueError(f'occupancy_mlp.layers must end with width 1 (logits[..., 0]), got {widths}')
    self.hidden = widths[:-1]
    if config.occupancy_mlp.apply_input_activation:
      raise NotImplementedError('occupancy_mlp.apply_input_activation (not used by the reference configs)')

  def init_params(self, gen, device):
    return {'streetview_encoder': self.streetview_encoder.init_params(gen, device),
            'mlp_out': self.mlp_out.init_params(gen, device)}

  def _voxel_centres(self, B, device):
    grid = self.grid
    xyz = base.device_const(('occupancy_voxel_centres', tuple(grid.extent), float(grid.cell_size)), device,
                            lambda: grid.index_to_xyz(grid.grid_index().to(torch.float32)).to(torch.float32),
                            owner=self)
    return xyz.unsqueeze(0).expand(B, *xyz.shape)

  def use_fused_head(self, params, volume=None):
    """The fused query kernel serves the call when nothing needs gradients (neither the MLP nor the
    ``volume``, when given), the engine in force is f32-class and the MLP shape is one the kernel
    takes.  Its hidden products are exact f32 (the f32 Dense engine's k-ordered MFMA chain), so on
    'bf16x3' / 'bf16x6' it is at least as accurate as the split engines it stands in for; 'bf16' /
    'fp16' keep their own arithmetic (producer + Dense)."""
    p = params['mlp_out']
    leaves = [p[f'Dense_{i}'][k] for i in range(len(self.hidden) + 1) for k in ('kernel', 'bias')]
    if volume is not None:
      leaves.append(volume)
    return (not base.needs_grad(*leaves) and ops.precision() in F32_CLASS
            and not self.config.occupancy_mlp.apply_input_activation
            and ops.occupancy_head_supported(self.feature_dim, self.hidden))

  def __call__(self, params, data, train=False, debug=False, rng=None, ctx=None):
    cfg = self.config
    if 'map' in data:
      data = data['map']
    queries = data.get('occupancy_queries')
    rays = data.get('lidar_rays')
    if queries is None and rays is None:
      raise ValueError('No points or rays given in the data dict.')
    enc_params = params['streetview_encoder']
    enc_grad = torch.is_grad_enabled() and any(t.requires_grad for _, t in _leaves(enc_params))
    if enc_grad and not self.train_encoder:
      raise NotImplementedError(
          'OccupancyNet: this model does not train the StreetView encoder through the occupancy head; '
          "freeze it: trainer.train_step(..., freeze_params_reg_exp='streetview_encoder/'), or build the "
          'model with train_encoder=True')
    images = data['images']
    B = len(images)
    enc_data = {**data, 'xyz_query': self._voxel_centres(B, images.device)}
    if enc_grad:
      pred = self.streetview_encoder(enc_params, enc_data, train, ctx=ctx)
    else:
      with torch.no_grad():
        pred = self.streetview_encoder(enc_params, enc_data, train, ctx=ctx)
    volume = pred['feature_volume']
    features, vvalid = volume.features.contiguous(), volume.valid.contiguous()
    kw = dict(points=queries.to(torch.float32).contiguous()) if queries is not None else dict(
        rays=(rays['points'].to(torch.float32).contiguous(), rays['origins'].to(torch.float32).contiguous(),
              rays['mask'].to(torch.bool).contiguous()),
        num_samples=int(cfg.num_samples_per_ray), margin=float(cfg.ray_margin))
    cell = float(self.grid.cell_size)
    p = params['mlp_out']
    mlp = [(p[f'Dense_{i}']['kernel'], p[f'Dense_{i}']['bias']) for i in range(len(self.hidden) + 1)]
    # (the fused head reads the volume in 16-byte taps: a contiguous view at an unaligned offset, which
    # .contiguous() leaves as it is, takes the producer, which has a scalar kernel for it)
    if self.use_fused_head(params, features) and features.data_ptr() % 16 == 0:
      logits, valid, samples = ops.occupancy_head(features, vvalid, cell, mlp, **kw)
    else:
      producer = ag.occupancy_ray_features if base.needs_grad(features) else ops.occupancy_ray_features
      feats, valid, samples = producer(features, vvalid, cell, **kw)
      logits = dense_chain(mlp, feats)[..., 0].reshape(valid.shape)
    logits = logits.to(torch.float32)
    if samples is not None:
      pred['ray_samples'] = types.LidarRaySamples(points=samples[0], labels=samples[1], valid=samples[2])
    pred['occupancy'] = types.OccupancySamples(values=torch.sigmoid(logits), valid=valid, logits=logits)
    return pred

  default_config = staticmethod(default_configs.occupancy_net)


def _leaves(tree, prefix=''):
  from snap_amd import dist
  return dist.flatten_tree(tree, prefix)


class OccupancyNetModel(base.BaseModel):
  """Trainer-facing wrapper (occupancy_net.py:128-166)."""

  def __init__(self, config, dataset_meta_data, dtype=torch.float32, engine=None, train_encoder=False):
    self.train_encoder = bool(train_encoder)
    super().__init__(config, dataset_meta_data, dtype=dtype, engine=engine)

  def build_flax_model(self):
    return OccupancyNet(self.config, self.dataset_meta_data['grid'], self.dtype, train_encoder=self.train_encoder)

  @classmethod
  def default_flax_model_config(cls):
    return default_configs.occupancy_net()

  def loss_metrics_function(self, pred, data, model_params=None):
    labels = pred['ray_samples'].labels
    logits = pred['occupancy'].logits
    occ = logits > 0
    # the loss and metrics only on points visible by at least one view
    mask = pred['occupancy'].valid & pred['ray_samples'].valid
    ls = torch.nn.functional.logsigmoid
    bce_per_sample = -torch.where(labels, ls(logits), ls(-logits))
    bce_pos = masked_mean(bce_per_sample, mask & labels, 1)
    bce_neg = masked_mean(bce_per_sample, mask & ~labels, 1)
    bce = (bce_pos + bce_neg) / 2
    losses = {'occupancy_bce': bce, 'total': bce}
    correct = (occ == labels).to(logits.dtype)
    metrics = {
        'occupancy/accuracy': masked_mean(correct, mask, 1),
        'occupancy/recall': masked_mean(correct, mask & labels, 1),
        # (the reference's name: the true-negative rate over the negatives)
        'occupancy/precision': masked_mean(correct, mask & ~labels, 1),
    }
    return losses, metrics
