"""`-m gpu` checks of the OccupancyNet query kernels (occupancy.hip), the module and its frozen-encoder
training path, against the reference chain of occupancy_reference.py."""
import copy

import numpy as np
import pytest
import torch

import helpers
import occupancy_reference as occ_ref
from oracle import grids as o_grids
from snap_amd import models
from snap_amd import ops
from snap_amd import trainer
from snap_amd.configs import defaults
from snap_amd.data import synthetic
from snap_amd.models import occupancy_net

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
CELL = 0.2


def _volume(B, X, Y, Z, D, seed, invalid=0.15):
  g = torch.Generator(device='cpu').manual_seed(seed)
  vol = (torch.rand((B, X, Y, Z, D), generator=g) * 2 - 1).to(DEV)
  valid = (torch.rand((B, X, Y, Z), generator=g) >= invalid).to(DEV)
  return vol, valid


def _rays(B, N, extent, seed, pad=0.1):
  """Origins inside the grid, hits up to 1.5 x the extent away (many outside), ~10 % padding rays."""
  rng = np.random.default_rng(seed)
  ext = np.asarray(extent, np.float32) * CELL
  origins = rng.uniform(0.1, 0.9, (B, N, 3)).astype(np.float32) * ext
  d = rng.normal(size=(B, N, 3))
  d /= np.linalg.norm(d, axis=-1, keepdims=True)
  hits = (origins + d * rng.uniform(0.3, 1.5, (B, N, 1)) * ext.max()).astype(np.float32)
  hits[:, :3] = origins[:, :3] + np.float32(0.5) * np.array([1, 0, 0], np.float32)   # short rays: the clip
  mask = rng.random((B, N)) >= pad
  hits = np.where(mask[..., None], hits, 0).astype(np.float32)
  origins = np.where(mask[..., None], origins, 0).astype(np.float32)
  return tuple(torch.from_numpy(a).to(DEV) for a in (hits, origins, mask))


def _mlp_params(D, layers, seed):
  g = torch.Generator(device='cpu').manual_seed(seed)
  out, d_in = [], D
  for w in layers:
    lim = (6.0 / (d_in + w)) ** 0.5
    out.append(((torch.rand((d_in, w), generator=g) * 2 - 1) * lim * 2, torch.rand(w, generator=g) * 0.2 - 0.1))
    d_in = w
  return [(k.to(DEV), b.to(DEV)) for k, b in out]


def _unfused(feats, mlp):
  """producer rows -> the Dense chain of the fallback path on the exact f32 engine.  Split-K off: on
  the small test shapes the engine would split the K = 256 logit layer in two partial chains (a
  different summation order); at the workload's row counts it never does."""
  with ops.engine_scope('f32'), ops.tuning_scope(USE_SPLITK=False):
    return occupancy_net.dense_chain(mlp, feats)[..., 0]


def _assert_close_to_unfused(fused, unfused):
  """Fused head vs the f32 Dense chain: both exact-f32 MFMA products with a bias(-ReLU) epilogue, but not
  bitwise the same order (the engine's slab staging; the fused width-1 layer is a plain fmaf chain)."""
  err = float((fused - unfused).abs().max())
  assert err <= 2e-6 * float(unfused.abs().max()), err


def _ref_logits(feats, mlp):
  """f64 MLP on the (bitwise-checked) producer rows."""
  x = feats.double()
  for i, (k, b) in enumerate(mlp):
    x = x @ k.double() + b.double()
    if i + 1 < len(mlp):
      x = torch.relu(x)
  return x[..., 0]


@pytest.mark.parametrize('S', [1, 2, 7])
def test_producer_points_features_and_validity(S):
  B, X, Y, Z, D = 2, 20, 24, 10, 64
  vol, vvalid = _volume(B, X, Y, Z, D, seed=S)
  hits, origins, mask = _rays(B, 300, (X, Y, Z), seed=10 + S)
  feats, valid, (pts, labels, rvalid) = ops.occupancy_ray_features(
      vol, vvalid, CELL, rays=(hits, origins, mask), num_samples=S, margin=0.2)
  torch.cuda.synchronize()
  r_pts, r_labels, r_valid = occ_ref.sample_rays_f32(hits.cpu().numpy(), origins.cpu().numpy(),
                                                     mask.cpu().numpy(), S, 0.2)
  np.testing.assert_array_equal(pts.cpu().numpy(), r_pts)               # bitwise: the host f32 restatement
  np.testing.assert_array_equal(labels.cpu().numpy(), r_labels)
  np.testing.assert_array_equal(rvalid.cpu().numpy(), r_valid)
  feats = feats.reshape(B, -1, D)
  vol_np, vv_np = vol.cpu().numpy(), vvalid.cpu().numpy()
  for b in range(B):
    idx = torch.from_numpy(r_pts[b] / np.float32(CELL)).to(DEV)
    f_i, v_i = ops.interpolate_nd(vol[b].contiguous(), idx, vvalid[b].contiguous())
    assert torch.equal(feats[b], f_i)                                     # bitwise: ops.interpolate_nd
    assert torch.equal(valid[b], v_i)
    _, v_ref = o_grids.interpolate_nd(vol_np[b], r_pts[b] / np.float32(CELL), vv_np[b])
    np.testing.assert_array_equal(valid[b].cpu().numpy(), v_ref)
  v = valid.cpu().numpy()
  assert 0.1 < v.mean() < 0.9                                             # both kinds exercised


@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('layers', [(128, 1), (128, 256, 1)])
@pytest.mark.parametrize('S', [1, 2, 7, 100, 'queries'])
def test_fused_head_against_reference_and_unfused(D, layers, S):
  B, X, Y, Z = 2, 24, 20, 12
  vol, vvalid = _volume(B, X, Y, Z, D, seed=D + len(layers))
  if S == 'queries':
    g = torch.Generator(device='cpu').manual_seed(7)
    q = (torch.rand((B, 5000, 3), generator=g) * 1.2 - 0.1) * torch.tensor([X, Y, Z]) * CELL
    kw = dict(points=q.to(DEV).contiguous())
  else:
    kw = dict(rays=_rays(B, 20000 // S if S > 2 else 3000, (X, Y, Z), seed=S), num_samples=S, margin=0.2)
  mlp = _mlp_params(D, layers, seed=3)
  assert ops.occupancy_head_supported(D, layers[:-1])
  logits, valid, samples = ops.occupancy_head(vol, vvalid, CELL, mlp, **kw)
  feats, valid_p, samples_p = ops.occupancy_ray_features(vol, vvalid, CELL, **kw)
  unfused = _unfused(feats, mlp).reshape(valid.shape)
  ref = _ref_logits(feats, mlp).reshape(valid.shape)
  torch.cuda.synchronize()
  assert torch.equal(valid, valid_p)
  if samples is not None:
    for a, b in zip(samples, samples_p):
      assert torch.equal(a, b)
  scale = float(ref.abs().max())
  err = float((logits.double() - ref).abs().max())
  assert err <= 1e-5 * scale + 1e-6, (err, scale)
  _assert_close_to_unfused(logits, unfused)


def test_full_size_fused_equals_unfused_and_repeats():
  B, X, Y, Z, D, N, S = 1, 120, 160, 60, 128, 10_000, 100
  vol, vvalid = _volume(B, X, Y, Z, D, seed=1)
  rays = _rays(B, N, (X, Y, Z), seed=2)
  kw = dict(rays=rays, num_samples=S, margin=0.2)
  for layers in ((128, 1), (128, 256, 1)):
    mlp = _mlp_params(D, layers, seed=4)
    l1, v1, _ = ops.occupancy_head(vol, vvalid, CELL, mlp, want_samples=False, **kw)
    l2, v2, _ = ops.occupancy_head(vol, vvalid, CELL, mlp, want_samples=False, **kw)
    feats, vp, _ = ops.occupancy_ray_features(vol, vvalid, CELL, want_samples=False, **kw)
    unfused = _unfused(feats, mlp).reshape(l1.shape)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(v1, v2)                    # bitwise repeatable
    assert torch.equal(v1, vp)
    _assert_close_to_unfused(l1, unfused)
    del feats, unfused
  # shapes the fused kernel does not take: the producer + Dense chain serves them
  assert not ops.occupancy_head_supported(D, (48,))
  assert not ops.occupancy_head_supported(D, (128, 128, 128))
  for layers in ((48, 1), (64, 64, 64, 1)):
    mlp = _mlp_params(D, layers, seed=5)
    feats, vp, _ = ops.occupancy_ray_features(vol, vvalid, CELL, want_samples=False, **kw)
    got = _unfused(feats, mlp)
    rows = torch.arange(0, feats.shape[0], 997, device=DEV)
    ref = _ref_logits(feats[rows], mlp)
    assert float((got[rows].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6
    del feats


def _tiny(layers=(32, 1), S=5, feature_dim=32, dtype=torch.float32, engine=None):
  sv = helpers.tiny_localizer_config(aerial=False, feature_dim=feature_dim).bev_mapper.streetview_encoder
  cfg = defaults.occupancy_net()
  cfg.streetview_encoder = copy.deepcopy(sv)
  cfg.occupancy_mlp.layers = tuple(layers)
  cfg.num_samples_per_ray = S
  meta = synthetic.meta_data(0.2, (3.2, 3.2, 1.6))
  return cfg, meta, occupancy_net.OccupancyNetModel(cfg, meta, dtype=dtype, engine=engine)


@pytest.mark.parametrize('engine', ['f32', 'bf16x3'])
@pytest.mark.parametrize('layers', [(32, 1), (32, 64, 1), (48, 1)])
def test_module_forward_against_reference_chain(engine, layers):
  cfg, meta, model = _tiny(layers=layers, engine=engine)
  net = model.flax_model
  variables = net.init(0, device='cpu')
  batch = synthetic.make_batch(2, meta['grid'], 2, (64, 64), seed=3, with_aerial=False, lidar_rays=400)
  params = helpers.params_to_device(variables['params'], DEV)
  with torch.no_grad():
    with ops.engine_scope(engine):
      assert net.use_fused_head(params) == (layers != (48, 1))
    pred = net.apply({'params': params}, helpers.batch_to_device(batch, DEV))
  data = helpers.scene_to_oracle(batch['map'])
  data['lidar_rays'] = {k: v.numpy() for k, v in batch['map']['lidar_rays'].items()}
  ref = occ_ref.occupancy_net(helpers.params_to_numpy(variables['params']), cfg, meta['grid'], data)
  vol, rvol = pred['feature_volume'], ref['feature_volume']
  grid = meta['grid']
  X, Y, Z = grid.extent
  idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij'), -1)
  xyz = np.broadcast_to(((idx + 0.5) * grid.cell_size).astype(np.float32), (2, X, Y, Z, 3))
  helpers.assert_validity_mismatches_on_borders('volume valid', vol.valid, rvol['valid'], data, xyz,
                                                _stride(pred))
  both = vol.valid.cpu().numpy() & rvol['valid']
  rng = float(np.abs(rvol['features']).max())
  assert float(np.abs(vol.features.cpu().numpy() - rvol['features'])[both].max()) <= 1e-3 * rng
  np.testing.assert_array_equal(pred['ray_samples'].points.cpu().numpy(), ref['ray_samples']['points'])
  ov, rv = pred['occupancy'].valid.cpu().numpy(), ref['occupancy']['valid']
  agree = ov & rv
  assert agree.sum() >= 100
  lg, rl = pred['occupancy'].logits.cpu().numpy(), ref['occupancy']['logits']
  assert float(np.abs(lg - rl)[agree].max()) <= 1e-3 * float(np.abs(rl).max())


def _stride(pred):
  s = pred['image_feature_pyramid'].strides[-1]
  s = np.asarray(s.cpu() if hasattr(s, 'cpu') else s).reshape(-1)
  return (float(s[0]), float(s[1]))


def _train_setup(dtype=torch.float32, seed=0):
  cfg, meta, model = _tiny(layers=(32, 64, 1), S=8, dtype=dtype)
  variables = model.flax_model.init(seed, device='cpu')
  params = helpers.params_to_device(variables['params'], DEV)
  batch = helpers.batch_to_device(
      synthetic.make_batch(1, meta['grid'], 2, (64, 64), seed=seed + 1, with_aerial=False, lidar_rays=500), DEV)
  return model, params, batch


def _run(steps, dtype=torch.float32, ds=None):
  model, params, batch = _train_setup(dtype)
  state = trainer.TrainState.create(params, dynamic_scale=ds)
  init = {n: t.clone() for n, t in trainer.flatten_params(params)}
  logs = []
  for _ in range(steps):
    state, _, lg = trainer.train_step(state, batch, model=model, lr_fn=lambda s: 3e-3,
                                      freeze_params_reg_exp='streetview_encoder/')
    logs.append(lg)
  return state, init, logs


def test_frozen_encoder_training():
  state, init, logs = _run(3)
  names = [n for n, _ in trainer.flatten_params(state.params)]
  cur = dict(trainer.flatten_params(state.params))
  assert any(n.startswith('streetview_encoder/') for n in names)
  for i, n in enumerate(names):
    if n.startswith('streetview_encoder/'):
      assert torch.equal(cur[n], init[n]), n
      assert not state.m[i].any() and not state.v[i].any(), n
    else:
      assert not torch.equal(cur[n], init[n]), n
  assert all(lg['is_finite'] for lg in logs)
  assert logs[-1]['loss'] < logs[0]['loss'], [lg['loss'] for lg in logs]
  state2, _, logs2 = _run(3)
  for (n, a), (_, b) in zip(trainer.flatten_params(state.params), trainer.flatten_params(state2.params)):
    assert torch.equal(a, b), n
  assert [lg['loss'] for lg in logs] == [lg['loss'] for lg in logs2]


def test_frozen_encoder_head_gradients_match_fp64():
  model, params, batch = _train_setup()
  net = model.flax_model
  with torch.no_grad():
    pred = net.apply({'params': params}, batch)
  vol = pred['feature_volume']
  rays = batch['map']['lidar_rays']
  feats, valid, samples = ops.occupancy_ray_features(
      vol.features.contiguous(), vol.valid.contiguous(), CELL, rays=(rays['points'], rays['origins'], rays['mask']),
      num_samples=8, margin=0.2)
  p = params['mlp_out']
  leaves = [p[f'Dense_{i}'][k] for i in range(3) for k in ('kernel', 'bias')]
  for t in leaves:
    t.requires_grad_(True)

  def loss_of(logits):
    fake = {'ray_samples': occupancy_net.types.LidarRaySamples(*samples),
            'occupancy': occupancy_net.types.OccupancySamples(torch.sigmoid(logits), valid, logits)}
    return model.loss_metrics_function(fake, batch)[0]['total'].sum()

  logits = occupancy_net.dense_chain([(leaves[2 * i], leaves[2 * i + 1]) for i in range(3)], feats)
  logits = logits[..., 0].reshape(valid.shape)
  grads = torch.autograd.grad(loss_of(logits), leaves)
  for t in leaves:
    t.requires_grad_(False)
  p64 = [t.detach().double().requires_grad_(True) for t in leaves]
  x = feats.double()
  for i in range(3):
    x = x @ p64[2 * i] + p64[2 * i + 1]
    if i < 2:
      x = torch.relu(x)
  ref = torch.autograd.grad(loss_of(x[..., 0].reshape(valid.shape)), p64)
  for g, r in zip(grads, ref):
    scale = float(r.abs().max())
    assert float((g.double() - r).abs().max()) <= 2e-5 * scale + 1e-9


def test_fp16_dynamic_scale_step_is_finite():
  state, _, logs = _run(1, dtype=torch.float16, ds=trainer.DynamicScale(minimum_scale=256))
  assert np.isfinite(logs[0]['loss']) and np.isfinite(logs[0]['l2_grads'])


def test_unfrozen_training_raises():
  model, params, batch = _train_setup()
  state = trainer.TrainState.create(params)
  with pytest.raises(NotImplementedError, match='streetview_encoder/'):
    trainer.train_step(state, batch, model=model, lr_fn=lambda s: 1e-3)


def test_freeze_none_is_the_plain_step_on_the_localizer():
  cfg = helpers.tiny_localizer_config(num_pose_samples=48, retries=2)
  meta = synthetic.meta_data(0.2, (6.4, 6.4, 12))
  model = models.get_model('bev_localizer')(cfg, meta)
  variables = model.flax_model.init(0, device='cpu')
  batch = helpers.batch_to_device(synthetic.make_batch(2, meta['grid'], 3, (64, 64), seed=1), DEV)
  out = []
  for kw in ({}, {'freeze_params_reg_exp': None}):
    state = trainer.TrainState.create(helpers.params_to_device(variables['params'], DEV))
    state, _, logs = trainer.train_step(state, batch, model=model, lr_fn=lambda s: 1e-3, **kw)
    out.append((state, logs))
  (s0, l0), (s1, l1) = out
  for (n, a), (_, b) in zip(trainer.flatten_params(s0.params), trainer.flatten_params(s1.params)):
    assert torch.equal(a, b), n
  for a, b in zip(s0.m + s0.v, s1.m + s1.v):
    assert torch.equal(a, b)
  assert l0['loss'] == l1['loss'] and l0['l2_grads'] == l1['l2_grads']
