"""`-m gpu` checks of the OccupancyNet query kernels (occupancy.hip), the module and its frozen-encoder
training path, against the reference chain of occupancy_reference.py."""
import copy

import numpy as np
import pytest
import torch

import helpers
import occupancy_reference as occ_ref
from oracle import encoder as o_enc
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


# (D, hidden widths) of the bitwise head tests: every LDS layout of snap_occupancy_head_f32 (small A +
# small H: D, h1 <= 128; wide A: D > 128, h1 <= 128; wide H: h1 > 128), each with one and two hidden layers
HEAD_SHAPES = [(32, (32,)), (32, (256,)), (96, (96, 32)), (128, (128,)), (128, (128, 256)), (160, (64,)),
               (160, (96, 160)), (256, (256,)), (256, (256, 256)), (64, (160, 32)), (128, (224,))]


def _fused_cases():
  """(D, layers, S) of test_fused_head_against_reference_and_unfused: the original D x MLP x S product (ids
  kept) and HEAD_SHAPES with rays (S = 7) and explicit queries."""
  cases = [pytest.param(D, layers, S, id=f'{S}-layers{li}-{D}')
           for D in (64, 128) for li, layers in enumerate(((128, 1), (128, 256, 1))) for S in (1, 2, 7, 100, 'queries')]
  for D, hidden in HEAD_SHAPES:
    for S in (7, 'queries'):
      cases.append(pytest.param(D, (*hidden, 1), S, id=f'{S}-{"x".join(map(str, hidden))}-{D}'))
  return cases


@pytest.mark.parametrize('D,layers,S', _fused_cases())
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


# -- exact host restatement (occupancy_reference.fmaf32 / gather_f32 / head_f32) --------------------
def _np_mlp(mlp):
  return [(k.cpu().numpy(), b.cpu().numpy()) for k, b in mlp]


def _assert_bits_equal(got, want, what):
  """f32 arrays equal bit for bit; NaN positions must agree (their payloads are not compared)."""
  got = np.asarray(got, np.float32)
  want = np.asarray(want, np.float32)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  nan_g, nan_w = np.isnan(got), np.isnan(want)
  np.testing.assert_array_equal(nan_g, nan_w, err_msg=what)
  g = np.where(nan_g, np.float32(0), got).view(np.uint32)
  w = np.where(nan_w, np.float32(0), want).view(np.uint32)
  bad = g != w
  assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def _host_head(vol, vvalid, mlp, kw, cell=CELL):
  """The restatement of one ops.occupancy_head call -> (points, features, valid, logits [B, P])."""
  vol_np = vol.cpu().numpy()
  vv_np = None if vvalid is None else vvalid.cpu().numpy().astype(bool)
  if 'rays' in kw:
    hits, origins, mask = (t.cpu().numpy() for t in kw['rays'])
    pts, _, _ = occ_ref.sample_rays_f32(hits, origins, mask, kw['num_samples'], kw['margin'])
  else:
    pts = kw['points'].cpu().numpy()
  feats, valid = occ_ref.gather_f32(vol_np, vv_np, pts, cell)
  logits = occ_ref.head_f32(feats.reshape(-1, feats.shape[-1]), _np_mlp(mlp)).reshape(valid.shape)
  return pts, feats, valid, logits


def test_head_shapes_reach_every_layout():
  """The bitwise shape matrix runs all three LDS layouts of the dispatch, each with one and two hidden layers."""
  for D, hidden in HEAD_SHAPES:
    assert occ_ref.occupancy_head_supported(D, hidden) and ops.occupancy_head_supported(D, hidden)
  got = {(occ_ref.head_layout(D, hidden[0]), len(hidden)) for D, hidden in HEAD_SHAPES}
  assert got == {(lay, n) for lay in ('small', 'wide_a', 'wide_ah') for n in (1, 2)}, got


@pytest.mark.parametrize('source', ['rays', 'queries'])
@pytest.mark.parametrize('D,hidden', HEAD_SHAPES, ids=[f'{D}-{"x".join(map(str, h))}' for D, h in HEAD_SHAPES])
def test_fused_head_bitwise_against_host_restatement(D, hidden, source):
  """Logits bit for bit, validity and samples exactly, against head_f32(gather_f32(sample_rays_f32(...))):
  two scenes with their own volumes, row counts that leave partial workgroups (rays: 2 x 5 x 61 = 610
  or 2 x 5 x 23 = 230 rows; queries: P = 1, 23, 130 or 300 per scene), volume_valid given or None."""
  i = HEAD_SHAPES.index((D, hidden))
  B, X, Y, Z = 2, 13, 11, 7
  vol, vvalid = _volume(B, X, Y, Z, D, seed=100 + i)
  if i % 3 == 0:
    vvalid = None
  wide = max(D, *hidden) > 160                    # (the host's fmaf chains: fewer rows at the widest MLPs)
  if source == 'rays':
    kw = dict(rays=_rays(B, 23 if wide else 61, (X, Y, Z), seed=200 + i), num_samples=5, margin=0.2)
  else:
    P = (1, 23, 130 if wide else 300)[i % 3]
    g = torch.Generator(device='cpu').manual_seed(300 + i)
    q = (torch.rand((B, P, 3), generator=g) * 1.2 - 0.1) * torch.tensor([X, Y, Z]) * CELL
    kw = dict(points=q.to(DEV).contiguous())
  mlp = _mlp_params(D, (*hidden, 1), seed=400 + i)
  logits, valid, samples = ops.occupancy_head(vol, vvalid, CELL, mlp, **kw)
  torch.cuda.synchronize()
  pts, _, r_valid, r_logits = _host_head(vol, vvalid, mlp, kw)
  np.testing.assert_array_equal(valid.cpu().numpy(), r_valid)
  if samples is not None:
    np.testing.assert_array_equal(samples[0].cpu().numpy(), pts)
  _assert_bits_equal(logits.cpu().numpy(), r_logits, f'logits D={D} hidden={hidden} {source}')


def _producer_vs_host(vol, vvalid, kw, cell=CELL):
  """ops.occupancy_ray_features: features bit for bit (NaN positions included), validity and sample points
  exactly, against gather_f32 on sample_rays_f32's points -> (features, valid)."""
  feats, valid, samples = ops.occupancy_ray_features(vol, vvalid, cell, **kw)
  torch.cuda.synchronize()
  vol_np = vol.cpu().numpy()
  vv_np = None if vvalid is None else vvalid.cpu().numpy().astype(bool)
  if 'rays' in kw:
    hits, origins, mask = (t.cpu().numpy() for t in kw['rays'])
    pts, _, _ = occ_ref.sample_rays_f32(hits, origins, mask, kw['num_samples'], kw['margin'])
    np.testing.assert_array_equal(samples[0].cpu().numpy(), pts)
  else:
    pts = kw['points'].cpu().numpy()
  r_feats, r_valid = occ_ref.gather_f32(vol_np, vv_np, pts, cell)
  _assert_bits_equal(feats.cpu().numpy(), r_feats.reshape(feats.shape), 'producer features')
  np.testing.assert_array_equal(valid.cpu().numpy(), r_valid)
  return feats, valid


def _head_vs_host(vol, vvalid, mlp, kw, cell=CELL):
  logits, valid, _ = ops.occupancy_head(vol, vvalid, cell, mlp, **kw)
  torch.cuda.synchronize()
  _, _, r_valid, r_logits = _host_head(vol, vvalid, mlp, kw, cell)
  np.testing.assert_array_equal(valid.cpu().numpy(), r_valid)
  _assert_bits_equal(logits.cpu().numpy(), r_logits, 'head logits')
  return logits, valid


@pytest.mark.parametrize('D', [1, 3, 6, 33, 130, 'offset64'])
def test_scalar_producer_bitwise(D):
  """occ_features_kernel<1>: taken for D % 4 != 0 and for a volume that is not 16-byte aligned (here a
  contiguous view at a 1-float storage offset).  Bitwise against gather_f32, and the offset volume
  against the vector kernel on an aligned copy; the fused head refuses the unaligned volume."""
  B, X, Y, Z = 2, 9, 8, 5
  d = 64 if D == 'offset64' else D
  vol, vvalid = _volume(B, X, Y, Z, d, seed=500 + d)
  if D == 'offset64':
    buf = torch.empty(vol.numel() + 1, dtype=torch.float32, device=DEV)
    vol_u = buf[1:].view(vol.shape)
    vol_u.copy_(vol)
    assert vol_u.is_contiguous() and vol_u.data_ptr() % 16 != 0 and vol.data_ptr() % 16 == 0
  else:
    vol_u = vol
  kw = dict(rays=_rays(B, 50, (X, Y, Z), seed=600 + d), num_samples=3, margin=0.2)
  feats, valid = _producer_vs_host(vol_u, vvalid, kw)
  kwq = dict(points=((torch.rand((B, 77, 3), generator=torch.Generator().manual_seed(d)) * 1.2 - 0.1)
                     * torch.tensor([X, Y, Z]) * CELL).to(DEV).contiguous())
  _producer_vs_host(vol_u, vvalid, kwq)
  if D == 'offset64':
    f_vec, v_vec, _ = ops.occupancy_ray_features(vol, vvalid, CELL, **kw)      # the vector kernel
    torch.cuda.synchronize()
    assert torch.equal(feats, f_vec) and torch.equal(valid, v_vec)
    mlp = _mlp_params(d, (64, 1), seed=7)
    with pytest.raises(RuntimeError, match='snap_occupancy_head_f32'):
      ops.occupancy_head(vol_u, vvalid, CELL, mlp, **kw)
    torch.cuda.synchronize()


def test_module_falls_back_to_the_producer_on_an_unaligned_volume():
  """The fused head refuses a volume that is not 16-byte aligned; OccupancyNet must then take the
  producer + Dense path instead of raising (a contiguous volume at an offset survives .contiguous())."""
  cfg, meta, model = _tiny(layers=(32, 1), engine='f32')
  net = model.flax_model
  variables = net.init(0, device='cpu')
  batch = helpers.batch_to_device(
      synthetic.make_batch(1, meta['grid'], 2, (64, 64), seed=3, with_aerial=False, lidar_rays=300), DEV)
  params = helpers.params_to_device(variables['params'], DEV)
  with torch.no_grad():
    ref = net.apply({'params': params}, batch)
  encoder = net.streetview_encoder
  seen = []

  def unaligned_encoder(*args, **kwargs):
    pred = encoder(*args, **kwargs)
    f = pred['feature_volume'].features
    buf = torch.empty(f.numel() + 1, dtype=f.dtype, device=f.device)
    fu = buf[1:].view(f.shape)
    fu.copy_(f)
    seen.append(fu.data_ptr() % 16)
    pred['feature_volume'] = occupancy_net.types.FeatureVolume(features=fu, valid=pred['feature_volume'].valid)
    return pred

  net.streetview_encoder = unaligned_encoder
  try:
    with torch.no_grad():
      got = net.apply({'params': params}, batch)
  finally:
    net.streetview_encoder = encoder
  assert seen and seen[0] != 0
  assert torch.equal(got['occupancy'].valid, ref['occupancy'].valid)
  assert torch.equal(got['ray_samples'].points, ref['ray_samples'].points)
  _assert_close_to_unfused(ref['occupancy'].logits, got['occupancy'].logits)


EDGE_CELL = 0.25          # a power of two: point / cell is exact, so p lands where the test puts it


def test_geometry_edges_bitwise():
  """Points at p = 0, p = size (invalid), the largest f32 below size, p in (-0.5, 0) (invalid, taps clamped),
  voxel centres (whi = 0) and faces (whi = 0.5); an axis of extent 1; an invalid voxel beside a query
  that gives it zero weight.  Producer and head (one and two hidden layers) bitwise against the host."""
  B, X, Y, Z, D = 2, 5, 1, 3, 32
  vol, _ = _volume(B, X, Y, Z, D, seed=700)
  vvalid = torch.ones((B, X, Y, Z), dtype=torch.bool, device=DEV)
  vvalid[0, 3, 0, 1] = False
  below = lambda n: float(np.nextafter(np.float32(n), np.float32(0)))
  p = [[0, 0, 0], [5, 0.5, 1.5], [below(5), 0.5, 1.5], [-0.25, 0.5, 1.5], [-1e-6, 0.5, 1.5], [2.5, 0.5, 1.5],
       [3, 0.5, 1.5], [4.5, 0.5, 0.5], [2.5, 0, 1.5], [2.5, below(1), 1.5], [2.5, 1, 1.5], [1.5, 0.5, below(3)],
       [2.5, 0.5, 1.0], [below(5), below(1), below(3)], [4.0, 0.25, 2.0]]
  pts = np.asarray(p, np.float32) * np.float32(EDGE_CELL)
  pts = np.broadcast_to(pts, (B, *pts.shape)).copy()
  kw = dict(points=torch.from_numpy(pts).to(DEV))
  feats, valid = _producer_vs_host(vol, vvalid, kw, cell=EDGE_CELL)
  v = valid.cpu().numpy()
  assert v[:, 0].all() and not v[:, 1].any() and v[:, 2].all() and not v[:, 3].any() and not v[:, 4].any()
  assert not v[0, 5] and v[1, 5]                         # zero-weight tap on the invalid voxel (3, 0, 1)
  assert not v[:, 10].any() and v[:, 13].all()
  f = feats.reshape(B, -1, D).cpu().numpy()
  np.testing.assert_array_equal(f[1, 5], vol[1, 2, 0, 1].cpu().numpy())   # a centre is the voxel itself
  for hidden in ((32,), (32, 64)):
    _head_vs_host(vol, vvalid, _mlp_params(D, (*hidden, 1), seed=8), kw, cell=EDGE_CELL)
    _head_vs_host(vol, None, _mlp_params(D, (*hidden, 1), seed=9), kw, cell=EDGE_CELL)


@pytest.mark.parametrize('S', [1, 2, 3])
def test_ray_edges_and_non_finite_inputs_bitwise(S):
  """Padding rays (length 0), rays of length exactly 1 and below 1 (the clip), a margin longer than the
  ray (the direction flips), and NaN / +-inf / 1e30 coordinates.  Every tap index is clamped into the
  volume: occ_taps clamps floor(c) to [-1, size] as a float before converting it (this case first ran
  with an integer clamp only, which the compiler rewrote into one that wrapped at lo = +inf / 1e30:
  an illegal address), so these rows read in bounds.  Points equal the restatement (NaN positions included), non-finite rows are
  invalid, and the head's other rows in the same launch are bitwise those of the host."""
  B, X, Y, Z, D = 2, 12, 9, 6, 32
  vol, vvalid = _volume(B, X, Y, Z, D, seed=800 + S, invalid=0.05)
  rng = np.random.default_rng(S)
  N = 40
  o = (rng.uniform(0.2, 0.8, (B, N, 3)) * np.array([X, Y, Z]) * EDGE_CELL).astype(np.float32)
  u = rng.normal(size=(B, N, 3))
  u = u / np.linalg.norm(u, axis=-1, keepdims=True)
  length = rng.uniform(0.05, 2.0, (B, N, 1))
  length[:, :6, 0] = [0, 0, 1, 0.5, 0.1, 0.15]              # length 0 (two), 1, below 1, shorter than the margin
  h = (o + u * length).astype(np.float32)
  h[:, 2] = o[:, 2] + np.float32(1) * np.array([0, 1, 0], np.float32)          # exactly 1 along an axis
  mask = rng.random((B, N)) >= 0.1
  mask[:, 0] = False
  h[:, 0] = o[:, 0] = 0                                       # a padding ray
  bad = [(6, 'h', 0, np.nan), (7, 'o', 1, np.nan), (8, 'h', 2, np.inf), (9, 'h', 0, -np.inf), (10, 'o', 2, np.inf),
         (11, 'h', 1, 1e30), (12, 'o', 0, 1e30), (13, 'h', 0, -1e30)]
  for n, which, axis, val in bad:
    (h if which == 'h' else o)[:, n, axis] = val
  rays = tuple(torch.from_numpy(a).to(DEV) for a in (h, o, mask))
  kw = dict(rays=rays, num_samples=S, margin=0.2)
  feats, valid = _producer_vs_host(vol, vvalid, kw, cell=EDGE_CELL)
  pts, _, _ = occ_ref.sample_rays_f32(h, o, mask, S, 0.2)
  finite = np.isfinite(pts / np.float32(EDGE_CELL)).all(-1)
  assert not finite.all() and np.isnan(pts).any()
  assert not valid.cpu().numpy()[~finite].any()
  feats = feats.reshape(B, -1, D)
  for b in range(B):                   # interpolate_nd_kernel shares the tap set-up: same bits on these points
    f_i, v_i = ops.interpolate_nd(vol[b].contiguous(), torch.from_numpy(pts[b] / np.float32(EDGE_CELL)).to(DEV),
                                  vvalid[b].contiguous())
    torch.cuda.synchronize()
    _assert_bits_equal(f_i.cpu().numpy(), feats[b].cpu().numpy(), 'interpolate_nd')
    assert torch.equal(v_i, valid[b])
  for hidden in ((32,), (64, 32)):
    logits, hv = _head_vs_host(vol, vvalid, _mlp_params(D, (*hidden, 1), seed=10), kw, cell=EDGE_CELL)
    assert torch.equal(hv, valid)
    assert np.isfinite(logits.cpu().numpy()[finite]).all()


class _Planted:
  """A [B, X, Y, Z, ...] array that is zero (or ``fill``) except in one box: what gather_f32 reads of a huge
  volume without the volume existing on the host (it only indexes vol[b, x, y, z] at the taps)."""

  def __init__(self, shape, lo, box, fill=0):
    self.shape, self.lo, self.box, self.fill = shape, lo, box, fill

  def __getitem__(self, idx):
    idx = np.broadcast_arrays(*idx)
    out = np.full(idx[0].shape + self.box.shape[4:], self.fill, self.box.dtype)
    rel = [i - l for i, l in zip(idx, self.lo)]
    inside = np.all([(r >= 0) & (r < n) for r, n in zip(rel, self.box.shape[:4])], 0)
    out[inside] = self.box[tuple(r[inside] for r in rel)]
    return out


def test_scene_offsets_beyond_2_to_31_elements():
  """16 scenes of 120 x 160 x 60 x 128 (9.4 GB): from scene 15 on the scene offset b * X*Y*Z * D exceeds
  2^31 elements (and scene 14's taps above x = 68 do).  The volume is zero except for random voxels
  planted around the queries of the last three scenes; producer and head bitwise at every query."""
  B, X, Y, Z, D = 16, 120, 160, 60, 128
  assert (B - 1) * X * Y * Z * D > 2 ** 31
  lo = (B - 3, 96, 140, 40)
  rng = np.random.default_rng(11)
  box = rng.uniform(-1, 1, (3, 16, 12, 10, D)).astype(np.float32)
  box_valid = rng.random((3, 16, 12, 10)) >= 0.05
  vol = torch.zeros((B, X, Y, Z, D), dtype=torch.float32, device=DEV)
  vvalid = torch.ones((B, X, Y, Z), dtype=torch.bool, device=DEV)
  try:
    sl = (slice(lo[0], lo[0] + 3), slice(lo[1], lo[1] + 16), slice(lo[2], lo[2] + 12), slice(lo[3], lo[3] + 10))
    vol[sl] = torch.from_numpy(box).to(DEV)
    vvalid[sl] = torch.from_numpy(box_valid).to(DEV)
    P = 40
    q = rng.uniform(0, 1, (B, P, 3)) * np.array([14, 10, 8]) + np.array(lo[1:]) + 1    # inside the box, taps too
    pts = (q * CELL).astype(np.float32)
    kw = dict(points=torch.from_numpy(pts).to(DEV))
    feats, valid, _ = ops.occupancy_ray_features(vol, vvalid, CELL, **kw)
    mlp = _mlp_params(D, (128, 256, 1), seed=12)
    logits, hvalid, _ = ops.occupancy_head(vol, vvalid, CELL, mlp, **kw)
    torch.cuda.synchronize()
    feats, valid, logits, hvalid = (t.cpu().numpy() for t in (feats, valid, logits, hvalid))
  finally:
    del vol, vvalid
    torch.cuda.empty_cache()
  host_vol = _Planted((B, X, Y, Z, D), lo, box)
  host_valid = _Planted((B, X, Y, Z), lo, box_valid, fill=True)
  r_feats, r_valid = occ_ref.gather_f32(host_vol, host_valid, pts, CELL)
  _assert_bits_equal(feats, r_feats.reshape(feats.shape), 'features')
  np.testing.assert_array_equal(valid, r_valid)
  np.testing.assert_array_equal(hvalid, r_valid)
  assert np.abs(r_feats[-1]).min() > 0 and 0.3 < r_valid.mean() < 1     # the planted voxels were read
  r_logits = occ_ref.head_f32(r_feats.reshape(-1, D), _np_mlp(mlp)).reshape(B, P)
  _assert_bits_equal(logits, r_logits, 'logits')


@pytest.mark.parametrize('engine', ['bf16', 'fp16'])
def test_dense_chain_on_the_half_engines(engine):
  """dense_chain with the train config's (128, 256, 1) MLP on producer rows, on the bf16 / IEEE-half
  engines, against the rounded-operand restatement (each layer's input and kernel rounded to the half
  type, float64 products, f32 bias, ReLU) -- layer by layer on the engine's own previous output, so a
  rounding flip of the half conversion cannot cascade.  Tolerance class of test_conv_fp16_plain."""
  B, X, Y, Z, D = 2, 24, 20, 12, 128
  vol, vvalid = _volume(B, X, Y, Z, D, seed=900)
  feats, _, _ = ops.occupancy_ray_features(vol, vvalid, CELL, rays=_rays(B, 400, (X, Y, Z), seed=901),
                                           num_samples=8, margin=0.2, want_samples=False)
  mlp = _mlp_params(D, (128, 256, 1), seed=902)
  rnd = o_enc.fp16_round if engine == 'fp16' else o_enc.bf16_round
  with ops.engine_scope(engine):
    outs = [occupancy_net.dense_chain(mlp[:n], feats) for n in (1, 2, 3)]
  with ops.engine_scope('f32'):
    exact = occupancy_net.dense_chain(mlp, feats)
  torch.cuda.synchronize()
  x = feats.cpu().numpy()
  for n, (out, (k, b)) in enumerate(zip(outs, mlp)):
    want = (rnd(x).astype(np.float64) @ rnd(k.cpu().numpy()).astype(np.float64)
            + b.cpu().numpy().astype(np.float64))
    helpers.report(f'dense_chain {engine} layer {n}', out, want, atol=3e-5, rtol=1e-5)
    x = np.maximum(out.cpu().numpy(), 0)
  assert outs[-1].shape == (B * 400 * 8, 1)
  e_half = float((outs[-1] - exact).abs().max())
  assert e_half > 1e-5                                                # the half engine really ran


def _mlp_grads_after_one_step(dtype, ds):
  """One frozen-encoder train_step of the (32, 64, 1) tiny model built with ``dtype`` -> (loss, the MLP's
  gradient: Adam's first moment after one step is (1 - b1) * g, scaled back)."""
  state, _, logs = _run(1, dtype=dtype, ds=ds)
  names = [n for n, _ in trainer.flatten_params(state.params)]
  g = torch.cat([state.m[i].reshape(-1) for i, n in enumerate(names) if n.startswith('mlp_out/')])
  assert logs[0]['is_finite']
  return logs[0]['loss'], g.double() / (1 - trainer.ADAM_B1)


def test_half_precision_training_step_tracks_f32():
  """A frozen-encoder OccupancyNet step on the half engines vs the f32 step, with the thresholds of
  test_bf16_training_precision_tracks_f32 (loss within 2 %, cosine of the MLP gradients > 0.98, norm
  ratio in (0.9, 1.1)): bfloat16, and float16 under DynamicScale (train_occupancy's dtype_str).
  Observed on an MI355X: bfloat16 loss 1.8e-4 relative from f32, cosine 0.99978, norm ratio 0.9922;
  float16 3.3e-5, 0.999999, 1.0003."""
  l32, g32 = _mlp_grads_after_one_step(torch.float32, None)
  for dtype_str in ('bfloat16', 'float16'):
    dtype, ds = trainer.dtype_and_dynamic_scale(dtype_str)
    assert (ds is not None) == (dtype_str == 'float16')
    l16, g16 = _mlp_grads_after_one_step(dtype, ds)
    cos = float(torch.dot(g32, g16) / (g32.norm() * g16.norm()))
    ratio = float(g16.norm() / g32.norm())
    assert l16 != l32                                                  # the half engines really ran
    assert abs(l16 - l32) <= 2e-2 * abs(l32) + 1e-3, (dtype_str, l32, l16)
    assert cos > 0.98 and 0.9 < ratio < 1.1, (dtype_str, cos, ratio)
