"""Tool (not product): the OccupancyNet query chain on the lidar training workload -- one scene, a
120 x 160 x 60 x 128 f32 volume, 10 000 rays x 100 samples -- fused (ops.occupancy_head, one launch)
against the unfused chain (ops.occupancy_ray_features + one ops.dense per layer on the exact f32
engine), alternating A / B in one process with device events.  Prints one JSON line per MLP shape.

  python tools/occupancy_bench.py [--reps 15] [--warmup 3] [--out FILE]
  python tools/occupancy_bench.py --vjp [--out FILE]     the gather VJP leg (below)

Floor = max(algorithmic FLOP / 157 TFLOP/s (f32 MFMA), compulsory bytes / 8 TB/s); compulsory bytes =
the distinct 512-byte voxel rows the 8 taps of all samples touch (counted on the host) + the volume
validity bytes of those voxels + the outputs.  Intermediate bytes avoided = what the unfused chain
writes and re-reads: the [P, 128] feature rows and every hidden activation.

--vjp: the producer's VJP into the volume (ops_bwd.occupancy_ray_features_vjp) on the same volume and rays,
alternating with the producer forward; the record histogram (records per touched voxel, host sampler);
essential bytes = the record keys + weights written and read back (8 B each way), the gathered d_features
row of every record, and the d_volume write; and one train_step of a small OccupancyNet with the encoder
frozen vs trained through the head (train_encoder=True).  The per-kernel split comes from running this
leg under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from snap_amd import ops  # noqa: E402
from snap_amd.models import occupancy_net  # noqa: E402

PEAK_F32_MFMA = 157e12
PEAK_HBM = 8e12
X, Y, Z, D, N, S, CELL = 120, 160, 60, 128, 10_000, 100, 0.2


def rays(seed=2):
  """Rays of a street scene: origins near the grid centre at ~2 m, hits up to ~30 m away, some outside."""
  rng = np.random.default_rng(seed)
  ext = np.array([X, Y, Z], np.float32) * CELL
  origins = (ext * np.array([0.5, 0.5, 0.0]) + rng.normal(0, 2.0, (1, N, 3)) * [1, 1, 0] + [0, 0, 2.0])
  az = rng.uniform(0, 2 * np.pi, (1, N))
  el = rng.uniform(-0.5, 0.2, (1, N))
  d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
  hits = origins + d * rng.uniform(2.0, 30.0, (1, N, 1))
  mask = rng.random((1, N)) >= 0.1
  hits = np.where(mask[..., None], hits, 0).astype(np.float32)
  origins = np.where(mask[..., None], origins, 0).astype(np.float32)
  return hits, origins, mask


def compulsory_rows(points):
  """Distinct voxel rows the eight taps of every sample read (the kernels' clamped tap indices)."""
  p = points.reshape(-1, 3) / np.float32(CELL)
  c = p - np.float32(0.5)
  lo = np.floor(c).astype(np.int64)
  ids = []
  for bits in range(8):
    idx = [np.clip(lo[:, t] + ((bits >> (2 - t)) & 1), 0, s - 1) for t, s in enumerate((X, Y, Z))]
    ids.append((idx[0] * Y + idx[1]) * Z + idx[2])
  return int(np.unique(np.concatenate(ids)).size)


def voxel_keys(points):
  """The voxel of each of the 8 taps of every sample, in record order (occ_taps' clamped indices)."""
  p = points.reshape(-1, 3) / np.float32(CELL)
  c = p - np.float32(0.5)
  lo = np.fmin(np.fmax(np.floor(c), np.float32(-1)), np.float32(max(X, Y, Z))).astype(np.int64)
  ids = []
  for bits in range(8):
    idx = [np.clip(lo[:, t] + ((bits >> (2 - t)) & 1), 0, s - 1) for t, s in enumerate((X, Y, Z))]
    ids.append((idx[0] * Y + idx[1]) * Z + idx[2])
  return np.stack(ids, -1).reshape(-1)


def train_step_ms(train_encoder, reps):
  sys.path.insert(0, 'tests')
  import copy
  import helpers
  from snap_amd import trainer
  from snap_amd.configs import defaults
  from snap_amd.data import synthetic
  sv = helpers.tiny_localizer_config(aerial=False, feature_dim=32).bev_mapper.streetview_encoder
  cfg = defaults.occupancy_net()
  cfg.streetview_encoder = copy.deepcopy(sv)
  cfg.occupancy_mlp.layers = (32, 64, 1)
  cfg.num_samples_per_ray = 8
  meta = synthetic.meta_data(0.2, (6.4, 6.4, 3.2))
  model = occupancy_net.OccupancyNetModel(cfg, meta, engine='f32', train_encoder=train_encoder)
  params = helpers.params_to_device(model.flax_model.init(0, device='cpu')['params'], torch.device('cuda'))
  batch = helpers.batch_to_device(synthetic.make_batch(2, meta['grid'], 2, (128, 128), seed=1, with_aerial=False,
                                                       lidar_rays=5000), torch.device('cuda'))
  state = trainer.TrainState.create(params)
  freeze = None if train_encoder else 'streetview_encoder/'
  ts = []
  for i in range(reps + 2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    state, _, _ = trainer.train_step(state, batch, model=model, lr_fn=lambda s: 1e-3, freeze_params_reg_exp=freeze)
    torch.cuda.synchronize()
    if i >= 2:
      ts.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ts)), meta['grid'].extent


def vjp_leg(args, vol, vvalid, r, pts):
  from snap_amd import ops_bwd
  dev = vol.device
  P = S * N
  g = torch.Generator(device='cpu').manual_seed(3)
  dfeat = (torch.rand((P, D), generator=g) * 2 - 1).to(dev)
  kw = dict(rays=r, num_samples=S, margin=0.2)

  def fwd():
    return ops.occupancy_ray_features(vol, vvalid, CELL, want_samples=False, **kw)[0]

  def vjp():
    return ops_bwd.occupancy_ray_features_vjp(dfeat, vol.shape, CELL, **kw)

  for _ in range(args.warmup):
    fwd(); vjp()
  torch.cuda.synchronize()
  tf, tv = [], []
  for _ in range(args.reps):
    tf.append(timeit(fwd, args.inner))
    tv.append(timeit(vjp, args.inner))
  a, b = vjp(), vjp()
  same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
  del a, b
  keys = voxel_keys(pts)
  counts = np.bincount(keys, minlength=X * Y * Z)
  touched = counts[counts > 0]
  R = keys.size
  L = ops_bwd.occupancy_features_vjp_chunk()
  nbytes = R * 8 * 2 + R * D * 4 + X * Y * Z * D * 4
  f_ms, v_ms = float(np.median(tf)), float(np.median(tv))
  tr_frozen, ext = train_step_ms(False, args.reps)
  tr_enc, _ = train_step_ms(True, args.reps)
  res = dict(
      workload=f'occupancy VJP {X}x{Y}x{Z}x{D} volume, {N} rays x {S} samples', records=int(R), chunk=L,
      vjp_ms=round(v_ms, 4), producer_fwd_ms=round(f_ms, 4), vjp_ms_all=[round(t, 4) for t in tv],
      producer_fwd_ms_all=[round(t, 4) for t in tf], vjp_bitwise_repeatable=same,
      touched_voxels=int(touched.size), records_per_voxel_median=float(np.median(touched)),
      records_per_voxel_p99=float(np.percentile(touched, 99)), records_per_voxel_max=int(touched.max()),
      voxels_over_512=int((touched > 512).sum()),
      share_of_records_in_voxels_over_512=round(float(touched[touched > 512].sum()) / R, 4),
      chunks=int(((touched + L - 1) // L).sum()), essential_mb=round(nbytes / 1e6, 1),
      essential_tb_per_s=round(nbytes / v_ms / 1e9, 3),
      train_step=dict(shape=f'1 x 2 views 128 x 128, grid {tuple(ext)}, 5000 rays x 8 samples, f32 engine',
                      frozen_encoder_ms=round(tr_frozen, 2), train_encoder_ms=round(tr_enc, 2)),
      reps=args.reps, inner=args.inner)
  print(json.dumps(res), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


def timeit(fn, n):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(n):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / n


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=15)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--inner', type=int, default=3)
  ap.add_argument('--out', default=None)
  ap.add_argument('--vjp', action='store_true', help='the gather VJP leg instead of fused vs unfused')
  args = ap.parse_args()
  dev = torch.device('cuda')
  g = torch.Generator(device='cpu').manual_seed(0)
  vol = (torch.rand((1, X, Y, Z, D), generator=g) * 2 - 1).to(dev)
  vvalid = (torch.rand((1, X, Y, Z), generator=g) >= 0.4).to(dev)
  h, o, m = rays()
  r = tuple(torch.from_numpy(a).to(dev) for a in (h, o, m))
  kw = dict(rays=r, num_samples=S, margin=0.2, want_samples=False)
  _, _, (pts, _, _) = ops.occupancy_ray_features(vol, vvalid, CELL, rays=r, num_samples=S, margin=0.2)
  if args.vjp:
    return vjp_leg(args, vol, vvalid, r, pts.cpu().numpy())
  P = S * N
  rows = compulsory_rows(pts.cpu().numpy())
  results = []
  for layers in ((128, 1), (128, 256, 1)):
    gw = torch.Generator(device='cpu').manual_seed(1)
    mlp, d_in = [], D
    for w in layers:
      mlp.append(((torch.rand((d_in, w), generator=gw) - 0.5).to(dev) * 0.2, torch.zeros(w, device=dev)))
      d_in = w

    def fused():
      return ops.occupancy_head(vol, vvalid, CELL, mlp, **kw)[0]

    def unfused():
      x = ops.occupancy_ray_features(vol, vvalid, CELL, **kw)[0]
      with ops.engine_scope('f32'):
        return occupancy_net.dense_chain(mlp, x)

    for _ in range(args.warmup):
      fused(); unfused()
    torch.cuda.synchronize()
    tf, tu = [], []
    for _ in range(args.reps):                      # alternating A / B
      tf.append(timeit(fused, args.inner))
      tu.append(timeit(unfused, args.inner))
    same = bool(torch.equal(fused().reshape(-1), unfused()[..., 0].reshape(-1)))
    widths = (D,) + tuple(layers)
    flop = 2.0 * P * sum(a * b for a, b in zip(widths[:-1], widths[1:]))
    comp = rows * D * 4 + rows + 3 * 4 * N * 2 + N + P * 5      # rows, validity, rays, logits + valid
    inter = 2.0 * 4 * P * sum(widths[:-1])                        # features + hidden: written and re-read
    floor_c, floor_m = flop / PEAK_F32_MFMA, comp / PEAK_HBM
    floor = max(floor_c, floor_m)
    f_ms, u_ms = float(np.median(tf)), float(np.median(tu))
    res = dict(
        workload=f'occupancy {X}x{Y}x{Z}x{D} volume, {N} rays x {S} samples', mlp=list(layers),
        fused_ms=round(f_ms, 4), unfused_ms=round(u_ms, 4), speedup=round(u_ms / f_ms, 3),
        fused_ms_all=[round(t, 4) for t in tf], unfused_ms_all=[round(t, 4) for t in tu],
        gflop=round(flop / 1e9, 2), compulsory_mb=round(comp / 1e6, 1), distinct_voxel_rows=rows,
        intermediate_gb_avoided=round(inter / 1e9, 3), floor_ms=round(floor * 1e3, 4),
        bound='compute (f32 MFMA)' if floor_c >= floor_m else 'memory (HBM)',
        fused_frac_of_floor=round(floor * 1e3 / f_ms, 3), fused_tflops=round(flop / f_ms / 1e9, 1),
        fused_equals_unfused_bitwise=same, reps=args.reps, inner=args.inner,
    )
    results.append(res)
    print(json.dumps(res), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(results, f, indent=1)


if __name__ == '__main__':
  main()
