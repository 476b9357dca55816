"""Tool (not product): the OccupancyNet query chain on the lidar training workload -- one scene, a
120 x 160 x 60 x 128 f32 volume, 10 000 rays x 100 samples -- fused (ops.occupancy_head, one launch)
against the unfused chain (ops.occupancy_ray_features + one ops.dense per layer on the exact f32
engine), alternating A / B in one process with device events.  Prints one JSON line per MLP shape.

  python tools/occupancy_bench.py [--reps 15] [--warmup 3] [--out FILE]

Floor = max(algorithmic FLOP / 157 TFLOP/s (f32 MFMA), compulsory bytes / 8 TB/s); compulsory bytes =
the distinct 512-byte voxel rows the 8 taps of all samples touch (counted on the host) + the volume
validity bytes of those voxels + the outputs.  Intermediate bytes avoided = what the unfused chain
writes and re-reads: the [P, 128] feature rows and every hidden activation.
"""
import argparse
import json
import sys

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
  args = ap.parse_args()
  dev = torch.device('cuda')
  g = torch.Generator(device='cpu').manual_seed(0)
  vol = (torch.rand((1, X, Y, Z, D), generator=g) * 2 - 1).to(dev)
  vvalid = (torch.rand((1, X, Y, Z), generator=g) >= 0.4).to(dev)
  h, o, m = rays()
  r = tuple(torch.from_numpy(a).to(dev) for a in (h, o, m))
  kw = dict(rays=r, num_samples=S, margin=0.2, want_samples=False)
  _, _, (pts, _, _) = ops.occupancy_ray_features(vol, vvalid, CELL, rays=r, num_samples=S, margin=0.2)
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
