"""Tool (not product): one ``ops.vote_pairs`` call next to one ``ops.vote_smooth`` call at the C4 vote lattice (R = 36,
511 x 511) with ``motion_taps`` of one increment at the smoother benchmark's noise (sigma_xy = 0.2 m on 0.2 m cells,
sigma_yaw = 2 degrees: taps [4, 8, 8]), alternating A / B in one process with device events.  Prints one JSON line.

  python tools/vote_pairs_bench.py [--reps 30] [--warmup 5] [--out FILE]

No time is fixed: the yardstick is the smoother in the same run.  The new op repeats its predict, ratio and two adjoint
passes (no rotation gather, no combine, no normalisation) and adds three reductions that read T sources per cell; both
move 22 passes over the volume by their headers' count.  Reported: the median and the spread of each op's time, the
ratio, and launch bytes / time for both (algorithmic bytes of the launches over the call's time: an end-to-end figure
of the op, not a kernel's share of peak).  Both ops are checked once for equal bits on a repeat call before they are
timed.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from snap_amd import ops  # noqa: E402
from snap_amd.models import pose_exhaustive_voting as pev  # noqa: E402
from snap_amd.utils import geometry, grids  # noqa: E402

R, H, CELL = 36, 256, 0.2
SIGMA_XY, SIGMA_YAW, EPS, SCALE = 0.2, float(np.deg2rad(2.0)), 1e-3, 4.0
PASSES_PAIRS, PASSES_SMOOTH = 22, 22


def timed(fn, reps):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) / reps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('vote_pairs_bench: no GPU')
  dev = torch.device('cuda')
  rng = np.random.default_rng(7)
  Ho = 2 * H - 1
  grid = grids.Grid2D((H, H), CELL)
  inc = geometry.Transform2D(torch.tensor(np.deg2rad(5.0)), torch.tensor([0.93, 0.37], dtype=torch.float64))
  taps = pev.motion_taps(inc, grid, R, SIGMA_XY, SIGMA_YAW, device=dev)
  assert (taps[0].shape[0], taps[2].shape[1], taps[3].shape[1]) == (4, 8, 8)
  votes0 = torch.from_numpy((rng.standard_normal((R, Ho, Ho)) * 0.5).astype(np.float32)).to(dev)
  votes1 = torch.from_numpy((rng.standard_normal((R, Ho, Ho)) * 0.5).astype(np.float32)).to(dev)
  n = votes0.numel()
  belief = ops.vote_filter(None, votes0, pev._still_taps(R, str(dev)), SCALE, EPS)[0]
  nxt = ops.vote_filter(belief, votes1, taps, SCALE, EPS)[0]
  run_p = lambda: ops.vote_pairs(belief, nxt, taps, EPS)
  run_s = lambda: ops.vote_smooth(belief, nxt, taps, EPS)
  for run in (run_p, run_s):
    a, b = run(), run()
    assert all(bool((x.reshape(-1).view(torch.uint8) == y.reshape(-1).view(torch.uint8)).all()) for x, y in zip(a, b))
  for _ in range(args.warmup):
    run_p(), run_s()
  torch.cuda.synchronize()
  tp, ts = [], []
  for _ in range(args.rounds):                              # alternate: both see the same neighbours on the machine
    tp.append(timed(run_p, args.reps))
    ts.append(timed(run_s, args.reps))
  mp, ms = float(np.median(tp)), float(np.median(ts))
  out = run_p()
  res = dict(tool='vote_pairs_bench', device=torch.cuda.get_device_name(0), shape=[R, Ho, Ho],
             taps=[int(taps[0].shape[0]), int(taps[2].shape[1]), int(taps[3].shape[1])], uniform_mix=EPS, reps=args.reps,
             rounds=args.rounds, pairs_ms=round(mp, 4), pairs_ms_min_max=[round(min(tp), 4), round(max(tp), 4)],
             smooth_ms=round(ms, 4), smooth_ms_min_max=[round(min(ts), 4), round(max(ts), 4)],
             ratio_pairs_over_smooth=round(mp / ms, 3), passes=[PASSES_PAIRS, PASSES_SMOOTH],
             pairs_launch_tb_s=round(4.0 * n * PASSES_PAIRS / (mp * 1e-3) / 1e12, 3),
             smooth_launch_tb_s=round(4.0 * n * PASSES_SMOOTH / (ms * 1e-3) / 1e12, 3),
             pairs_stats=[float(v) for v in out[3].cpu()], pairs_count=out[4].cpu().tolist())
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
