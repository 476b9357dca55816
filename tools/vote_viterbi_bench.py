"""Tool (not product): one step of ``ops.vote_viterbi`` next to one step of ``ops.vote_filter`` at the C4 vote lattice
(R = 36, 511 x 511) with ``motion_taps`` / ``motion_log_taps`` of one increment at the filter tests' default noise
(sigma_xy = 0.2 m on 0.25 m cells, sigma_yaw = 0.15 rad), alternating A / B in one process with device events.  Prints
one JSON line.

  python tools/vote_viterbi_bench.py [--reps 30] [--warmup 5] [--out FILE]

The expectation checked is qualitative: the Viterbi step moves 10 passes over the volume (4-byte cells; the kernel
file's header) against the filter's 12 and has no float64 or transcendental work per tap, so it should not be slower.
Reported: the median and the spread of each op's time, the ratio, and launch bytes / time for both (algorithmic bytes
of the launches over the call's time: an end-to-end figure of the op, not a kernel's share of peak).  Both ops are
checked once for equal bits on a repeat call before they are timed.  Needs a GPU: there is no fall-back.
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

R, H, CELL = 36, 256, 0.25
SIGMA_XY, SIGMA_YAW, EPS, SCALE = 0.2, 0.15, 1e-3, 4.0
PASSES_VITERBI, PASSES_FILTER = 10, 12


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
    raise SystemExit('vote_viterbi_bench: no GPU')
  dev = torch.device('cuda')
  rng = np.random.default_rng(7)
  Ho = 2 * H - 1
  grid = grids.Grid2D((H, H), CELL)
  inc = geometry.Transform2D(torch.tensor(0.12, dtype=torch.float64), torch.tensor([0.3, -0.2], dtype=torch.float64))
  taps = pev.motion_taps(inc, grid, R, SIGMA_XY, SIGMA_YAW, device=dev)
  ltaps = pev.motion_log_taps(inc, grid, R, SIGMA_XY, SIGMA_YAW, device=dev)
  votes0 = torch.from_numpy((rng.standard_normal((R, Ho, Ho)) * 0.5).astype(np.float32)).to(dev)
  votes1 = torch.from_numpy((rng.standard_normal((R, Ho, Ho)) * 0.5).astype(np.float32)).to(dev)
  n = votes0.numel()
  log_stay, log_jump = pev._viterbi_log_weights(EPS, n)
  belief = ops.vote_filter(None, votes0, pev._still_taps(R, str(dev)), SCALE, EPS)[0]
  score = ops.vote_viterbi(None, votes0, pev._still_log_taps(R, str(dev)), SCALE, log_stay, log_jump)[0]
  run_v = lambda: ops.vote_viterbi(score, votes1, ltaps, SCALE, log_stay, log_jump)
  run_f = lambda: ops.vote_filter(belief, votes1, taps, SCALE, EPS)
  for run in (run_v, run_f):
    a, b = run(), run()
    assert all(bool((x.reshape(-1).view(torch.int32) == y.reshape(-1).view(torch.int32)).all()) for x, y in zip(a, b))
  for _ in range(args.warmup):
    run_v(), run_f()
  torch.cuda.synchronize()
  tv, tf = [], []
  for _ in range(args.rounds):                              # alternate: both see the same neighbours on the machine
    tv.append(timed(run_v, args.reps))
    tf.append(timed(run_f, args.reps))
  mv, mf = float(np.median(tv)), float(np.median(tf))
  count = run_v()[3].cpu().tolist()
  res = dict(tool='vote_viterbi_bench', device=torch.cuda.get_device_name(0), shape=[R, Ho, Ho],
             taps=[int(ltaps[0].shape[0]), int(ltaps[2].shape[1]), int(ltaps[3].shape[1])], reps=args.reps,
             rounds=args.rounds, viterbi_ms=round(mv, 4), viterbi_ms_min_max=[round(min(tv), 4), round(max(tv), 4)],
             filter_ms=round(mf, 4), filter_ms_min_max=[round(min(tf), 4), round(max(tf), 4)],
             ratio_viterbi_over_filter=round(mv / mf, 3), passes=[PASSES_VITERBI, PASSES_FILTER],
             viterbi_launch_tb_s=round(4.0 * n * PASSES_VITERBI / (mv * 1e-3) / 1e12, 3),
             filter_launch_tb_s=round(4.0 * n * PASSES_FILTER / (mf * 1e-3) / 1e12, 3), viterbi_count=count)
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
