"""Tool (not product): ``ops.vote_sample`` (B = 1024 and 65536) and ``ops.vote_sample_back`` (B = 1024) at the C4 vote
lattice (R = 36, 511 x 511) and at [36, 31, 33], with ``motion_taps`` of one increment at the filter tests' default
noise (sigma_xy = 0.2 m on 0.25 m cells, sigma_yaw = 0.15 rad); next to each ``vote_sample`` the only other way to draw
from a volume, ``torch.softmax`` + ``torch.multinomial`` over the flattened volume on the same device, where the volume
has fewer than 2^24 cells (torch's limit).  Alternating A / B in one process with device events.  Prints one JSON line.

  python tools/vote_sample_bench.py [--reps 20] [--warmup 3] [--rounds 7] [--out FILE]

No ratio is fixed in advance.  The expectation: ``vote_sample`` reads the volume twice (the peak, the row sums) and a
row of cells per draw, in four launches, so at these sizes it is bound by its launches and, at B = 65536, by the draws;
``vote_sample_back`` repeats the filter's predict step (8 passes over the volume) before its chains.  Reported: the
median and the spread of each time.  Every op is checked once for equal bytes on a repeat call before it is timed.
Needs a GPU: there is no fall-back.
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

R, CELL = 36, 0.25
SIGMA_XY, SIGMA_YAW, EPS, SCALE = 0.2, 0.15, 1e-3, 4.0
SHAPES = (('c4', (R, 511, 511)), ('small', (R, 31, 33)))
TORCH_MAX_CATEGORIES = 1 << 24


def timed(fn, reps):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) / reps


def same_bytes(a, b):
  return all(bool((x.reshape(-1).view(torch.uint8) == y.reshape(-1).view(torch.uint8)).all()) for x, y in zip(a, b))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('vote_sample_bench: no GPU')
  dev = torch.device('cuda')
  rng = np.random.default_rng(7)
  inc = geometry.Transform2D(torch.tensor(0.12, dtype=torch.float64), torch.tensor([0.3, -0.2], dtype=torch.float64))
  res = dict(tool='vote_sample_bench', device=torch.cuda.get_device_name(0), reps=args.reps, rounds=args.rounds,
             shapes={})
  for tag, (r, Ho, Wo) in SHAPES:
    grid = grids.Grid2D(((Ho + 1) // 2, (Wo + 1) // 2), CELL)
    taps = pev.motion_taps(inc, grid, r, SIGMA_XY, SIGMA_YAW, device=dev)
    votes = torch.from_numpy((rng.standard_normal((r, Ho, Wo)) * 0.5).astype(np.float32)).to(dev)
    belief = ops.vote_filter(None, votes, pev._still_taps(r, str(dev)), SCALE, EPS)[0]
    n = belief.numel()
    nxt = ops.vote_sample(belief, 1024, 1, 1)[0]
    runs = {'sample_1024': lambda: ops.vote_sample(belief, 1024, 1, 0),
            'sample_65536': lambda: ops.vote_sample(belief, 65536, 1, 0),
            'sample_back_1024': lambda: ops.vote_sample_back(belief, nxt, taps, EPS, 1, 0)}
    for run in runs.values():
      assert same_bytes(run(), run())
    if n < TORCH_MAX_CATEGORIES:
      flat = belief.reshape(-1)
      runs['torch_1024'] = lambda: torch.multinomial(torch.softmax(flat, 0), 1024, replacement=True)
      runs['torch_65536'] = lambda: torch.multinomial(torch.softmax(flat, 0), 65536, replacement=True)
    for _ in range(args.warmup):
      for run in runs.values():
        run()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):                            # alternate: all see the same neighbours on the machine
      for k, run in runs.items():
        times[k].append(timed(run, args.reps))
    out = dict(shape=[r, Ho, Wo], cells=n, taps=[int(taps[0].shape[0]), int(taps[2].shape[1]), int(taps[3].shape[1])])
    for k, t in times.items():
      out[k + '_ms'] = round(float(np.median(t)), 4)
      out[k + '_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
    for b in (1024, 65536):
      if f'torch_{b}' in times:
        out[f'ratio_sample_over_torch_{b}'] = round(out[f'sample_{b}_ms'] / out[f'torch_{b}_ms'], 3)
    out['sample_back_count'] = runs['sample_back_1024']()[3].cpu().tolist()
    res['shapes'][tag] = out
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
