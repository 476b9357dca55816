"""Tool (not product): one ``ops.vote_credible`` call next to one ``ops.vote_posterior`` call and next to the torch
formulation a user would otherwise write (``torch.sort`` descending of the flattened volume, ``exp``, ``cumsum``,
``searchsorted``), at the C4 vote lattice (R = 36, 511 x 511), alternating in one process with device events.  Prints
one JSON line.

  python tools/vote_credible_bench.py [--reps 20] [--warmup 3] [--rounds 9] [--out FILE]

No time is fixed: the yardsticks are the posterior (one read of the volume by its header) and the sort in the same
run.  The op reads the volume six times for every L by its header (the maximum, four digit passes, the level pass), so
the ratio to the posterior is reported next to 6 / 1.  Reported for L = 3 and L = 8: the median and the spread of each
time, the two ratios, and launch bytes / time of the op (algorithmic bytes of the launches over the call's time: an
end-to-end figure, not a kernel's share of peak).  The op is checked once for equal bits on a repeat call, and its
thresholds against the sort formulation's, before anything is timed.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from snap_amd import ops  # noqa: E402

R, H = 36, 256
SCALE = 4.0
LEVELS = {3: (0.5, 0.9, 0.99), 8: (0.1, 0.25, 0.5, 0.68, 0.9, 0.95, 0.99, 0.999)}
PASSES_CREDIBLE, PASSES_POSTERIOR = 6, 1


def timed(fn, reps):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(reps):
    fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) / reps


def sort_formulation(votes, levels, scale):
  """Thresholds and masses by full sort (ties are NOT closed: a user's first version).  Masked cells stay in the
  sort as -inf (weight 0): no compaction and no host synchronisation inside the timed region."""
  s = torch.sort(votes.reshape(-1), descending=True).values
  w = torch.exp(scale * (s.double() - s[0].double()))
  c = torch.cumsum(w, 0)
  idx = torch.searchsorted(c, levels * c[-1]).clamp(max=c.numel() - 1)
  return s[idx], c[idx] / c[-1]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('vote_credible_bench: no GPU')
  dev = torch.device('cuda')
  rng = np.random.default_rng(7)
  Ho = 2 * H - 1
  # two street corners: a two-mode log-score with noise, 20 % of the cells masked
  a = np.arange(Ho, dtype=np.float32)[None, :, None]
  b = np.arange(Ho, dtype=np.float32)[None, None, :]
  r = np.arange(R, dtype=np.float32)[:, None, None]
  bump = lambda cr, ca, cb: -((a - ca) ** 2 + (b - cb) ** 2) / (2 * 12.0 ** 2) - np.minimum(np.abs(r - cr), R - np.abs(r - cr)) ** 2 / 8
  v = np.maximum(bump(4, 150, 170), bump(22, 380, 300) - 0.3) + 0.1 * rng.standard_normal((R, Ho, Ho)).astype(np.float32)
  v = v.astype(np.float32)
  v[rng.random(v.shape) < 0.2] = -np.inf
  votes = torch.from_numpy(v).to(dev)
  n = votes.numel()
  res = dict(tool='vote_credible_bench', device=torch.cuda.get_device_name(0), shape=[R, Ho, Ho], scale=SCALE,
             masked_fraction=0.2, reps=args.reps, rounds=args.rounds, passes=[PASSES_CREDIBLE, PASSES_POSTERIOR])
  run_p = lambda: ops.vote_posterior(votes, SCALE)
  for L, levels in LEVELS.items():
    lv_dev = torch.tensor(levels, dtype=torch.float32, device=dev).double()
    run_c = lambda: ops.vote_credible(votes, levels, SCALE)
    run_s = lambda: sort_formulation(votes, lv_dev, SCALE)
    x, y = run_c(), run_c()
    assert all(bool((p.reshape(-1).view(torch.uint8) == q.reshape(-1).view(torch.uint8)).all())
               for p, q in zip(x, y) if p is not None)
    thr_s, mass_s = run_s()
    same = bool((x[0] == thr_s).all())
    for _ in range(args.warmup):
      run_c(), run_p(), run_s()
    torch.cuda.synchronize()
    tc, tp, ts = [], [], []
    for _ in range(args.rounds):                            # alternate: all see the same neighbours on the machine
      tc.append(timed(run_c, args.reps))
      tp.append(timed(run_p, args.reps))
      ts.append(timed(run_s, args.reps))
    mc, mp, ms = float(np.median(tc)), float(np.median(tp)), float(np.median(ts))
    res['L%d' % L] = dict(
        levels=list(levels), credible_ms=round(mc, 4), credible_ms_min_max=[round(min(tc), 4), round(max(tc), 4)],
        posterior_ms=round(mp, 4), posterior_ms_min_max=[round(min(tp), 4), round(max(tp), 4)],
        sort_ms=round(ms, 4), sort_ms_min_max=[round(min(ts), 4), round(max(ts), 4)],
        ratio_credible_over_posterior=round(mc / mp, 3), ratio_of_passes=PASSES_CREDIBLE / PASSES_POSTERIOR,
        ratio_sort_over_credible=round(ms / mc, 3),
        credible_launch_tb_s=round(4.0 * n * PASSES_CREDIBLE / (mc * 1e-3) / 1e12, 3),
        thresholds_equal_to_sort=same, threshold=[float(t) for t in x[0].cpu()], mass=[float(t) for t in x[1].cpu()],
        cells=x[2][:, 0].cpu().tolist(), count=x[7].cpu().tolist())
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
