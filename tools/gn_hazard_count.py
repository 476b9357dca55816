"""How many (image, group) entries of bench.py's default workload trip the hazard of the GroupNorm
finalize (gn_finalize_tiled_kernel re-reduces a group with mean^2 > 4 var from y): wraps
``ops.group_norm_stats``, runs one bench step and prints the count and the largest mean^2 / var
(profiles/gn_hazard_ab.json).  Run from the repository root on the GPU: ``python tools/gn_hazard_count.py``."""
import runpy, sys, torch
sys.path.insert(0, '.')
from snap_amd import ops
orig = ops.group_norm_stats
tot = {'fused_calls': 0, 'groups': 0, 'hazard': 0, 'max_ratio2': 0.0}
def wrapped(x, gamma, *, groups=32, eps=1e-5, relu_first=False, want_rstd=False):
  out = orig(x, gamma, groups=groups, eps=eps, relu_first=relu_first, want_rstd=True)
  if getattr(x, '_snap_gn_partial', None) is not None or getattr(x, '_snap_gn_partial_relu', None) is not None:
    mu, _, rstd = out
    C = mu.shape[1]
    m = mu.double()[:, ::C // groups]; r = rstd.double()[:, ::C // groups]
    var = (1 / (r * r) - eps).clamp_min(1e-30)
    ratio2 = m * m / var
    tot['fused_calls'] += 1; tot['groups'] += ratio2.numel(); tot['hazard'] += int((ratio2 > 4).sum())
    tot['max_ratio2'] = max(tot['max_ratio2'], float(ratio2.max()))
  return out if want_rstd else out[:2]
ops.group_norm_stats = wrapped
sys.argv = ['bench.py', '--gpus', '1', '--steps', '1', '--warmup', '0']
try:
  runpy.run_path('bench.py', run_name='__main__')
except SystemExit:
  pass
print('HAZARD_COUNT', tot)
