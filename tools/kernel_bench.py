"""Single-kernel micro-benchmarks at the C2 shapes (HIP-event timed; used for tuning and
as the target of rocprofv3 --pmc passes).   python tools/kernel_bench.py pose_score [iters]
(pose_score | pose_score_c4 | voting_c4 | vote_peaks_c4 | vote_posterior_c4 | vote_fuse_c4 | vote_filter_c4 | vote_smooth_c4 | vote_refine_c4 | vote_modes_c4 | vote_recall_c4 | vote_odometry_c4 | vote_rebase_c4 | vote_temper_c4 | vote_prior_c4 | vote_raster)
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snap_amd import ops  # noqa: E402


def timeit(fn, iters):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  e0 = torch.cuda.Event(enable_timing=True)
  e1 = torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / iters


def pose_score(iters):
  B, Nq, X, Y, P = 8, 4652, 128, 128, 10001
  g = torch.Generator(device='cuda').manual_seed(0)
  sim = torch.rand((B, Nq, X, Y), device='cuda', generator=g)
  ang = (torch.rand((B, P), device='cuda', generator=g) - 0.5) * 2 * math.pi
  t = torch.rand((B, P, 2), device='cuda', generator=g) * 25.6
  poses = torch.cat([ang[..., None], t], -1).contiguous()
  q_xy = (torch.rand((B, Nq, 2), device='cuda', generator=g) - 0.5) * 16.0
  valid = torch.ones((B, Nq), dtype=torch.bool, device='cuda')
  ms = timeit(lambda: ops.pose_score(sim, poses, q_xy, valid, None, 0.2), iters)
  by = 4.0 * sim.numel()
  print(f'pose_score: {ms:.4f} ms  {by / ms / 1e6:.1f} GB/s  ({by / ms / 1e6 / 8000:.3f} of 8 TB/s)')


def pose_score_c4(iters):
  """Eval-path shapes (BASELINE configs[3] / SURVEY C4): 256x256 map, 20 001 sampled poses,
  then the 41^3 refinement lattice -- the band-tiled kernel (a 256 KB plane does not fit LDS)."""
  B, Nq, X, Y = 1, 4652, 256, 256
  g = torch.Generator(device='cuda').manual_seed(0)
  sim = torch.rand((B, Nq, X, Y), device='cuda', generator=g)
  q_xy = (torch.rand((B, Nq, 2), device='cuda', generator=g) - 0.5) * 16.0
  valid = torch.ones((B, Nq), dtype=torch.bool, device='cuda')
  for P in (20001, 68921):
    ang = (torch.rand((B, P), device='cuda', generator=g) - 0.5) * 2 * math.pi
    t = torch.rand((B, P, 2), device='cuda', generator=g) * 51.2
    poses = torch.cat([ang[..., None], t], -1).contiguous()
    ms = timeit(lambda: ops.pose_score(sim, poses, q_xy, valid, None, 0.2), iters)
    by = 4.0 * sim.numel()
    print(f'pose_score C4 P={P}: {ms:.3f} ms  plane bytes {by / 1e9:.2f} GB -> {by / ms / 1e6:.0f} GB/s; '
          f'gather volume 16 B x P x Nq = {16.0 * P * Nq / 1e9:.2f} GB -> {16.0 * P * Nq / ms / 1e6:.0f} GB/s')


def voting_c4(iters):
  """Exhaustive (x, y, theta) correlation at H = W = 256, R = 36, Dm = 32 (k14 + k15)."""
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.models import types
  from snap_amd.utils import grids
  H = W = 256
  R, Dm = 36, 32
  g = torch.Generator(device='cuda').manual_seed(0)
  fq = torch.nn.functional.normalize(torch.randn((H, W, Dm), device='cuda', generator=g), dim=-1)
  fm = torch.nn.functional.normalize(torch.randn((H, W, Dm), device='cuda', generator=g), dim=-1)
  vq = torch.rand((H, W), device='cuda', generator=g) < 0.9
  vm = torch.ones((H, W), dtype=torch.bool, device='cuda')
  grid = grids.Grid2D((H, W), 0.2)
  pq = types.FeaturePlane(features=fq, valid=vq)
  pm = types.FeaturePlane(features=fm, valid=vm)
  ms = timeit(lambda: pev.exhaustive_pose_voting(pq, pm, R, grid), max(2, iters // 5))
  flop = 2.0 * R * (2 * H - 1) * (2 * W - 1) * H * W * Dm
  by = 4.0 * (R * H * W * Dm + H * W * Dm + R * (2 * H - 1) * (2 * W - 1))
  print(f'voting C4: {ms:.1f} ms  direct-form {flop / 1e12:.1f} TFLOP -> {flop / ms / 1e9:.1f} TFLOP/s '
        f'({flop / ms / 1e9 / 157.3:.3f} of the f32 MFMA peak); algorithmic bytes {by / 1e6:.0f} MB')


def median_ms(fn, reps):
  """Median of ``reps`` single calls, each between its own pair of events (after the caller's warm-up)."""
  evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
  for e0, e1 in evs:
    e0.record()
    fn()
    e1.record()
  torch.cuda.synchronize()
  return sorted(e0.elapsed_time(e1) for e0, e1 in evs)[reps // 2]


def alternated_blocks(cases, blocks=5):
  """cases = (fn, warm-up calls, calls per block), ...: warm every case up, then ``blocks`` rounds of one ``median_ms``
  block of each case in turn -> per case (the median block, the blocks)."""
  for fn, warm, _ in cases:
    for _ in range(warm):
      fn()
  torch.cuda.synchronize()
  out = [[] for _ in cases]
  for _ in range(blocks):
    for ms, (fn, _, reps) in zip(out, cases):
      ms.append(median_ms(fn, reps))
  return [(sorted(ms)[blocks // 2], ms) for ms in out]


def emit_json(res):
  """One JSON line on stdout; a `json=<path>` argument behind the iteration count also writes it to that file."""
  import json
  line = json.dumps(res)
  print(line)
  for a in sys.argv[3:]:
    if a.startswith('json='):
      with open(a[5:], 'w') as f:
        f.write(line + '\n')


def torch_peaks(votes, k, radius_r, radius_xy):
  """What a user would write without the kernel: circular pad on r, max_pool3d (-inf padded in a, b), compare, topk.
  (Ties on a plateau all survive the compare: the composition has no order contract.)"""
  x = torch.cat([votes[-radius_r:], votes, votes[:radius_r]], 0) if radius_r else votes
  win = (2 * radius_r + 1, 2 * radius_xy + 1, 2 * radius_xy + 1)
  m = torch.nn.functional.max_pool3d(x[None, None], win, stride=1, padding=(0, radius_xy, radius_xy))[0, 0]
  val, idx = torch.topk(torch.where(votes == m, votes, float('-inf')).reshape(-1), k)
  return idx, val


def vote_peaks_c4(iters):
  """Top-K peak extraction on the C4 vote volume (R = 36, 511 x 511, K = 16, radius (1, 1)): the kernel alone against
  the torch composition on the same votes, blocks of the two alternated, medians of single calls.  One JSON line;
  `json=<path>` as a third argument also writes it to that file."""
  R, Ho, Wo, K, rr, rx = 36, 511, 511, 16, 1, 1
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g)       # (peak density 1 / 27: denser than real votes)
  index, score, count = ops.vote_peaks(votes, K, rr, rx)
  idx, val = torch_peaks(votes, K, rr, rx)
  flat = (index[:, 0].long() * Ho + index[:, 1]) * Wo + index[:, 2]
  assert torch.equal(flat, idx) and torch.equal(score, val), 'kernel and torch composition disagree on tie-free votes'
  kernel = lambda: ops.vote_peaks(votes, K, rr, rx)
  compo = lambda: torch_peaks(votes, K, rr, rx)
  (k_ms, ks), (t_ms, ts) = alternated_blocks(((kernel, 5, max(iters, 5)), (compo, 5, max(iters // 2, 5))))
  # the other settings run the kernel's generic body (run-time radii): timed alone, on the same votes
  generic = {}
  for kk, r_, x_ in ((64, 2, 4), (5, 0, 2)):
    fn = lambda: ops.vote_peaks(votes, kk, r_, x_)
    for _ in range(5):
      fn()
    torch.cuda.synchronize()
    generic[f'K{kk}_r{r_}_xy{x_}'] = round(sorted(median_ms(fn, max(iters // 2, 5)) for _ in range(3))[1], 4)
  by = 4.0 * votes.numel()
  pose_score_rate = 5.4e12        # B/s of pose_score_db_kernel on this chip
  res = dict(case='vote_peaks_c4', shape=[R, Ho, Wo], K=K, radius=[rr, rx], kernel_ms=round(k_ms, 4),
             kernel_ms_blocks=[round(v, 4) for v in ks], torch_composition_ms=round(t_ms, 4),
             torch_composition_ms_blocks=[round(v, 4) for v in ts], speedup=round(t_ms / k_ms, 2),
             generic_body_ms=generic, volume_bytes=int(by), kernel_GBps_of_one_read=round(by / k_ms / 1e6, 1),
             fraction_of_pose_score_hbm_rate=round(by / (k_ms * 1e-3) / pose_score_rate, 3),
             pose_score_hbm_rate_Bps=pose_score_rate, timing='median of single calls between device events, 5 blocks '
             'of each alternated, median block; ops.vote_peaks = both launches + its three torch.empty outputs and workspace')
  emit_json(res)


def torch_posterior(votes, scale):
  """What a user would write without the kernel: logsumexp over the volume and along each axis, the marginals'
  moments, the entropy from the full normalised volume (f32 throughout, centred second moments)."""
  R, Ho, Wo = votes.shape
  fin = torch.isfinite(votes)
  x = torch.where(fin, votes * scale, float('-inf'))
  log_z = torch.logsumexp(x.reshape(-1), 0)
  lxy = torch.logsumexp(x, 0) - log_z
  lr = torch.logsumexp(x.reshape(R, -1), 1) - log_z
  pxy, pr = lxy.exp(), lr.exp()
  a = torch.arange(Ho, device=votes.device, dtype=torch.float32)[:, None]
  b = torch.arange(Wo, device=votes.device, dtype=torch.float32)[None, :]
  ea, eb = (pxy * a).sum(), (pxy * b).sum()
  ang = torch.arange(R, device=votes.device, dtype=torch.float32) * (2 * math.pi / R)
  c, s = (pr * ang.cos()).sum(), (pr * ang.sin()).sum()
  ent = log_z - ((x - log_z).exp() * torch.where(fin, x, 0.0)).sum()
  stats = torch.stack([log_z, x.max(), ea, eb, (pxy * (a - ea) ** 2).sum(), (pxy * (a - ea) * (b - eb)).sum(),
                       (pxy * (b - eb) ** 2).sum(), c, s, torch.atan2(s, c) * (R / (2 * math.pi)) % R,
                       torch.hypot(c, s), ent])
  return lxy, lr, stats, fin.sum()


def vote_posterior_c4(iters):
  """The pose distribution of the C4 vote volume (R = 36, 511 x 511; the border the voting masks for low overlap is
  -inf): whole ops.vote_posterior calls against the torch composition on the same votes, blocks of the two
  alternated, medians of single calls (kernel times: a rocprofv3 --kernel-trace --stats run of this case).  One JSON line; `json=<path>` as a third argument also writes it to that file."""
  R, H, scale = 36, 256, 8.0
  Ho = Wo = 2 * H - 1
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  lxy, lr, stats, count = ops.vote_posterior(votes, scale)
  t_lxy, t_lr, t_stats, t_n = torch_posterior(votes, scale)
  fin = torch.isfinite(t_lxy)
  assert torch.equal(fin, torch.isfinite(lxy)) and int(count[0]) == int(t_n)
  err = dict(log_prob_xy=float((lxy[fin] - t_lxy[fin]).abs().max()), log_prob_r=float((lr - t_lr).abs().max()),
             stats=[float(v) for v in (stats[:12] - t_stats).abs()])
  assert err['log_prob_xy'] < 1e-3 and err['log_prob_r'] < 1e-3 and max(err['stats'][:2]) < 1e-3, err
  kernel = lambda: ops.vote_posterior(votes, scale)
  compo = lambda: torch_posterior(votes, scale)
  (k_ms, ks), (t_ms, ts) = alternated_blocks(((kernel, 5, max(iters, 5)), (compo, 5, max(iters // 2, 5))))
  by = 4.0 * votes.numel()
  hbm_peak = 8.0e12               # B/s, the MI355X's HBM3E peak
  res = dict(case='vote_posterior_c4', shape=[R, Ho, Wo], scale=scale, masked_fraction=round(1 - int(t_n) / votes.numel(), 4),
             call_ms=round(k_ms, 4), call_ms_blocks=[round(v, 4) for v in ks],
             torch_composition_ms=round(t_ms, 4), torch_composition_ms_blocks=[round(v, 4) for v in ts],
             speedup=round(t_ms / k_ms, 2), volume_bytes=int(by), call_GBps_of_one_read=round(by / k_ms / 1e6, 1),
             call_fraction_of_hbm_peak=round(by / (k_ms * 1e-3) / hbm_peak, 3),
             torch_GBps_of_one_read=round(by / t_ms / 1e6, 1),
             torch_fraction_of_hbm_peak=round(by / (t_ms * 1e-3) / hbm_peak, 3), hbm_peak_Bps=hbm_peak,
             max_abs_difference_to_torch=err, timing='call_ms = one whole ops.vote_posterior call between device events '
             'on an idle stream (its five torch.empty allocations, the ctypes call and both launches), NOT kernel time: '
             'the two kernels alone are in profiles/vote_posterior_kernel_stats.csv; median of single calls, 5 blocks of '
             'each alternated, median block', caveat='the 37.6 MB volume is read again on every repetition and fits the '
             '256 MB Infinity Cache, so the read need not come from HBM: the fractions relate one read of the volume per '
             'call to the HBM peak, whatever served the read')
  emit_json(res)


def torch_fuse(volumes, shifts_host, weights_host):
  """What a user would write without the kernel, per frame and rotation: ``roll`` in k, shifted slices in (a, b),
  ``lerp`` along every axis with a fraction, -inf outside the slice and where any tap is -inf (finite votes otherwise: no NaN handling)."""
  N, R, Ho, Wo = volumes.shape
  total = torch.zeros((R, Ho, Wo), device=volumes.device)
  dead = torch.zeros((R, Ho, Wo), dtype=torch.bool, device=volumes.device)
  for n in range(N):
    dk = float(shifts_host[n, 0, 0])
    lk = math.floor(dk)
    fk = dk - lk
    lo = torch.roll(volumes[n], -lk, 0)
    hi = torch.roll(volumes[n], -lk - 1, 0)
    for r in range(R):
      da, db = float(shifts_host[n, r, 1]), float(shifts_host[n, r, 2])
      la, lb = math.floor(da), math.floor(db)
      fa, fb = da - la, db - lb
      ua, ub = int(fa > 0), int(fb > 0)                  # an upper tap only where the fraction is not 0
      a0, a1 = max(0, -la), min(Ho, Ho - la - ua)
      b0, b1 = max(0, -lb), min(Wo, Wo - lb - ub)
      planes = []
      for src in (lo[r], hi[r]) if fk > 0 else (lo[r],):
        rows = []
        for da_ in range(ua + 1):
          c0 = src[a0 + la + da_:a1 + la + da_, b0 + lb:b1 + lb]
          rows.append(torch.lerp(c0, src[a0 + la + da_:a1 + la + da_, b0 + lb + 1:b1 + lb + 1], fb) if ub else c0)
        planes.append(torch.lerp(rows[0], rows[1], fa) if ua else rows[0])
      bl = torch.lerp(planes[0], planes[1], fk) if fk > 0 else planes[0]
      ok = torch.isfinite(bl)
      inside = torch.zeros((Ho, Wo), dtype=torch.bool, device=volumes.device)
      inside[a0:a1, b0:b1] = ok
      dead[r] |= ~inside
      total[r, a0:a1, b0:b1] += float(weights_host[n]) * torch.where(ok, bl, 0.0)
  return torch.where(dead, float('-inf'), total)


def vote_fuse_c4(iters):
  """Multi-frame fusion at the C4 vote volume (R = 36, 511 x 511, N = 4 frames; the low-overlap border of every
  frame's volume -inf; shifts from a motion of 1 m and 5 degrees per frame on the 256^2 grid of 0.2 m cells, all
  fractional): whole ops.vote_fuse calls against the torch composition of the same result on the same inputs, blocks
  of the two alternated, medians of single calls.  One JSON line; `json=<path>` as a third argument also writes it."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import geometry, grids
  R, H, N = 36, 256, 4
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  volumes = torch.randn((N, R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  volumes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None, None], volumes, float('-inf')).contiguous()
  step = np.arange(N)
  yaw = np.deg2rad(5.0) * step
  q0_t_q = geometry.Transform2D(torch.tensor(yaw), torch.tensor(np.stack([0.93 * step, 0.37 * step], -1)))
  shifts = pev.sequence_shift_table(q0_t_q, grid, R).cuda()
  weights = torch.tensor([1.0, 0.9, 0.8, 0.7], device='cuda')
  sh_host, w_host = shifts.cpu().numpy(), weights.cpu().numpy()
  planes_read = sum(2 if (sh_host[n, 0, 0] % 1) else 1 for n in range(N))
  fused, count = ops.vote_fuse(volumes, shifts, weights)
  t_fused = torch_fuse(volumes, sh_host, w_host)
  fin = torch.isfinite(t_fused)
  assert torch.equal(fin, torch.isfinite(fused)) and int(count[0]) == int(fin.sum()) and int(count[1]) == 0
  err = float((fused[fin] - t_fused[fin]).abs().max())
  assert err < 1e-4, err
  kernel = lambda: ops.vote_fuse(volumes, shifts, weights)
  compo = lambda: torch_fuse(volumes, sh_host, w_host)
  (k_ms, ks), (t_ms, ts) = alternated_blocks(((kernel, 5, max(iters, 5)), (compo, 2, 3)))
  by = 4.0 * R * Ho * Wo * (1 + planes_read)
  hbm_peak = 8.0e12               # B/s, the MI355X's HBM3E peak
  res = dict(case='vote_fuse_c4', shape=[N, R, Ho, Wo], masked_fraction_in=round(1 - float(torch.isfinite(volumes).float().mean()), 4),
             masked_fraction_out=round(1 - int(count[0]) / fused.numel(), 4), planes_read=planes_read,
             shift_rows_frame1=[[round(float(x), 4) for x in sh_host[1, r]] for r in (0, 9)],
             call_ms=round(k_ms, 4), call_ms_blocks=[round(v, 4) for v in ks],
             torch_composition_ms=round(t_ms, 4), torch_composition_ms_blocks=[round(v, 4) for v in ts],
             speedup=round(t_ms / k_ms, 2), algorithmic_bytes=int(by), call_GBps_algorithmic=round(by / k_ms / 1e6, 1),
             call_fraction_of_hbm_peak=round(by / (k_ms * 1e-3) / hbm_peak, 3), hbm_peak_Bps=hbm_peak,
             max_abs_difference_to_torch=err, timing='call_ms = one whole ops.vote_fuse call between device events on an '
             'idle stream (its three torch.empty allocations, the ctypes call and the three launches), NOT kernel time; '
             'median of single calls, 5 blocks of each alternated, median block; the torch composition is N R = 144 '
             'rounds of slices and lerps, 3 calls per block',
             caveat='the 150 MB of volumes are read again on every repetition and fit the 256 MB Infinity Cache, so the '
             'reads need not come from HBM: the fraction relates the algorithmic bytes of one call to the HBM peak, '
             'whatever served them')
  emit_json(res)


def torch_filter(belief, votes, taps_host, scale, eps):
  """What a user would write without the kernel: exp relative to the peak, ``roll`` in k, shifted slices per rotation
  and tap in (a, b), then log, the vote product and ``logsumexp`` (f32 throughout; finite votes or -inf: no NaN
  handling)."""
  tk, lk, ta, tb, off = taps_host
  R, Ho, Wo = belief.shape
  fin = torch.isfinite(belief)
  M = torch.where(fin, belief, float('-inf')).max()
  d = belief - M
  p = torch.where(fin & (d >= -40), d.exp(), 0.0)
  t0 = torch.zeros_like(p)
  for i, w in enumerate(tk):
    t0 += float(w) * torch.roll(p, -(lk + i), 0)
  t2 = torch.zeros_like(p)
  for r in range(R):
    t1 = torch.zeros_like(p[0])
    for i, w in enumerate(ta[r]):
      s = int(off[r, 0]) + i
      a0, a1 = max(0, -s), min(Ho, Ho - s)
      if a0 < a1 and w:
        t1[a0:a1] += float(w) * t0[r, a0 + s:a1 + s]
    for i, w in enumerate(tb[r]):
      s = int(off[r, 1]) + i
      b0, b1 = max(0, -s), min(Wo, Wo - s)
      if b0 < b1 and w:
        t2[r, :, b0:b1] += float(w) * t1[:, b0 + s:b1 + s]
  prior = (1 - eps) * t2 / t2.sum(dtype=torch.float64).float() + eps / p.numel()
  u = scale * votes + prior.log()
  log_z = torch.logsumexp(u.reshape(-1), 0)
  return u - log_z, log_z


def vote_filter_c4(iters):
  """One step of the recursive pose filter at the C4 vote volume (R = 36, 511 x 511; the low-overlap border of the
  votes -inf; the belief a previous step's output; Tk = 4, Ta = Tb = 8: an increment of 1 m and 5 degrees with
  sigma_xy = 0.2 m, sigma_yaw = 2 degrees on the 256^2 grid of 0.2 m cells): whole ops.vote_filter calls against the
  torch composition of the same result on the same inputs, blocks of the two alternated, medians of single calls.
  One JSON line; `json=<path>` as a third argument also writes it."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import geometry, grids
  R, H, scale, eps = 36, 256, 8.0, 1e-3
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  keep = (ov[:, None] * ov[None, :] > 0.05 * H * H)[None]
  frames = [torch.where(keep, torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25, float('-inf')).contiguous()
            for _ in range(2)]
  step = geometry.Transform2D(torch.tensor(np.deg2rad(5.0)), torch.tensor([0.93, 0.37], dtype=torch.float64))
  taps = pev.motion_taps(step, grid, R, 0.2, np.deg2rad(2.0), device='cuda')
  Tk, Ta, Tb = taps[0].shape[0], taps[2].shape[1], taps[3].shape[1]
  assert (Tk, Ta, Tb) == (4, 8, 8), (Tk, Ta, Tb)
  taps_host = tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in taps)
  belief = pev.filter_votes(None, frames[0], None, grid, R, 0.2, np.deg2rad(2.0), temperature=scale)['belief']
  votes = frames[1]
  out, stats, count = ops.vote_filter(belief, votes, taps, scale, eps)
  t_out, t_lz = torch_filter(belief, votes, taps_host, scale, eps)
  fin = torch.isfinite(t_out)
  assert torch.equal(fin, torch.isfinite(out)) and int(count[0]) == int(fin.sum()) and int(count[2]) == 0
  err = float((out[fin] - t_out[fin]).abs().max())
  assert err < 1e-3 and abs(float(stats[0]) - float(t_lz)) < 1e-3, (err, float(stats[0]), float(t_lz))
  kernel = lambda: ops.vote_filter(belief, votes, taps, scale, eps)
  start = lambda: ops.vote_filter(None, votes, taps, scale, eps)
  compo = lambda: torch_filter(belief, votes, taps_host, scale, eps)
  (k_ms, ks), (s_ms, ss), (t_ms, ts) = alternated_blocks(
      ((kernel, 5, max(iters, 5)), (start, 5, max(iters, 5)), (compo, 2, 3)))
  n = R * Ho * Wo
  by = 4.0 * n * 12                # vote_filter.hip's header: 12 passes over the volume with a belief, 3 without
  hbm_peak = 8.0e12                # B/s, the MI355X's HBM3E peak
  res = dict(case='vote_filter_c4', shape=[R, Ho, Wo], taps=[Tk, Ta, Tb], scale=scale, uniform_mix=eps,
             masked_fraction_votes=round(1 - float(torch.isfinite(votes).float().mean()), 4),
             cells_with_mass=int(count[3]), mass_kept=round(float(stats[1]), 6), log_evidence=round(float(stats[0]), 4),
             call_ms=round(k_ms, 4), call_ms_blocks=[round(v, 4) for v in ks],
             call_ms_without_belief=round(s_ms, 4), call_ms_without_belief_blocks=[round(v, 4) for v in ss],
             torch_composition_ms=round(t_ms, 4), torch_composition_ms_blocks=[round(v, 4) for v in ts],
             speedup=round(t_ms / k_ms, 2), launch_bytes=int(by), call_GBps_of_launch_bytes=round(by / k_ms / 1e6, 1),
             call_fraction_of_hbm_peak=round(by / (k_ms * 1e-3) / hbm_peak, 3), hbm_peak_Bps=hbm_peak,
             max_abs_difference_to_torch=err, timing='call_ms = one whole ops.vote_filter call between device events on '
             'an idle stream (its four torch.empty allocations, the ctypes call and the seven launches; three without a '
             'belief), NOT kernel time; median of single calls, 5 blocks of each alternated, median block; the torch '
             'composition is Tk rolls and R (Ta + Tb) = 576 shifted slice updates, 3 calls per block',
             caveat='launch_bytes counts every pass a launch makes over the 37.6 MB volume (12 with a belief); the belief, '
             'the votes and the two intermediates together fit the 256 MB Infinity Cache, so the passes need not come '
             'from HBM: the fraction relates the launch bytes of one call to the HBM peak, whatever served them')
  emit_json(res)


def vote_smooth_c4(iters):
  """One backward smoothing step at the C4 vote volume: vote_filter_c4's shape, taps and data recipe, `next` one
  filter step further than the belief (so beliefs and taps belong together: log_norm is 0 up to rounding).  Whole
  ops.vote_smooth calls with whole ops.vote_filter calls measured alongside, blocks of the two alternated, medians of
  single calls.  One JSON line; `json=<path>` as a third argument also writes it."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import geometry, grids
  R, H, scale, eps = 36, 256, 8.0, 1e-3
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  keep = (ov[:, None] * ov[None, :] > 0.05 * H * H)[None]
  frames = [torch.where(keep, torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25, float('-inf')).contiguous()
            for _ in range(2)]
  step = geometry.Transform2D(torch.tensor(np.deg2rad(5.0)), torch.tensor([0.93, 0.37], dtype=torch.float64))
  taps = pev.motion_taps(step, grid, R, 0.2, np.deg2rad(2.0), device='cuda')
  Tk, Ta, Tb = taps[0].shape[0], taps[2].shape[1], taps[3].shape[1]
  assert (Tk, Ta, Tb) == (4, 8, 8), (Tk, Ta, Tb)
  belief = pev.filter_votes(None, frames[0], None, grid, R, 0.2, np.deg2rad(2.0), temperature=scale)['belief']
  votes = frames[1]
  nxt, f_stats, _ = ops.vote_filter(belief, votes, taps, scale, eps)
  out, stats, count = ops.vote_smooth(belief, nxt, taps, eps)
  fin = torch.isfinite(out)
  total = float(out[fin].double().exp().sum())
  assert torch.equal(fin, torch.isfinite(belief)) and int(count[0]) == int(fin.sum()) and int(count[1]) == 0
  assert abs(float(stats[0])) < 1e-4 and abs(total - 1) < 1e-4, (float(stats[0]), total)
  assert float(stats[1]) == float(f_stats[1])               # the filter's mass_kept of that step, the same bits
  smooth = lambda: ops.vote_smooth(belief, nxt, taps, eps)
  filt = lambda: ops.vote_filter(belief, votes, taps, scale, eps)
  (k_ms, ks), (f_ms, fs) = alternated_blocks(((smooth, 5, max(iters, 5)), (filt, 5, max(iters, 5))))
  n = R * Ho * Wo
  by, by_f = 4.0 * n * 22, 4.0 * n * 12   # the headers of vote_smooth.hip / vote_filter.hip: passes over the volume
  hbm_peak = 8.0e12                # B/s, the MI355X's HBM3E peak
  res = dict(case='vote_smooth_c4', shape=[R, Ho, Wo], taps=[Tk, Ta, Tb], uniform_mix=eps,
             cells_with_ratio_mass=int(count[3]), mass_kept=round(float(stats[1]), 6), log_norm=float(stats[0]),
             call_ms=round(k_ms, 4), call_ms_blocks=[round(v, 4) for v in ks],
             filter_call_ms=round(f_ms, 4), filter_call_ms_blocks=[round(v, 4) for v in fs],
             ratio_to_filter_call=round(k_ms / f_ms, 2), launch_bytes=int(by),
             call_GBps_of_launch_bytes=round(by / k_ms / 1e6, 1),
             filter_launch_bytes=int(by_f), filter_call_GBps_of_launch_bytes=round(by_f / f_ms / 1e6, 1),
             call_fraction_of_hbm_peak=round(by / (k_ms * 1e-3) / hbm_peak, 3), hbm_peak_Bps=hbm_peak,
             timing='call_ms = one whole ops.vote_smooth call between device events on an idle stream (its four '
             'torch.empty allocations, the ctypes call and the eleven launches), NOT kernel time; filter_call_ms the '
             'same for ops.vote_filter (seven launches) in the same process; median of single calls, 5 blocks of each '
             'alternated, median block',
             caveat='launch_bytes counts every pass a launch makes over the 37.6 MB volume (22; the filter 12); the '
             'volumes of a call together fit the 256 MB Infinity Cache, so the passes need not come from HBM: the '
             'fraction relates the launch bytes of one call to the HBM peak, whatever served them')
  emit_json(res)


def vote_refine_c4(iters):
  """Peak refinement at the C4 planes (256^2 cells, D = 32, R = 36, 16 peaks x the default 11 x 9 x 9 lattice = 14 256
  poses; 10 % / 5 % invalid cells): whole ops.plane_align_score calls, median of single calls, against the only way to
  get the same scores without the kernel: one ops.interpolate_nd of the map at the query cells' positions and a torch
  reduction PER POSE, timed on a subset of the poses and scaled to all of them.  One JSON line; `json=<path>` as a
  third argument also writes it."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import grids
  H, D, R, K = 256, 32, 36, 16
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  fq = torch.randn((H, H, D), device='cuda', generator=g)
  fm = torch.randn((H, H, D), device='cuda', generator=g)
  vq = torch.rand((H, H), device='cuda', generator=g) > 0.10
  vm = torch.rand((H, H), device='cuda', generator=g) > 0.05
  rng = np.random.default_rng(0)
  index = torch.tensor(np.stack([rng.integers(0, R, K), rng.integers(H - 41, H + 40, K), rng.integers(H - 41, H + 40, K)],
                                -1).astype(np.int32), device='cuda')
  cont, poses = pev.refine_lattice(index, grid, R, (H, H))
  P = poses.shape[0]
  thr = 0.05 * H * H
  score, overlap = ops.plane_align_score(fq, vq, fm, vm, poses, thr)
  ii, jj = torch.meshgrid(torch.arange(H, device='cuda') + 0.5, torch.arange(H, device='cuda') + 0.5, indexing='ij')
  fq_rows, tcount = fq.reshape(-1, D), vq.sum()

  def composed(rows):
    out = []
    for c, s, tx, ty in rows:
      pts = torch.stack(((c * ii - s * jj) + tx, (s * ii + c * jj) + ty), -1).reshape(-1, 2)
      values, valid = ops.interpolate_nd(fm, pts, vm)
      ok = valid & vq.reshape(-1)
      raw = torch.where(ok, (fq_rows * values).sum(-1), 0.0).sum(dtype=torch.float64)
      out.append(torch.where(ok.sum() > thr, (raw / tcount).float(), float('-inf')))
    return torch.stack(out)

  sub = list(range(0, P, P // 32))[:32]
  sub_rows = [tuple(poses[i]) for i in sub]
  t_score = composed(sub_rows)
  k_sub = score[torch.tensor(sub, device='cuda')]
  fin = torch.isfinite(t_score)
  assert torch.equal(fin, torch.isfinite(k_sub)) and bool(fin.any())
  err = float((t_score[fin] - k_sub[fin]).abs().max())
  assert err < 1e-4, err
  kernel = lambda: ops.plane_align_score(fq, vq, fm, vm, poses, thr)
  compo = lambda: composed(sub_rows)
  (k_ms, ks), (t_ms, ts) = alternated_blocks(((kernel, 2, max(iters, 3)), (compo, 2, 3)), blocks=3)
  t_ms *= P / len(sub)
  flop = 2.0 * 4 * P * H * H * D
  res = dict(case='vote_refine_c4', query=[H, H, D], map=[H, H, D], rotations=R, peaks=K, lattice=[11, 9, 9], poses=P,
             valid_fraction=[round(float(vq.float().mean()), 4), round(float(vm.float().mean()), 4)],
             finite_scores=int(torch.isfinite(score).sum()), mean_overlap=round(float(overlap.float().mean()), 1),
             call_ms=round(k_ms, 3), call_ms_blocks=[round(v, 3) for v in ks], flop=flop,
             call_TFLOPs=round(flop / (k_ms * 1e-3) / 1e12, 3),
             interpolate_loop_ms_scaled=round(t_ms, 1), interpolate_loop_poses_timed=len(sub),
             interpolate_loop_ms_per_pose=round(t_ms / P, 4), speedup=round(t_ms / k_ms, 1),
             max_abs_difference_to_loop=err,
             timing='call_ms = one whole ops.plane_align_score call between device events on an idle stream (its three '
             'torch.empty allocations, the ctypes call and the three launches), NOT kernel time; median of single calls, '
             '3 blocks alternated with the loop, median block; flop = 2 * 4 * P * Hq * Wq * D counts every query cell '
             'of every pose, counted or not; the loop is timed on every (P / 32)-th pose and scaled by P / 32')
  emit_json(res)


def vote_modes_c4(iters):
  """The modes of the C4 vote volume (R = 36, 511 x 511, the low-overlap border -inf; K = 16 peaks of ops.vote_peaks,
  window (2, 16): ~9e4 cells, so the call is launch-bound): whole ops.vote_modes calls beside whole ops.vote_posterior
  and ops.vote_peaks calls on the same votes, blocks alternated, medians of single calls.  One JSON line; `json=<path>`
  as a third argument also writes it to that file."""
  R, H, scale, K, win_r, win_xy = 36, 256, 8.0, 16, 2, 16
  Ho = Wo = 2 * H - 1
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  peaks = ops.vote_peaks(votes, K, 2, 4)[0]
  stats, count = ops.vote_modes(votes, peaks, win_r, win_xy, scale)
  log_z = ops.vote_posterior(votes, scale)[2][0]
  weight = (stats[:, 0].double() - log_z.double()).exp()
  assert bool((count[:, 0] > 0).all()) and bool(torch.isfinite(stats[:, :11]).all()) and 0 < float(weight.sum()) <= 1
  modes = lambda: ops.vote_modes(votes, peaks, win_r, win_xy, scale)
  post = lambda: ops.vote_posterior(votes, scale)
  pk = lambda: ops.vote_peaks(votes, K, 2, 4)
  n = max(iters, 5)
  (m_ms, ms), (p_ms, ps), (k_ms, ks) = alternated_blocks(((modes, 5, n), (post, 5, n), (pk, 5, n)))
  cells = int(count.sum())
  res = dict(case='vote_modes_c4', shape=[R, Ho, Wo], K=K, window=[win_r, win_xy], scale=scale, owned_cells=cells,
             mass_in_modes=round(float(weight.sum()), 6), vote_modes_call_ms=round(m_ms, 4),
             vote_modes_call_ms_blocks=[round(v, 4) for v in ms], vote_posterior_call_ms=round(p_ms, 4),
             vote_posterior_call_ms_blocks=[round(v, 4) for v in ps], vote_peaks_call_ms=round(k_ms, 4),
             vote_peaks_call_ms_blocks=[round(v, 4) for v in ks],
             timing='whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the launches) between '
             'device events on an idle stream, NOT kernel time; median of single calls, 5 blocks of each alternated, '
             'median block; no threshold is set on this case')
  emit_json(res)


def vote_recall_c4(iters):
  """The expected recall of the C4 vote volume (R = 36, 511 x 511, the low-overlap border -inf; the reference's three
  threshold pairs (0.5 m, 1 deg), (1 m, 2 deg), (2 m, 4 deg) at 0.25 m cells and 10 degree bins = rho2 (3, 15, 63),
  half_r 0; K = 16 peaks of ops.vote_peaks as centres): whole ops.vote_recall calls, without and with the maps, beside
  whole ops.vote_posterior calls on the same votes, blocks alternated, medians of single calls.  One JSON line;
  `json=<path>` as a third argument also writes it to that file."""
  R, H, scale, K = 36, 256, 8.0, 16
  rho2, half_r = (3, 15, 63), (0, 0, 0)
  Ho = Wo = 2 * H - 1
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  peaks = ops.vote_peaks(votes, K, 2, 4)[0]
  best_index, best_lm, centre_lm, _, stats, count, _ = ops.vote_recall(votes, rho2, half_r, peaks, scale)
  log_z = ops.vote_posterior(votes, scale)[2][0]
  assert abs(float(stats[0]) - float(log_z)) <= 1e-4 * abs(float(log_z)) and int(count[0]) > 0
  assert bool((best_index >= 0).all()) and bool((best_lm <= 0).all()) and bool((best_lm[1:] >= best_lm[:-1]).all())
  assert bool((centre_lm <= best_lm[None] + 1e-6).all()) and bool(torch.isfinite(centre_lm).all())
  recall = lambda: ops.vote_recall(votes, rho2, half_r, peaks, scale)
  with_maps = lambda: ops.vote_recall(votes, rho2, half_r, peaks, scale, maps=True)
  post = lambda: ops.vote_posterior(votes, scale)
  n = max(iters, 5)
  (r_ms, rs), (m_ms, ms), (p_ms, ps) = alternated_blocks(((recall, 3, n), (with_maps, 3, n), (post, 3, n)))
  res = dict(case='vote_recall_c4', shape=[R, Ho, Wo], K=K, rho2=list(rho2), half_r=list(half_r), scale=scale,
             best_recall=[round(float(v), 6) for v in best_lm.exp()], vote_recall_call_ms=round(r_ms, 4),
             vote_recall_call_ms_blocks=[round(v, 4) for v in rs], vote_recall_maps_call_ms=round(m_ms, 4),
             vote_recall_maps_call_ms_blocks=[round(v, 4) for v in ms], vote_posterior_call_ms=round(p_ms, 4),
             vote_posterior_call_ms_blocks=[round(v, 4) for v in ps], ratio_to_vote_posterior=round(r_ms / p_ms, 2),
             workspace_bytes=int(ops._lib.load().snap_vote_recall_workspace_bytes(R, Ho, Wo, K, len(rho2))),
             timing='whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the launches) between '
             'device events on an idle stream, NOT kernel time; median of single calls, 5 blocks of each alternated, '
             'median block; no threshold is set on this case')
  emit_json(res)


def vote_odometry_c4(iters):
  """The increment posterior at the C4 vote volume (R = 36, 511 x 511, the low-overlap border -inf; prev = the belief
  of one filter step at temperature 8, cur = the next frame's votes at scale 8: every unmasked cell carries mass, the
  dense case in which no tile is skipped; Kr = 2, S = 16, U = 5 x 33 x 33 candidates with one (k, i, j) for all
  rotations): whole ops.vote_odometry calls beside whole ops.vote_filter calls (Tk = 4, Ta = Tb = 8) on the same
  volumes, blocks alternated, medians of single calls.  One JSON line; `json=<path>` as a third argument also writes it
  to that file."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import geometry, grids
  R, H, scale, Kr, S = 36, 256, 8.0, 2, 16
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  keep = (ov[:, None] * ov[None, :] > 0.05 * H * H)[None]
  frames = [torch.where(keep, torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25, float('-inf')).contiguous()
            for _ in range(2)]
  belief = pev.filter_votes(None, frames[0], None, grid, R, 0.2, np.deg2rad(2.0), temperature=scale)['belief']
  votes = frames[1]
  k, i, j = torch.meshgrid(torch.arange(-Kr, Kr + 1), torch.arange(-S, S + 1), torch.arange(-S, S + 1), indexing='ij')
  rows = torch.stack((k.reshape(-1), i.reshape(-1), j.reshape(-1)), -1).to(torch.int32)
  shifts = rows[:, None, :].expand(-1, R, -1).contiguous().cuda()
  U = int(shifts.shape[0])
  log_table, log_evidence, best, stats, count = ops.vote_odometry(belief, votes, Kr, S, shifts, 1.0, scale)
  assert U == 5 * 33 * 33 and int(count[4]) == 0 and int(count[5]) == U and bool((log_table <= 0).all())
  # candidate u sums its table entry over the rotations
  want = torch.logsumexp(log_table.double(), 1).reshape(-1)
  assert float((log_evidence.double() - want).abs().max()) < 1e-5 and int(best[0]) == int(log_evidence.argmax())
  step = geometry.Transform2D(torch.tensor(np.deg2rad(5.0)), torch.tensor([0.93, 0.37], dtype=torch.float64))
  taps = pev.motion_taps(step, grid, R, 0.2, np.deg2rad(2.0), device='cuda')
  odo = lambda: ops.vote_odometry(belief, votes, Kr, S, shifts, 1.0, scale)
  flt = lambda: ops.vote_filter(belief, votes, taps, scale, 1e-3)
  n = max(iters, 3)
  (o_ms, os_), (f_ms, fs) = alternated_blocks(((odo, 3, n), (flt, 3, n)))
  W = 2 * S + 1
  fma_nominal = R * Ho * Wo * (2 * Kr + 1) * W * W           # every cell of cur against its whole window
  fma_mass = int(count[2]) * (2 * Kr + 1) * W * W            # the cells of cur with mass: the fmas that are issued
  peak = 78.6e12 / 2                                         # MI355X float64 vector peak, 78.6 TFLOP/s = 39.3e12 fma/s
  res = dict(case='vote_odometry_c4', shape=[R, Ho, Wo], Kr=Kr, S=S, U=U, scale=scale,
             cells_with_mass=[int(count[0]), int(count[2])], vote_odometry_call_ms=round(o_ms, 3),
             vote_odometry_call_ms_blocks=[round(v, 3) for v in os_], vote_filter_call_ms=round(f_ms, 4),
             vote_filter_call_ms_blocks=[round(v, 4) for v in fs], ratio_to_vote_filter=round(o_ms / f_ms, 1),
             f64_fma_nominal=fma_nominal, f64_fma_on_cells_with_mass=fma_mass,
             share_of_f64_vector_peak=round(fma_mass / (o_ms * 1e-3) / peak, 4),
             workspace_bytes=int(ops._lib.load().snap_vote_odometry_workspace_bytes(R, Ho, Wo, Kr, S, U)),
             timing='whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the six launches) between '
             'device events on an idle stream, NOT kernel time; median of single calls, 5 blocks of each alternated, '
             'median block; the share counts the fmas on cells of cur with mass against 39.3e12 float64 fma/s (the '
             '78.6 TFLOP/s vector peak of the data sheet); untuned; no threshold is set on this case')
  emit_json(res)


def vote_rebase_c4(iters):
  """A change of map frame at the C4 vote volume (R = 36, 511 x 511, the low-overlap border -inf; a turn of 0.37 rad
  about the map centre with a fractional translation: fractional dk, every tile's footprint turned): whole
  ops.rebase_volume calls beside whole ops.vote_posterior calls on the same votes, blocks alternated, medians of single
  calls.  One JSON line; `json=<path>` as a third argument also writes it to that file."""
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import geometry, grids
  R, H, scale = 36, 256, 8.0
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  new_t_old = geometry.Transform2D(torch.tensor(0.37, dtype=torch.float64), torch.tensor([9.13, -6.47], dtype=torch.float64))
  table = pev.rebase_table(new_t_old, grid, R)
  dst, stats, count = ops.rebase_volume(votes, table, scale)
  log_z = ops.vote_posterior(votes, scale)[2][0]
  assert table[0] % 1 != 0 and abs(float(stats[0]) - float(log_z)) <= 1e-4 * abs(float(log_z))
  assert 0.5 < float(stats[1]) < 1.05 and int(count[1]) == 0 and int(count[3]) > 0
  assert abs(float(dst[torch.isfinite(dst)].double().exp().sum()) - 1) < 1e-5
  rebase = lambda: ops.rebase_volume(votes, table, scale)
  post = lambda: ops.vote_posterior(votes, scale)
  n = max(iters, 5)
  (r_ms, rs), (p_ms, ps) = alternated_blocks(((rebase, 5, n), (post, 5, n)))
  by = 4.0 * votes.numel() * 5       # vote_rebase.hip's header: about 5 passes over the volume (an estimate)
  res = dict(case='vote_rebase_c4', shape=[R, Ho, Wo], scale=scale, phi=0.37, dk=round(table[0], 6),
             offset_cells=[round(float(v), 4) for v in table[2]], mass_kept=round(float(stats[1]), 6),
             cells_not_covered=int(count[3]), vote_rebase_call_ms=round(r_ms, 4),
             vote_rebase_call_ms_blocks=[round(v, 4) for v in rs], vote_posterior_call_ms=round(p_ms, 4),
             vote_posterior_call_ms_blocks=[round(v, 4) for v in ps], ratio_to_vote_posterior=round(r_ms / p_ms, 2),
             estimated_bytes=by, effective_bytes_per_s=round(by / (r_ms * 1e-3), 1),
             workspace_bytes=int(ops._lib.load().snap_vote_rebase_workspace_bytes(R, Ho, Wo)),
             timing='whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the four launches) between '
             'device events on an idle stream, NOT kernel time; median of single calls, 5 blocks of each alternated, '
             'median block; the time is measured, the bytes are the 5 n-cell ESTIMATE of the kernel file\'s header (HBM '
             'traffic was not measured), so effective_bytes_per_s is measured time against estimated traffic; no '
             'threshold is set on this case')
  emit_json(res)


def vote_temper_c4(iters):
  """The temperature ladder at the C4 vote volume (R = 36, 511 x 511, the low-overlap border -inf; 16 scales from 2^-2 to
  2^2): one whole ops.temper_volume call beside the 16 whole ops.vote_posterior calls on the same votes that it replaces
  (one per scale), blocks alternated, medians of single calls (one "call" of the second is all 16).  One JSON line;
  `json=<path>` as a third argument also writes it to that file."""
  R, H, S = 36, 256, 16
  Ho = Wo = 2 * H - 1
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  scales = [2.0 ** (-2 + 4 * i / (S - 1)) for i in range(S)]
  table, stats, count = ops.temper_volume(votes, scales)
  post = [ops.vote_posterior(votes, s)[2] for s in scales]
  diff = max(max(abs(float(table[l, 0]) - float(post[l][0])), abs(float(table[l, 3]) - float(post[l][11])))
             for l in range(S))
  assert diff < 1e-3 and int(count[1]) == 0, diff
  temper = lambda: ops.temper_volume(votes, scales)
  def posteriors():
    for s in scales:
      ops.vote_posterior(votes, s)
  n = max(iters, 5)
  (t_ms, ts), (p_ms, ps) = alternated_blocks(((temper, 5, n), (posteriors, 5, n)))
  by = 4.0 * votes.numel()
  res = dict(case='vote_temper_c4', shape=[R, Ho, Wo], scales=[round(s, 6) for s in scales], S=S,
             masked_fraction=round(1 - int(count[0]) / votes.numel(), 4), vote_temper_call_ms=round(t_ms, 4),
             vote_temper_call_ms_blocks=[round(v, 4) for v in ts], vote_posterior_x16_ms=round(p_ms, 4),
             vote_posterior_x16_ms_blocks=[round(v, 4) for v in ps], ratio_temper_to_posterior_x16=round(t_ms / p_ms, 4),
             block_ranges_overlap=bool(max(ts) >= min(ps)), volume_bytes=int(by),
             exponentials_per_s=round(S * int(count[0]) / (t_ms * 1e-3), 1),
             max_abs_difference_to_vote_posterior=diff,
             workspace_bytes=int(ops._lib.load().snap_vote_temper_workspace_bytes(R, Ho, Wo, S)),
             timing='whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the three launches; for '
             'vote_posterior all of that 16 times) between device events on an idle stream, NOT kernel time; median of '
             'single calls, 5 blocks of each alternated, median block; the 37.6 MB volume fits the 256 MB Infinity Cache, '
             'so repeated reads need not come from HBM; no threshold is set on this case')
  emit_json(res)


def vote_prior_c4(iters):
  """A GNSS / compass prior fused into the C4 vote volume (R = 36, 511 x 511, the low-overlap border -inf) with M = 1 and
  M = 8 components and a sensor off the grid centre: one whole ops.prior_volume call beside the same normalised volume
  composed from what the library offered before (torch broadcasting for the log-prior from the same table, an add,
  ops.vote_posterior for the normaliser, a subtraction), blocks alternated, medians of single calls.  One JSON line;
  `json=<path>` as a third argument also writes it to that file."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import grids
  R, H, scale = 36, 256, 8.0
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  rng = np.random.default_rng(0)
  res = dict(case='vote_prior_c4', shape=[R, Ho, Wo], scale=scale)
  for M in (1, 8):
    pos = 25.6 + rng.uniform(-8.0, 8.0, (M, 2))
    cov = np.stack([np.array([[4.0, 1.0], [1.0, 9.0]]) * rng.uniform(0.5, 2.0) for _ in range(M)])
    prior = pev.pose_prior(grid, R, position=pos, covariance=cov, heading=rng.uniform(-3, 3, M),
                           concentration=np.full(M, 4.0), weights=rng.uniform(0.5, 1.0, M), sensor_q=[27.0, 24.9])
    n = torch.tensor(prior.centres, device='cuda').float()
    f = torch.tensor(prior.planes, device='cuda')
    P = torch.tensor(prior.comps, device='cuda')
    a = torch.arange(Ho, device='cuda').float()[None, None, :, None]
    b = torch.arange(Wo, device='cuda').float()[None, None, None, :]

    def composed():
      da = (a - n[:, :, 0, None, None]) - f[:, :, 0, None, None]
      db = (b - n[:, :, 1, None, None]) - f[:, :, 1, None, None]
      q = (P[:, 0, None, None, None] * da * da + 2 * P[:, 1, None, None, None] * da * db
           + P[:, 2, None, None, None] * db * db)
      u = torch.logsumexp((P[:, 3, None] + f[:, :, 2])[:, :, None, None] - 0.5 * q, 0)
      t = scale * votes + u
      return t - ops.vote_posterior(t, 1.0)[2][0]
    fused = lambda: ops.prior_volume(votes, prior, scale)
    out, want = fused()[0], composed()
    fin = torch.isfinite(want)
    diff = float((out[fin] - want[fin]).abs().max())
    assert bool((torch.isfinite(out) == fin).all()) and diff < 1e-3, diff
    k = max(iters, 5)
    (p_ms, ps), (c_ms, cs) = alternated_blocks(((fused, 5, k), (composed, 5, k)))
    res[f'M{M}'] = dict(vote_prior_call_ms=round(p_ms, 4), vote_prior_call_ms_blocks=[round(v, 4) for v in ps],
                        composed_ms=round(c_ms, 4), composed_ms_blocks=[round(v, 4) for v in cs],
                        ratio_prior_to_composed=round(p_ms / c_ms, 4), block_ranges_overlap=bool(max(ps) >= min(cs)),
                        max_abs_difference=diff,
                        effective_bytes_per_s=round(8.0 * votes.numel() / (p_ms * 1e-3), 1),
                        workspace_bytes=int(ops._lib.load().snap_vote_prior_workspace_bytes(R, Ho, Wo, M)))
  res['timing'] = ('whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the four launches; for the '
                   'composition its torch kernels, their temporaries and one ops.vote_posterior call) between device '
                   'events on an idle stream, NOT kernel time; median of single calls, 5 blocks of each alternated, '
                   'median block; effective_bytes_per_s counts one read and one write of the volume against the '
                   'measured call time (the 37.6 MB volume fits the 256 MB Infinity Cache); no threshold is set on '
                   'this case')
  emit_json(res)


def vote_raster(iters):
  """A road / lane raster prior (256 x 256 cells) fused into the C4 vote volume (R = 36, 511 x 511, the low-overlap border
  -inf): one whole ops.raster_volume call with S = 1 and S = 8 strengths, a centred sensor (one tap per cell) and an
  off-centre one (four taps), each beside one whole ops.prior_volume call with M = 1 on the same volume, blocks
  alternated, medians of single calls.  One JSON line; `json=<path>` as a third argument also writes it to that file."""
  import numpy as np
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import grids
  R, H, scale = 36, 256, 8.0
  Ho = Wo = 2 * H - 1
  grid = grids.Grid2D((H, H), 0.2)
  g = torch.Generator(device='cuda').manual_seed(0)
  votes = torch.randn((R, Ho, Wo), device='cuda', generator=g) * 0.25
  ov = (H - (torch.arange(Ho, device='cuda') - (H - 1)).abs()).float()
  votes = torch.where((ov[:, None] * ov[None, :] > 0.05 * H * H)[None], votes, float('-inf')).contiguous()
  rng = np.random.default_rng(0)
  gps = pev.pose_prior(grid, R, position=[27.0, 24.0], covariance=[[4.0, 1.0], [1.0, 9.0]], heading=0.3,
                       concentration=4.0, sensor_q=[27.0, 24.9])
  area = -6.0 * rng.random((H, H))
  lanes = rng.uniform(-np.pi, np.pi, (H, H))
  valid = rng.random((H, H)) > 0.02
  ladders = {1: (1.0,), 8: tuple(2.0 ** (i - 4) for i in range(8))}
  prior_call = lambda: ops.prior_volume(votes, gps, scale)
  res = dict(case='vote_raster', shape=[R, Ho, Wo], raster=[H, H], scale=scale)
  k = max(iters, 5)
  for taps, sensor in ((1, None), (4, [27.0, 24.9])):
    for S in (1, 8):
      ras = pev.raster_prior(grid, R, log_area=area, valid=valid, heading=lanes, concentration=4.0, sensor_q=sensor,
                             strengths=ladders[S])
      assert int((ras.planes[:, :2] != 0).any(1).sum()) == (0 if taps == 1 else R)
      call = lambda: ops.raster_volume(votes, ras, scale)
      out, table, _, count = call()
      lse = float(torch.logsumexp(out.double().reshape(-1), 0))
      assert abs(lse) < 1e-3 and bool(torch.isfinite(table[:, 0]).all()), (lse, table)
      (r_ms, rs), (p_ms, ps) = alternated_blocks(((call, 5, k), (prior_call, 5, k)))
      nbytes = 8.0 * votes.numel() + ras.raster.nbytes
      res[f'taps{taps}_S{S}'] = dict(
          vote_raster_call_ms=round(r_ms, 4), vote_raster_call_ms_blocks=[round(v, 4) for v in rs],
          vote_prior_M1_call_ms=round(p_ms, 4), vote_prior_M1_call_ms_blocks=[round(v, 4) for v in ps],
          ratio_raster_to_prior_M1=round(r_ms / p_ms, 4), block_ranges_overlap=bool(max(ps) >= min(rs)),
          raster_bytes_per_ms=round(nbytes / r_ms, 1), prior_bytes_per_ms=round(8.0 * votes.numel() / p_ms, 1),
          cells_excluded_by_the_raster=int(count[2]),
          workspace_bytes=int(ops._lib.load().snap_vote_raster_workspace_bytes(R, Ho, Wo, H, H, S)))
  res['timing'] = ('whole wrapper calls (torch.empty outputs and workspace, the ctypes call, the four launches) between '
                   'device events on an idle stream, NOT kernel time; median of single calls, 5 blocks of each '
                   'alternated, median block; bytes_per_ms counts one read and one write of the volume (and one read of '
                   'the raster) against the measured call time (the 37.6 MB volume fits the 256 MB Infinity Cache); no '
                   'threshold is set on this case')
  emit_json(res)


if __name__ == '__main__':
  which = sys.argv[1] if len(sys.argv) > 1 else 'pose_score'
  iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
  {'pose_score': pose_score, 'pose_score_c4': pose_score_c4, 'voting_c4': voting_c4,
   'vote_peaks_c4': vote_peaks_c4, 'vote_posterior_c4': vote_posterior_c4, 'vote_fuse_c4': vote_fuse_c4,
   'vote_filter_c4': vote_filter_c4, 'vote_smooth_c4': vote_smooth_c4,
   'vote_refine_c4': vote_refine_c4, 'vote_modes_c4': vote_modes_c4, 'vote_recall_c4': vote_recall_c4,
   'vote_odometry_c4': vote_odometry_c4, 'vote_rebase_c4': vote_rebase_c4, 'vote_temper_c4': vote_temper_c4,
   'vote_prior_c4': vote_prior_c4, 'vote_raster': vote_raster}[which](iters)
