"""Float64 restatement of the camera-ray lift (csrc/lift_common.h + the pooling of csrc/lift.hip),
planted scenes that sit ON its geometric edges, readout inputs, and the border-flip rule.

numpy only: no HIP, no oracle/ import.  ``lift(..., dtype=np.float64)`` is the reference;
``dtype=np.float32`` runs the same statements in the header's expression order (every +, -, *, /
and sqrt is one IEEE operation in both), so on the planted scenes -- whose geometry is exact in
f32 -- it gives the bits a correct kernel gives wherever no exp / log / atan is on the path.

Layouts: cam [B, V, 11] = wh f c k(3) max_fov tan(max_fov / 2); Rt [B, V, 12] = R(9) t(3);
points [B, N, 3]; f_images [B, V, h, w, fd (+ nb)].
"""
import os
import re

import numpy as np

EPS32 = np.float32(1e-3)      # the near plane, as the f32 constant the header holds
U = 2.0 ** -23                # one f32 rounding, relative (the issue's unit)
MARGIN = 8                    # as the pose-chain and attention tests
PX_TOL = 1e-4                 # helpers.assert_validity_mismatches_on_borders: pixels
DEPTH_TOL = 1e-6              # ... and depth at the near plane
CAP_SHARE = 0.01              # explained flips: at most 1 % of a scene's (voxel, view) pairs

MUTANTS = ('depth_gt_eps', 'x_le_w', 'tie_highest', 'select_ignores_vis', 'min_dist_lt', 'swap_clip',
           'bin_clamp_after_log', 'softmax_no_floor', 'one_pass_variance', 'minmax_over_invisible')


def library_limits():
  """(largest V, largest number of selected views) from lift_desc_validate, csrc/lift_common.h."""
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'snap_amd', 'csrc', 'lift_common.h')
  with open(path) as fh:
    text = fh.read()
  return (int(re.search(r'd\.V > (\d+)', text).group(1)),
          int(re.search(r'lift_nsel\(d\) > (\d+)', text).group(1)))


def ulp32(x):
  """One f32 ulp at |x| (as float64)."""
  a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
  a = np.where(np.isfinite(a), a, np.float32(1))
  return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


# ------------------------------- the restatement ----------------------------------------------
def project(cam, Rt, pts, fisheye, dtype=np.float64, mut=()):
  """lift_project for every (voxel, view): arrays [B, N, V]."""
  T = dtype
  cam = np.asarray(cam, np.float32).astype(T)[:, None]
  Rt = np.asarray(Rt, np.float32).astype(T)[:, None]
  p = np.asarray(pts, np.float32).astype(T)[:, :, None]
  eps = T(EPS32)
  px, py, pz = p[..., 0], p[..., 1], p[..., 2]
  pv = []
  for i in range(3):                                   # R^T (p - t) as t_inv + R^T p
    r0, r1, r2 = Rt[..., i], Rt[..., 3 + i], Rt[..., 6 + i]
    tinv = -((r0 * Rt[..., 9] + r1 * Rt[..., 10]) + r2 * Rt[..., 11])
    pv.append(tinv + ((r0 * px + r1 * py) + r2 * pz))
  depth = pv[2]
  valid = (depth > eps) if 'depth_gt_eps' in mut else (depth >= eps)
  z = np.maximum(depth, eps)
  x, y = pv[0] / z, pv[1] / z
  o = {}
  if fisheye:
    r2 = x * x + y * y
    in_center = r2 < eps * eps
    radius = np.sqrt(np.where(in_center, eps * eps, r2))
    theta = np.arctan(radius)
    t2 = theta * theta
    offset = (cam[..., 6] * t2 + cam[..., 7] * (t2 * t2)) + cam[..., 8] * (t2 * t2 * t2)
    fdist = np.where(in_center, T(1), (offset + T(1)) * theta / radius)
    x, y = x * fdist, y * fdist
    valid = valid & (in_center | ((radius < cam[..., 10]) & (fdist > 0)))
    o.update(radius=np.sqrt(r2), fdist=fdist, fov_lim=np.broadcast_to(cam[..., 10], r2.shape))
  x = x * cam[..., 2] + cam[..., 4]
  y = y * cam[..., 3] + cam[..., 5]
  wlim, hlim = cam[..., 0], cam[..., 1]
  x_in = (x >= 0) & ((x <= wlim) if 'x_le_w' in mut else (x < wlim))
  valid = valid & x_in & (y >= 0) & (y < hlim)
  dx, dy, dz = px - Rt[..., 9], py - Rt[..., 10], pz - Rt[..., 11]
  dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
  o.update(pi=y, pj=x, depth=depth, dist=dist, vis=valid, vx=pv[0], vy=pv[1],
           wlim=np.broadcast_to(wlim, x.shape), hlim=np.broadcast_to(hlim, x.shape))
  return o


def select(dist, vis, K, mut=()):
  """lift_select_halfwave: sel [B, N, S] (the S = K nearest visible views, ties to the lowest index;
  K = 0: all views in index order), min_dist [B, N] = the nearest visible distance."""
  B, N, V = dist.shape
  key = np.where(vis, dist, np.inf)
  min_dist = key.min(-1)
  if K == 0:
    return np.broadcast_to(np.arange(V), (B, N, V)).copy(), min_dist
  if 'select_ignores_vis' in mut:
    key = dist
  if 'tie_highest' in mut:
    sel = V - 1 - np.argsort(key[..., ::-1], axis=-1, kind='stable')[..., :K]
  else:
    sel = np.argsort(key, axis=-1, kind='stable')[..., :K]
  return sel, min_dist


def taps(pi, pj, h, w, selective, dtype=np.float64):
  """lift_taps: selective (K > 0) clips the point, otherwise each tap index is clipped."""
  T = dtype
  ci, cj = pi - T(0.5), pj - T(0.5)
  if selective:
    ci = np.maximum(np.minimum(ci, T(h - 1)), T(0))
    cj = np.maximum(np.minimum(cj, T(w - 1)), T(0))
  fi, fj = np.floor(ci), np.floor(cj)
  wi1, wj1 = ci - fi, cj - fj
  wi0, wj0 = T(1) - wi1, T(1) - wj1
  cl = lambda a, n: np.minimum(np.maximum(a, 0), n - 1).astype(np.int64)
  return dict(i0=cl(fi, h), i1=cl(fi + 1, h), j0=cl(fj, w), j1=cl(fj + 1, w), wi1=wi1, wj1=wj1,
              w00=wi0 * wj0, w01=wi0 * wj1, w10=wi1 * wj0, w11=wi1 * wj1, ci=ci, cj=cj)


def depth_bins(depth, depth_min_max, nb, dtype=np.float64, mut=()):
  """lift_depth_bins: clamp the depth, log-space coordinate c, bins b0, b1 and the weight of b1."""
  T = dtype
  dmin, dmax = T(np.float32(depth_min_max[0])), T(np.float32(depth_min_max[1]))
  span = np.log(dmax / dmin)
  late = 'bin_clamp_after_log' in mut        # the clamp moved from the depth to the bin index
  dc = np.maximum(depth, T(1e-30)) if late else np.minimum(np.maximum(depth, dmin), dmax)
  tt = np.log(dc / dmin) / span
  index = T(0.5) + tt * T(nb - 1)
  c = index - T(0.5)
  fl = np.floor(c)
  b0 = np.minimum(np.maximum(fl, 0), nb - 1).astype(np.int64)
  b1 = np.minimum(np.maximum(fl + 1, 0), nb - 1).astype(np.int64)
  wb1 = (c - b0.astype(T)) if late else (c - fl)
  return dict(b0=b0, b1=b1, wb1=wb1, c=c)


def pooled_channels(fd, weighted, use_variance, add_minmax):
  return fd * (1 + int(use_variance) + 2 * int(add_minmax)) + int(weighted)


def lift(f, cam, Rt, pts, *, K, fisheye, fd, nb, depth_min_max=(1.0, 2.0), max_view_distance=None, weighted=True,
         use_variance=True, add_minmax=False, dtype=np.float64, mut=(), obs_in=None):
  """The whole lift.  Returns a dict: the geometry of ``project`` ([B, N, V]), per slot ([B, N, S]):
  sel, ok, taps, bins, feat [B, N, S, fd], score; rows [B, N, stride] (mean | var? | max, min? |
  score_max?, zero padded to a multiple of 4), valid [B, N], obs [B, N, S, fd + 4] (features | log10
  depth | unit ray), and -- float64 only -- tol_rows / tol_obs, the first-order f32 bound of every
  element times MARGIN."""
  T = dtype
  f = np.asarray(f, np.float32).astype(T)
  B, V, h, w, C = f.shape
  pr = project(cam, Rt, pts, fisheye, T, mut)
  sel, min_dist = select(pr['dist'], pr['vis'], K, mut)
  S = sel.shape[-1]
  g = lambda a: np.take_along_axis(a, sel, -1)
  pi, pj, depth, ok = g(pr['pi']), g(pr['pj']), g(pr['depth']), g(pr['vis'])
  selective = (K > 0) != ('swap_clip' in mut)
  tp = taps(pi, pj, h, w, selective, T)
  bn = depth_bins(depth, depth_min_max, max(nb, 1), T, mut)
  bidx = np.arange(B)[:, None, None]
  a = [f[bidx, sel, tp[i], tp[j]] for i, j in (('i0', 'j0'), ('i0', 'j1'), ('i1', 'j0'), ('i1', 'j1'))]
  wt = [tp[k] for k in ('w00', 'w01', 'w10', 'w11')]
  blend = lambda ch: ((wt[0][..., None] * a[0][..., ch] + wt[1][..., None] * a[1][..., ch])
                      + wt[2][..., None] * a[2][..., ch]) + wt[3][..., None] * a[3][..., ch]
  okc = ok[..., None]
  with np.errstate(invalid='ignore', over='ignore'):
    feat = np.where(okc, blend(slice(0, fd)), T(0))
    if obs_in is not None:
      feat = np.where(okc, np.asarray(obs_in, np.float32).astype(T), T(0))
    absf = sum(np.abs(wt[t][..., None] * a[t][..., :fd]) for t in range(4))
    sumf = sum(np.abs(a[t][..., :fd] - a[0][..., :fd]) for t in range(1, 4))   # (the weights sum to one)
  out = dict(pr, sel=sel, ok=ok, min_dist=min_dist, taps=tp, bins=bn, feat=feat)
  # first-order f32 bounds (float64 run only): roundings of the blend, and of the coordinate that
  # the weights come from (projection: 16 roundings, 32 through the fisheye model; bins: 8)
  r_proj = 32 if fisheye else 16
  cmag = np.maximum(np.maximum(np.abs(pi), np.abs(pj)), 1.0)
  dw = r_proj * U * cmag                                               # |delta weight|
  tol_feat = np.where(okc, 10 * U * absf + dw[..., None] * sumf, 0.0)
  score = np.zeros(ok.shape, T)
  tol_score = np.zeros(ok.shape)
  out['score_exact'] = out['bins_exact'] = np.ones(ok.shape, bool)
  if weighted:
    take = lambda t, b: np.take_along_axis(a[t][..., fd:], b[..., None], -1)[..., 0]
    s0 = ((wt[0] * take(0, bn['b0']) + wt[1] * take(1, bn['b0'])) + wt[2] * take(2, bn['b0'])) + wt[3] * take(3, bn['b0'])
    s1 = ((wt[0] * take(0, bn['b1']) + wt[1] * take(1, bn['b1'])) + wt[2] * take(2, bn['b1'])) + wt[3] * take(3, bn['b1'])
    wb1 = bn['wb1']
    wb0 = T(1) - wb1
    score = np.where(ok, wb0 * s0 + wb1 * s1, T(0))
    as0 = sum(np.abs(wt[t] * take(t, bn['b0'])) for t in range(4))
    as1 = sum(np.abs(wt[t] * take(t, bn['b1'])) for t in range(4))
    sabs = sum(np.abs(take(t, bn['b0'])) + np.abs(take(t, bn['b1'])) for t in range(4))
    ss = sum(np.abs(take(t, bn['b0']) - take(0, bn['b0'])) + np.abs(take(t, bn['b1']) - take(0, bn['b1'])) for t in range(1, 4))
    dwb = 8 * U * np.maximum(np.abs(bn['c']), 1.0)
    tol_score = np.where(ok, 13 * U * (np.abs(wb0) * as0 + np.abs(wb1) * as1) + dw * ss + dwb * np.abs(s1 - s0), 0.0)
    # where the score is free of log: the clamp ends (log(1) = 0, log(a) / log(a) = 1) and all-zero score taps
    dmin, dmax = np.float32(depth_min_max[0]), np.float32(depth_min_max[1])
    out['bins_exact'] = ~ok | (depth <= T(dmin)) | (depth >= T(dmax))
    out['score_exact'] = out['bins_exact'] | (sabs == 0)
  out['score'] = score
  nok = ok.sum(-1)
  anyv = nok > 0
  cnt = np.maximum(nok, 1).astype(T)[..., None]
  mean = np.zeros(feat.shape[:2] + (fd,), T)
  var = np.zeros_like(mean)
  tol_mean = np.zeros(mean.shape)
  tol_var = np.zeros(mean.shape)
  smax = np.zeros(nok.shape, T)
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    if weighted:
      sm = np.where(ok, score, -np.inf)
      smax = np.where(anyv, sm.max(-1), T(0))
      m = sm.max(-1) if 'softmax_no_floor' in mut else np.maximum(sm.max(-1), T(0))
      m = np.where(anyv, m, T(0))
      e = np.where(ok, np.exp(np.where(ok, score, T(0)) - m[..., None]), T(0))
      den = np.zeros(nok.shape, T)
      for r in range(S):
        den = den + e[..., r]
      wgt = e / np.where(anyv, den, T(1))[..., None]
      # relative bound of a weight: the scores it depends on, exp of a rounded argument, the sum
      rel_w = 2 * tol_score.max(-1)[..., None] + U * (np.abs(np.where(ok, score, 0) - m[..., None]) + 4 + S + 1)
      # ... and absolutely, only where exp(score - m) falls below the smallest normal f32 (score - m < -87): that
      # term may be lost altogether.  With the 0 floor and scores >= -80 this needs a view 87 below the row's best.
      under = ok & (np.where(ok, score, T(0)) - m[..., None] < -87)
      abs_w = np.where(under, 2.0 ** -126 / np.where(anyv, den, 1.0)[..., None].astype(np.float64), 0.0)
    else:
      wgt = np.where(ok, T(1), T(0))
      rel_w = np.full(ok.shape, 2 * U)
      abs_w = np.zeros(ok.shape)
    for r in range(S):
      mean = mean + wgt[..., r, None] * feat[..., r, :]
    if not weighted:
      mean = mean / cnt
    absm = np.zeros(mean.shape)
    for r in range(S):
      wr = np.abs(wgt[..., r, None]) / (1 if weighted else cnt)
      tol_mean += wr * tol_feat[..., r, :] + (wr * rel_w[..., r, None] + abs_w[..., r, None]) * np.abs(feat[..., r, :])
      absm += wr * np.abs(feat[..., r, :])
    tol_mean += (S + 1) * U * absm
    if 'one_pass_variance' in mut:
      ex2 = np.zeros_like(mean)
      for r in range(S):
        ex2 = ex2 + wgt[..., r, None] * (feat[..., r, :] * feat[..., r, :])
      var = (ex2 / cnt if not weighted else ex2) - mean * mean
    else:
      for r in range(S):
        dl = np.where(okc[..., r, :], feat[..., r, :] - mean, T(0))
        var = var + wgt[..., r, None] * (dl * dl)
      if not weighted:
        var = var / cnt
    absv = np.zeros(mean.shape)
    for r in range(S):
      wr = np.abs(wgt[..., r, None]) / (1 if weighted else cnt)
      dl = np.where(okc[..., r, :], np.abs(feat[..., r, :] - mean), 0.0)
      dd = tol_feat[..., r, :] + tol_mean + U * dl                       # |delta dl|: 2 |dl| |delta| and its square
      tol_var += (wr * rel_w[..., r, None] + abs_w[..., r, None]) * dl * dl + wr * (2 * dl * dd + MARGIN * dd * dd)
      absv += wr * dl * dl
    tol_var += (S + 3) * U * absv
    mm_ok = np.ones_like(okc) if 'minmax_over_invisible' in mut else okc
    mx = np.where(mm_ok, feat, -np.inf).max(-2)
    mn = np.where(mm_ok, feat, np.inf).min(-2)
  tol_mm = tol_feat.max(-2)
  parts, tols = [mean], [tol_mean]
  if use_variance:
    parts.append(var), tols.append(tol_var)
  if add_minmax:
    parts += [mx, mn]
    tols += [tol_mm, tol_mm]
  if weighted:
    parts.append(smax[..., None]), tols.append(tol_score.max(-1)[..., None])
  rows = np.where(anyv[..., None], np.concatenate(parts, -1), T(0))
  tol_rows = np.where(anyv[..., None], np.concatenate(tols, -1), 0.0)
  stride = (rows.shape[-1] + 3) // 4 * 4
  pad = lambda r: np.concatenate([r, np.zeros(r.shape[:2] + (stride - r.shape[-1],), r.dtype)], -1)
  valid = anyv
  if max_view_distance is not None and K > 0:
    lim = T(np.float32(max_view_distance))
    valid = valid & ((min_dist < lim) if 'min_dist_lt' in mut else (min_dist <= lim))
  # observations (lift_observations): features | log10 clip(depth, 0.1, 100) | unit viewing ray where visible
  vx, vy = g(pr['vx']), g(pr['vy'])
  nrm = np.maximum(np.sqrt((vx * vx + vy * vy) + depth * depth), T(np.float32(1e-5)))
  ld = np.log10(np.minimum(np.maximum(depth, T(np.float32(0.1))), T(np.float32(100.0))))
  ray = [np.where(ok, q / nrm, T(0)) for q in (vx, vy, depth)]
  obs = np.concatenate([feat, ld[..., None]] + [q[..., None] for q in ray], -1)
  tol_obs = np.concatenate([tol_feat, np.full(ld.shape + (1,), 4 * U * np.maximum(np.abs(ld[..., None]), 1.0))]
                           + [np.full(ld.shape + (1,), (r_proj + 6) * U)] * 3, -1)
  # what is free of exp / log / atan: bit-exact on a correct kernel when the geometry is exact
  sx = out['score_exact']
  first = np.take_along_axis(score, ok.argmax(-1)[..., None], -1)
  same = (np.where(ok, score, first) == first).all(-1) & (np.where(ok, score, 0) >= 0).all(-1)
  out.update(rows=pad(rows), tol_rows=MARGIN * pad(tol_rows), valid=valid, nok=nok, obs=obs, tol_obs=MARGIN * tol_obs,
             stats_exact=(nok <= 1) | (same & sx.all(-1)) | (not weighted), smax_exact=sx.all(-1),
             smax_channel=(rows.shape[-1] - 1) if weighted else None)
  return out


# ------------------------------- the border-flip rule -----------------------------------------
def border_rule(ref, K, max_view_distance=None):
  """From a float64 ``lift`` result alone: where may a decision of an f32 evaluation differ?

  Returns per-element booleans.  ``vis`` [B, N, V]: the visibility of the pair may flip -- x or y
  within PX_TOL pixels of 0 / w / h, depth within DEPTH_TOL of the near plane, and (fisheye) the
  radius within MARGIN ulps of the FoV limit or of eps, the distortion factor within MARGIN ulps of
  0.  ``order`` [B, N]: the selection may differ -- a visibility flip, or two visible views whose
  distances lie within MARGIN ulps across the K-th place.  ``valid`` [B, N]: a visibility flip or
  min_dist within MARGIN ulps of max_view_distance.  ``tap`` / ``bin`` [B, N, S]: the tap or bin
  pair may move by one -- the coordinate c within MARGIN ulps (of max(|c|, 1)) of an integer."""
  near = np.zeros(ref['vis'].shape, bool)
  x, y = ref['pj'], ref['pi']
  for q, lim in ((x, 0.0), (x, ref['wlim']), (y, 0.0), (y, ref['hlim'])):
    near |= np.abs(q - lim) <= PX_TOL
  near |= np.abs(ref['depth'] - float(EPS32)) <= DEPTH_TOL
  behind = ref['depth'] < float(EPS32) - DEPTH_TOL
  if 'radius' in ref:
    r = ref['radius']
    near |= np.abs(r - ref['fov_lim']) <= MARGIN * ulp32(r)
    near |= np.abs(r - float(EPS32)) <= MARGIN * ulp32(r)
    near |= np.abs(ref['fdist']) <= MARGIN * ulp32(1.0)
  near &= ~behind                                     # behind the camera nothing else is looked at
  anyflip = near.any(-1)
  d = np.where(ref['vis'] | near, ref['dist'], np.inf)
  order = anyflip.copy()
  if K > 0:
    with np.errstate(invalid='ignore'):
      ds = np.sort(d, -1)
      V = d.shape[-1]
      if K < V:
        a, b = ds[..., K - 1], ds[..., K]
        order |= np.isfinite(b) & (np.abs(b - a) <= MARGIN * ulp32(b))
      # an order flip inside the selected set changes slot order only: rows are sums, records are not
      gaps = np.diff(ds[..., :K + 1], axis=-1)
      order_inner = (np.isfinite(ds[..., 1:K + 1]) & (gaps <= MARGIN * ulp32(ds[..., 1:K + 1]))).any(-1)
  else:
    order_inner = np.zeros(anyflip.shape, bool)
  valid = anyflip.copy()
  if max_view_distance is not None and K > 0:
    md = ref['min_dist']
    lim = float(np.float32(max_view_distance))
    valid |= np.isfinite(md) & (np.abs(md - lim) <= MARGIN * ulp32(lim))
  frac = lambda c: np.abs(c - np.round(c))
  tp, bn = ref['taps'], ref['bins']
  tap = (frac(tp['ci']) <= MARGIN * ulp32(np.maximum(np.abs(tp['ci']), 1))) | \
        (frac(tp['cj']) <= MARGIN * ulp32(np.maximum(np.abs(tp['cj']), 1)))
  bins = frac(bn['c']) <= MARGIN * ulp32(np.maximum(np.abs(bn['c']), 1))
  return dict(vis=near, order=order, order_inner=order_inner, valid=valid, tap=tap & ref['ok'], bin=bins & ref['ok'])


def near_count(rule):
  """(voxel, view) decisions inside the border-flip distance: what the escape cap is measured against."""
  return int(rule['vis'].sum() + rule['order'].sum() + rule['valid'].sum())


# ------------------------------- planted scenes -----------------------------------------------
H, W, FD = 4, 8, 32
IDENT = np.eye(3)
ROTZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])     # an axis permutation with a sign


def _cam(f=(4.0, 2.0), c=(4.0, 2.0), k=(0.0, 0.0, 0.0), max_fov=np.pi * 0.9):
  return np.array([W, H, f[0], f[1], c[0], c[1], k[0], k[1], k[2], max_fov, np.tan(0.5 * max_fov)], np.float64)


def _exact32(a, what):
  a = np.asarray(a, np.float64)
  a32 = a.astype(np.float32)
  assert (a32.astype(np.float64) == a).all(), f'{what} is not exact in f32'
  return a32


def _scene(name, views, pts, *, K, nb, depth_min_max=(1.0, 8.0), max_view_distance=None, edges=None, exact=True):
  """views: per scene of the batch, a list of (R, t, cam row); pts [B, N, 3] (float64, f32-exact)."""
  cam = np.stack([np.stack([v[2] for v in vs]) for vs in views])
  Rt = np.stack([np.stack([np.concatenate([np.asarray(v[0], np.float64).reshape(9), np.asarray(v[1], np.float64)])
                           for v in vs]) for vs in views])
  cam32 = cam.astype(np.float32)            # (max_fov and its tangent are not dyadic: the pinhole path never reads them)
  return dict(name=name, cam=cam32, Rt=_exact32(Rt, name + ' Rt'), pts=_exact32(pts, name + ' points'), K=K, nb=nb,
              depth_min_max=depth_min_max, max_view_distance=max_view_distance, edges=edges or {}, fisheye=False,
              exact=exact, h=H, w=W, fd=FD)


def _at(x, y, z, R=IDENT, t=(0.0, 0.0, 0.0), f=(4.0, 2.0), c=(4.0, 2.0)):
  """The scene point that a pinhole view (R, t, f, c) sees at pixel (x, y), depth z."""
  pv = np.array([(x - c[0]) / f[0] * z, (y - c[1]) / f[1] * z, z], np.float64)
  return np.asarray(R, np.float64) @ pv + np.asarray(t, np.float64)


def _below(v):
  return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def _above(v):
  return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def scene_depth():
  e = float(EPS32)
  named = [('depth_eq_eps', e, True), ('depth_below_eps', _below(e), False), ('depth_zero', 0.0, False),
           ('depth_negative', -1.0, False), ('depth_minus_eps', -e, False), ('depth_above_eps', _above(e), True),
           ('depth_two', 2.0, True)]
  pts = np.array([[0.0, 0.0, d] for _, d, _ in named])[None]
  edges = {n: dict(voxel=(0, i), view=0, visible=v, depth=d) for i, (n, d, v) in enumerate(named)}
  return _scene('depth', [[(IDENT, (0, 0, 0), _cam())]], pts, K=0, nb=4, edges=edges)


def scene_pixels():
  """x and y borders in separate voxels of view 0 (identity, depth 2); view 1 is rotated by a signed axis
  permutation and stands back (depth 4): a transposed R or swapped w / h shows in either."""
  t1 = (0.0, 0.0, -2.0)
  views = [[(IDENT, (0, 0, 0), _cam()), (ROTZ, t1, _cam())]]
  d = 2.0 ** -20
  named = [('x_eq_0', 0.0, 2.5, True), ('x_below_0', -d, 2.5, False), ('x_eq_w', float(W), 2.5, False),
           ('x_below_w', _below(W), 2.5, True), ('y_eq_0', 4.5, 0.0, True), ('y_below_0', 4.5, -d, False),
           ('y_eq_h', 4.5, float(H), False), ('y_below_h', 4.5, _below(H), True),
           ('x_eq_h', float(H), 2.5, True), ('y_eq_w_over_2', 4.5, 3.5, True), ('corner_00', 0.0, 0.0, True),
           ('corner_wh', _below(W), _below(H), True)]
  pts, edges = [], {}
  for n, x, y, v in named:
    edges[n] = dict(voxel=(0, len(pts)), view=0, visible=v, x=x, y=y)
    pts.append(_at(x, y, 2.0))
  for n, x, y, v in named:                        # the same pixels of the rotated view
    edges[n + '_rot'] = dict(voxel=(0, len(pts)), view=1, visible=v, x=x, y=y)
    pts.append(_at(x, y, 4.0, ROTZ, t1))
  return _scene('pixels', views, np.array(pts)[None], K=0, nb=4, edges=edges)


def _tap_points():
  d = 2.0 ** -10
  ax = lambda n: sorted({0.25, n - 0.25, 2.0 ** -12, n - 2.0 ** -12}
                        | {k + 0.5 for k in range(n)} | {k + 0.5 - d for k in range(n)} | {k + 0.5 + d for k in range(n)}
                        | {k - d for k in range(1, n)} | {k + d for k in range(1, n)} | {float(k) for k in range(1, n)})
  ij = [(i, j) for i in ax(H) for j in (0.5, 3.25, W - 0.25)] + [(i, j) for j in ax(W) for i in (0.5, 1.75, H - 0.25)]
  return ij


def scene_taps(selective):
  """Pixel centres (wi1 == 0), the first and last half pixel (i0 == i1 after the clamp), both sides of every
  pixel seam and of every tap seam; K = 0 clips each tap index, K = 1 (a second view that sees nothing)
  clips the point."""
  ij = _tap_points()
  pts = np.array([_at(j, i, 2.0) for i, j in ij])[None]
  edges = {f'tap_{k}': dict(voxel=(0, k), view=0, pi=i, pj=j) for k, (i, j) in enumerate(ij)}
  views = [(IDENT, (0, 0, 0), _cam())]
  if selective:
    views.append((IDENT, (0.0, 0.0, 64.0), _cam()))       # in front of every point: never visible
  return _scene('taps_point_clip' if selective else 'taps_index_clip', [views], pts, K=1 if selective else 0, nb=4,
                edges=edges)


def scene_bins(nb, depth_min=1.0):
  """Depths on and beyond both clamp edges (logf(a) / logf(a) == 1: b0 == b1 == nb - 1, wb1 == 0), and the bin
  centres: with depth_max = depth_min 2^(nb-1) every centre is a power of two.  A bin centre is NOT exact in
  f32 (nor in f64: log(2^k) / log(2^(nb-1)) (nb - 1) may land one ulp under k): the pair (b0, b1) may move by
  one there, the blended score may not."""
  dmax = depth_min * 2.0 ** (nb - 1)
  named = [('depth_eq_min', depth_min, True), ('depth_below_min', depth_min / 2, True), ('depth_eq_max', dmax, True),
           ('depth_above_max', dmax * 2, True), ('depth_just_above_min', _above(depth_min), False),
           ('depth_just_below_max', _below(dmax), False)]
  named += [(f'bin_centre_{k}', depth_min * 2.0 ** k, False) for k in range(1, nb - 1)]
  named += [(f'bin_mid_{k}', depth_min * 2.0 ** k * 1.5, False) for k in range(0, nb - 1)]
  pts = np.array([[0.0, 0.0, d] for _, d, _ in named])[None]
  edges = {n: dict(voxel=(0, i), view=0, depth=d, exact=x) for i, (n, d, x) in enumerate(named)}
  return _scene(f'bins_nb{nb}_min{depth_min:g}', [[(IDENT, (0, 0, 0), _cam())]], pts, K=0, nb=nb,
                depth_min_max=(depth_min, dmax), edges=edges)


# camera centres whose offset from the origin is a 3-4-5 triangle: identity rotation, looking along +z
def _ring(s):
  return [(3.0 * s, 0.0, -4.0 * s), (-3.0 * s, 0.0, -4.0 * s), (0.0, 3.0 * s, -4.0 * s), (0.0, -3.0 * s, -4.0 * s)]


def _lattice(n):
  """n dyadic points on the plane z = 0 (every view depth is then a power of two), the origin first."""
  xs = np.arange(-12.0, 12.5, 0.5)
  ys = np.array([0.0, -1.0, 1.0, -0.5, 0.5])
  g = np.array([[x, y, 0.0] for y in ys for x in sorted(xs, key=abs)])
  extra = np.array([[0.0, 0.0, -96.0], [40.0, 0.0, 0.0]])
  g = np.concatenate([g[:1], extra, g[1:]])
  reps = -(-n // len(g))
  return np.concatenate([g] * reps)[:n]


def _pick(ref, cond, what):
  idx = np.argwhere(cond)
  assert len(idx), f'no voxel with: {what}'
  return tuple(int(i) for i in idx[0])


def scene_select(K, N=96):
  """Six views: 0 the nearest, looking away (invisible everywhere); 2, 3, 4 at bitwise-equal distance 5 from
  the origin; 1 at 10; 5 at 16."""
  ts = [(0.0, 0.0, 1.0), _ring(2)[0], _ring(1)[0], _ring(1)[1], _ring(1)[2], (0.0, 0.0, -16.0)]
  views = [[(IDENT, t, _cam()) for t in ts]]
  pts = _lattice(N)[None]
  sc = _scene(f'select_K{K}', views, pts, K=K, nb=4, edges={})
  ref = lift(np.zeros((1, 6, H, W, FD + 4), np.float32), sc['cam'], sc['Rt'], sc['pts'], K=K, fisheye=False, fd=FD, nb=4)
  nv = ref['vis'].sum(-1)
  sc['edges'] = {
      'tie_at_origin': dict(voxel=(0, 0), equal_views=(2, 3, 4), dist=5.0),
      'nearest_invisible': dict(voxel=(0, 0), view=0),
      'none_visible': dict(voxel=_pick(ref, nv == 0, 'no visible view')),
      'fewer_than_K': dict(voxel=_pick(ref, (nv > 0) & (nv < max(K, 2)), 'fewer than K visible') if K > 1 else None),
      'exactly_K': dict(voxel=_pick(ref, nv == K, 'exactly K visible')),
      'more_than_K': dict(voxel=_pick(ref, nv > K, 'more than K visible')),
  }
  return sc


def scene_tie_displaced():
  """Views 0 and 1 at bitwise-equal distance 5, view 2 nearer (4) and later in index order: K = 2 selects 2
  and 0.  (A sorted insertion that re-compares the entry it displaces with < hands the place to view 1.)"""
  ts = [_ring(1)[0], _ring(1)[1], (0.0, 0.0, -4.0), _ring(2)[2]]
  sc = _scene('tie_displaced', [[(IDENT, t, _cam()) for t in ts]], _lattice(21)[None], K=2, nb=4)
  sc['edges'] = {'tie_behind_a_nearer_later_view': dict(voxel=(0, 0), equal_views=(0, 1), selected=(2, 0))}
  return sc


def scene_select_max():
  """The largest V with the largest K the library accepts: three views at distance 5, four at 10, four at 20
  (the K-th place falls among these, the lowest index wins), the rest farther or blind, in a shuffled order."""
  V, K = library_limits()
  K = min(K, V - 1)
  ts = _ring(1)[:3] + _ring(2) + _ring(4) + _ring(8) + _ring(16)
  ts += [(0.0, 0.0, float(k)) for k in range(1, V - len(ts) + 1)]          # in front of the plane z = 0: blind
  order = np.random.default_rng(5).permutation(V)
  ts = [ts[i] for i in order]
  sc = _scene('select_max', [[(IDENT, t, _cam()) for t in ts]], _lattice(64)[None], K=K, nb=4)
  d20 = sorted(int(np.nonzero(order == i)[0][0]) for i in range(7, 11))
  sc['edges'] = {'tie_at_Kth_place': dict(voxel=(0, 0), equal_views=tuple(d20), dist=20.0, winner=d20[0])}
  return sc


def scene_maxdist(K, ulp_below):
  """min_dist == max_view_distance exactly is valid; a limit one ulp below min_dist (min_dist one ulp above the
  limit) is not; K = 0 ignores the limit."""
  ts = [_ring(1)[0], _ring(2)[1], (0.0, 0.0, -16.0)]
  lim = _below(5.0) if ulp_below else 5.0
  sc = _scene(f'maxdist_K{K}_{"ulp" if ulp_below else "eq"}', [[(IDENT, t, _cam()) for t in ts]], _lattice(40)[None],
              K=K, nb=4, max_view_distance=lim)
  sc['edges'] = {'min_dist_5': dict(voxel=(0, 0), min_dist=5.0, valid=(K == 0) or not ulp_below)}
  return sc


def scene_batch(N):
  """B = 2: other intrinsics and another view order in the second scene; N in {1, 31, 32, 33, 257}."""
  ts = [(0.0, 0.0, 1.0), _ring(2)[0], _ring(1)[0], _ring(1)[1], _ring(1)[2]]
  v0 = [(IDENT, t, _cam()) for t in ts]
  v1 = [(IDENT, t, _cam(f=(2.0, 1.0), c=(4.5, 1.5))) for t in (ts[3], ts[1], ts[4], ts[0], ts[2])]
  lat = _lattice(N)
  pts = np.stack([lat, lat[::-1]])
  return _scene(f'batch_N{N}', [v0, v1], pts, K=2, nb=4)


def planted_scenes():
  out = [scene_depth(), scene_pixels(), scene_taps(False), scene_taps(True), scene_bins(4), scene_bins(8),
         scene_bins(4, 2.0), scene_select(1), scene_select(2), scene_select(4), scene_tie_displaced(), scene_select_max(),
         scene_maxdist(1, False), scene_maxdist(1, True), scene_maxdist(2, True), scene_maxdist(0, True)]
  out += [scene_batch(N) for N in (1, 31, 32, 33, 257)]
  return out


def fisheye_version(sc, k_radial):
  """The same scene through the fisheye model: no longer exact, compared in float64 under the border rule."""
  o = dict(sc, name=f'{sc["name"]}_fisheye_k{k_radial:g}', fisheye=True, exact=False)
  cam = sc['cam'].copy()
  cam[..., 6] = k_radial
  cam[..., 7] = -k_radial / 4
  o['cam'] = cam
  return o


def random_scene(seed, B=2, V=5, N=257, K=2, k_radial=0.08, max_view_distance=None):
  """Random fisheye views around a cloud of points: nothing planted, everything float."""
  rng = np.random.default_rng(seed)
  cams, Rts = [], []
  for _ in range(B * V):
    q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
      q[:, 0] = -q[:, 0]
    a = rng.normal(size=3) * 0.25
    Rsmall = np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R, _r = np.linalg.qr(Rsmall)
    R = R * np.sign(np.diag(R))
    t = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(-6, -2)])
    cams.append(_cam(f=(rng.uniform(3, 5), rng.uniform(1.5, 2.5)), c=(rng.uniform(3.5, 4.5), rng.uniform(1.5, 2.5)),
                     k=(k_radial, -k_radial / 4, 0.0), max_fov=np.deg2rad(rng.uniform(100, 170))))
    Rts.append(np.concatenate([R.reshape(9), t]))
  pts = np.stack([rng.uniform(-5, 5, (B, N)), rng.uniform(-3, 3, (B, N)), rng.uniform(-3, 6, (B, N))], -1)
  return dict(name=f'random_{seed}', cam=np.array(cams, np.float32).reshape(B, V, 11),
              Rt=np.array(Rts, np.float32).reshape(B, V, 12), pts=pts.astype(np.float32), K=K, nb=8,
              depth_min_max=(1.0, 16.0), max_view_distance=max_view_distance, edges={}, fisheye=True, exact=False,
              h=H, w=W, fd=FD)


RANDOM_SEEDS = (11, 12)


def random_scenes():
  return [random_scene(RANDOM_SEEDS[0], K=2, max_view_distance=6.0), random_scene(RANDOM_SEEDS[1], V=3, K=0)]


# ------------------------------- readout inputs -----------------------------------------------
READOUTS = ('pixel', 'bins', 'equal', 'wide', 'offset')


def features(sc, kind, weighted=True, seed=0):
  """f_images [B, V, h, w, fd (+ nb)] f32.
  pixel:  channel c of view v is 2^v at pixel c and 0 elsewhere (fd == h w); scores 0 -- a one-view mean row IS
          the bilinear weight image, and the scale reads the view back.
  bins:   the same features; score channel b is the constant s_b = b - 2 -- score_max of a one-view voxel reads
          (1 - wb1) s_b0 + wb1 s_b1.
  equal:  unit noise features (dyadic, 8 bits), every score 0.5 -- bitwise-equal scores: weights 1 / n.
  wide:   unit noise features, scores in [-80, 80] -- rows of all-negative scores need the shift floor of 0.
  offset: 1000 + unit noise, unit noise scores -- the two-pass variance."""
  B, V = sc['cam'].shape[:2]
  nb = sc['nb'] if weighted else 0
  rng = np.random.default_rng(1000 + seed)
  f = np.zeros((B, V, H, W, FD + nb), np.float32)
  noise = lambda shape: (np.round(rng.uniform(-1, 1, shape) * 128) / 128).astype(np.float32)
  if kind in ('pixel', 'bins'):
    eye = np.eye(H * W, dtype=np.float32).reshape(H, W, FD)
    f[..., :FD] = eye[None, None] * (2.0 ** np.arange(V, dtype=np.float64)).astype(np.float32)[None, :, None, None, None]
    if kind == 'bins' and nb:
      f[..., FD:] = np.arange(nb, dtype=np.float32) - 2
  elif kind == 'equal':
    f[..., :FD] = noise(f[..., :FD].shape)
    f[..., FD:] = 0.5
  elif kind == 'wide':
    f[..., :FD] = noise(f[..., :FD].shape)
    f[..., FD:] = rng.uniform(-80, 80, f[..., FD:].shape).astype(np.float32)
    f[:, :, :, : W // 2, FD:] -= 80            # half of every image: all scores negative
    f[..., FD:] = np.clip(f[..., FD:], -80, 80)
  elif kind == 'offset':
    f[..., :FD] = 1000 + noise(f[..., :FD].shape)
    f[..., FD:] = noise(f[..., FD:].shape)
  else:
    raise ValueError(kind)
  return f


def plant_nonfinite(f, ref):
  """NaN / inf in every pixel that no selected, visible tap touches (a tap of weight 0 still touches: 0 * NaN
  is NaN) -- pixels of invisible views and of views beyond K included.  Returns (planted copy, count)."""
  B, V, h, w, C = f.shape
  touched = np.zeros((B, V, h, w), bool)
  tp = ref['taps']
  b = np.broadcast_to(np.arange(B)[:, None, None], ref['sel'].shape)
  ok = ref['ok']
  for i, j in (('i0', 'j0'), ('i0', 'j1'), ('i1', 'j0'), ('i1', 'j1')):
    touched[b[ok], ref['sel'][ok], tp[i][ok], tp[j][ok]] = True
  g = f.copy()
  free = np.argwhere(~touched)
  for n, (bb, v, i, j) in enumerate(free):
    g[bb, v, i, j] = (np.nan, np.inf, -np.inf)[n % 3]
  return g, len(free)


def tap_records(sc, res):
  """The tap records of csrc/lift_common.h (lift_rec_pack + the score) that a ``lift`` result implies for the
  voxels with one visible observation, and the row classes: recs [B, N, 8] int32, classes [B, N]."""
  B, V = sc['cam'].shape[:2]
  C = FD + sc['nb']
  one = res['nok'] == 1
  slot = res['ok'].argmax(-1)
  pick = lambda a: np.take_along_axis(a, slot[..., None], -1)[..., 0]
  tp, bn = res['taps'], res['bins']
  b = np.broadcast_to(np.arange(B)[:, None], one.shape)
  v = pick(res['sel'])
  i0, i1, j0, j1 = (pick(tp[k]) for k in ('i0', 'i1', 'j0', 'j1'))
  recs = np.zeros(one.shape + (8,), np.int32)
  recs[..., 0] = (((b * V + v) * H + i0) * W + j0) * C * 4
  recs[..., 1] = v | ((i1 != i0) << 8) | ((j1 != j0) << 9) | (pick(bn['b0']) << 10) | (pick(bn['b1']) << 18)
  recs[..., 2] = pick(tp['wi1']).astype(np.float32).view(np.int32)
  recs[..., 3] = pick(tp['wj1']).astype(np.float32).view(np.int32)
  recs[..., 4] = pick(res['score']).astype(np.float32).view(np.int32)
  recs[~one] = 0
  classes = np.where(res['valid'], np.where(res['nok'] > 1, 2, 1), 0).astype(np.uint8)
  return recs, classes


def reference(sc, f, dtype=np.float64, mut=(), **opts):
  return lift(f, sc['cam'], sc['Rt'], sc['pts'], K=sc['K'], fisheye=sc['fisheye'], fd=FD, nb=sc['nb'],
              depth_min_max=sc['depth_min_max'], max_view_distance=sc['max_view_distance'], dtype=dtype, mut=mut, **opts)
