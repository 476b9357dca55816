"""Restatement of the BEV plane family (``bev_ops.hip``, ``bev_conf_pool.hip``, the part of ``bev_bwd.hip`` below the
lift, ``bev_common.h``): float64 definitions, f32 models in the kernels' documented order, per-element bounds, the
dispatch rule, the case table and the mutants.  numpy only; nothing of ``snap_amd`` is imported.

Three layers, each a function of plain arrays (``vol [M, Z, D]`` f32, ``valid [M, Z]`` bool, planes ``[M, D]``):

* ``*_64``: the definitions, from ``oracle/bev.py`` and the reference's ``bev_mapper.py`` / ``layers.normalize``, with the
  closed-form VJPs.  ``tests/test_bev_plane_reference.py`` holds them to the oracle and to torch fp64 autograd.
* ``*_32``: the same arithmetic in ``np.float32`` in the order the comments of ``bev_common.h`` / ``bev_ops.hip``
  give.  The build uses ``-ffp-contract=off`` and no fast-math flag: every ``+ * / sqrt`` rounds once and correctly, so
  where no ``expf`` / ``log1pf`` is on the path the kernel's bits are these.  ``mutant=<name>`` is a wrong kernel.
* ``*_bound``: first-order f32 bounds of the ``*_64`` values, ``(n + 1) * 2^-24 * sum |terms|`` for ``n`` roundings on
  the path (the ``+ 1``: second-order remainder, and a single correctly rounded operation then sits at half its
  bound), errors of inputs propagated through quotients, and a stated term per ``expf`` / ``log1pf`` / reciprocal.
  The GPU tolerance is ``MARGIN`` times the bound.

Conventions restated from the kernels' comments (deliberate, pinned):
* forward max steps with a NaN-propagating max (as ``jnp.max``); every max VJP and the ``argz`` / ``ties`` record take
  the maximum by ``>`` over the valid entries, so a NaN never wins, holds no maximum and receives no gradient;
* ``eps`` is the f32 value the launcher receives; ``invalid = norm < eps`` is decided on the f32 norm.
"""
import functools
import zlib

import numpy as np

U = 2.0 ** -24          # f32 rounding unit
MARGIN = 8.0            # GPU tolerance = MARGIN x bound (the lift and pose-chain pins' multiplier)
ULP_EXP = 1.0           # allowance per expf / log1pf call in ulps (2U relative): the smallest power of two at which
                        # the f32 models stay <= 0.5 of the bound on every input (test_bev_plane_reference.py)
TINY = 2.0 ** -126      # absolute term per expf, and per product with a weight: a subnormal result may be flushed to zero
POOLINGS = ('max', 'sum', 'mean')
PERSISTENT_M = 8192     # bev_fuse_persistent: head and D == 128 and M >= 8192; the grid walks 1024 x 8 cells per trip
f32 = np.float32

MUTANTS = ('last_level_dropped', 'level63_masked', 'mean_by_Z', 'invalid_in_sum', 'argz_highest', 'ties_over_invalid',
           'full_grad_holders', 'no_bias', 'head_128_only', 'norm_le_eps', 'uncovered_bias', 'noncover_ties',
           'softmax_over_invalid', 'weight_on_invalid', 'persistent_first_trip_only')
UNREJECTABLE = ('softmax_no_floor',)


def g_(n):
  return (np.asarray(n, np.float64) + 1.0) * U


def f64(a):
  return np.asarray(a).astype(np.float64)


# ----------------------------------------------------------------------------------------------------
# dispatch, restated from the launchers' text
# ----------------------------------------------------------------------------------------------------
def pool_kernel(Z, D, pooling='max', want_arg=False):
  if want_arg and pooling == 'max' and Z <= 64 and D <= 128:
    return 'vertical_pool_max_arg_kernel'
  return 'vertical_pool_wave_kernel' if Z <= 64 else 'vertical_pool_kernel'


def pool_bwd_kernel(arg):
  return 'vertical_pool_max_bwd_arg_kernel' if arg else 'vertical_pool_bwd_kernel'


def fuse_kernel(M, D, head, bwd=False):
  persistent = head and D == 128 and M >= PERSISTENT_M
  return 'plane_fuse_match_' + ('bwd_' if bwd else '') + ('d128_' if persistent else '') + 'kernel'


def pool_refused(Z, D):
  return D <= 0 or D % 4 != 0 or D > 256 or Z <= 0


def fuse_refused(num_planes, D, Dm=None):
  return num_planes < 1 or num_planes > 4 or D % 4 != 0 or D > 256 or (Dm is not None and not 1 <= Dm <= 32)


def conf_pool_refused(Z, D):
  return Z <= 0 or Z > 64 or D % 4 != 0 or D > 128


KERNELS = ('vertical_pool_kernel', 'vertical_pool_wave_kernel', 'vertical_pool_max_arg_kernel', 'plane_fuse_match_kernel',
           'plane_fuse_match_d128_kernel', 'confidence_head_kernel', 'conf_pool_kernel', 'conf_pool_bwd_kernel',
           'vertical_pool_bwd_kernel', 'vertical_pool_max_bwd_arg_kernel', 'plane_fuse_match_bwd_kernel',
           'plane_fuse_match_bwd_d128_kernel', 'confidence_head_bwd_kernel')


# ----------------------------------------------------------------------------------------------------
# float64 definitions
# ----------------------------------------------------------------------------------------------------
def log_sigmoid64(x):
  return np.minimum(x, 0) - np.log1p(np.exp(-np.abs(x)))


def sigmoid64(x):
  with np.errstate(over='ignore'):
    return 1.0 / (1.0 + np.exp(-x))


def reduce_64(x, valid, pooling):
  """Masked max / sum / mean over axis -2 of x [..., N, D] with valid [..., N]: (out [..., D], any [...])."""
  x = f64(x)
  w = valid[..., None]
  n = valid.sum(-1)
  with np.errstate(invalid='ignore', divide='ignore'):
    if pooling == 'max':
      out = np.where(w, x, -np.inf).max(-2)
    else:
      out = np.where(w, x, 0).sum(-2)
      if pooling == 'mean':
        out = out / n[..., None]
  return np.where(n[..., None] > 0, out, 0.0), n > 0


def holders_64(x, valid):
  """The maximum by `>` over the valid entries (a NaN never wins), who holds it, and how many do."""
  x = f64(x)
  with np.errstate(invalid='ignore'):
    best = np.fmax.reduce(np.where(valid[..., None], x, -np.inf), axis=-2)
    best = np.where(np.isnan(best), -np.inf, best)
    hold = valid[..., None] & (x == best[..., None, :])
  return best, hold, hold.sum(-2)


def reduce_vjp_64(x, valid, g, pooling, mutant=None):
  """d out -> d x.  max: shared equally among the valid holders of the maximum."""
  g = f64(g)[..., None, :]
  w = valid[..., None]
  if pooling == 'sum':
    return np.where(w, g, 0.0) + np.zeros(np.shape(x))
  if pooling == 'mean':
    with np.errstate(invalid='ignore', divide='ignore'):
      return np.where(w, g / valid.sum(-1)[..., None, None], 0.0)
  _, hold, cnt = holders_64(x, valid)
  if mutant == 'noncover_ties':
    best = holders_64(x, valid)[0]
    cnt = (f64(x) == best[..., None, :]).sum(-2)
  with np.errstate(invalid='ignore', divide='ignore'):
    share = g if mutant == 'full_grad_holders' else g / cnt[..., None, :]
    return np.where(hold, share, 0.0)


def record_64(vol, valid, mutant=None):
  """argz / ties of vertical_pool_max_arg_kernel: lowest valid holder, number of valid holders; (255, 0) where no
  valid level holds a maximum (no valid level, or NaN only)."""
  best, hold, cnt = holders_64(vol, valid)
  Z = vol.shape[-2]
  lev = np.arange(Z)[:, None]
  if mutant == 'argz_highest':
    argz = np.where(hold, lev, -1).max(-2)
  else:
    argz = np.where(hold, lev, 255).min(-2)
  if mutant == 'ties_over_invalid':
    with np.errstate(invalid='ignore'):
      cnt = np.where(cnt > 0, (f64(vol) == best[..., None, :]).sum(-2), 0)
  argz = np.where(cnt > 0, argz, 255)
  return argz.astype(np.uint8), np.minimum(cnt, 255).astype(np.uint8)


def head_64(x, Wm, bm, normalize, eps, covered):
  """matching = where(covered, normalize(bm + x @ Wm), 0); also y and the norm."""
  y = f64(bm) + f64(x) @ f64(Wm)
  nrm = np.sqrt((y * y).sum(-1, keepdims=True))
  z = y
  if normalize:
    invalid = nrm < float(f32(eps))
    with np.errstate(invalid='ignore', divide='ignore'):
      z = np.where(invalid, 0.0, y / nrm)
  return np.where(covered[..., None], z, 0.0), y, nrm[..., 0]


def fuse_vjp_64(planes, valids, pooling, Wm, bm, normalize, eps, dmatching, dfused, mutant=None):
  """(d planes [P, M, D], dy [M, Dm] or None).  The fused vector is recomputed with the NaN-skipping maximum."""
  x = np.stack([f64(p) for p in planes], -2)
  v = stack_valids(valids, x.shape[0])
  any_ = v.any(-1)
  if pooling == 'max':
    fused = np.where(any_[:, None], holders_64(x, v)[0], 0.0)
  else:
    fused = reduce_64(x, v, pooling)[0]
  df = np.zeros_like(fused)
  dy = None
  if dmatching is not None:
    y = f64(bm) + fused @ f64(Wm)
    dz = np.where(any_[:, None], f64(dmatching), 0.0)
    dy = dz
    if normalize:
      nrm = np.sqrt((y * y).sum(-1, keepdims=True))
      with np.errstate(invalid='ignore', divide='ignore'):
        z = y / nrm
        dy = np.where(nrm >= float(f32(eps)), (dz - z * (z * dz).sum(-1, keepdims=True)) / nrm, 0.0)
    df = dy @ f64(Wm).T
  if dfused is not None:
    df = df + np.where(any_[:, None], f64(dfused), 0.0)
  dx = reduce_vjp_64(x, v, df, pooling, mutant=mutant)
  return np.moveaxis(dx, -2, 0), dy


def conf_head_64(f, valid, w, b):
  s = f64(f) @ f64(w) + float(f64(b).reshape(-1)[0])
  out = log_sigmoid64(s)
  return (out if valid is None else np.where(valid, out, 0.0)), s


def conf_head_vjp_64(f, valid, w, b, g):
  s = conf_head_64(f, None, w, b)[1]
  ds = f64(g) * sigmoid64(-s)
  if valid is not None:
    ds = np.where(valid, ds, 0.0)
  return ds[:, None] * f64(w), (ds[:, None] * f64(f)).sum(0), ds.sum(keepdims=True), ds


def conf_pool_64(vol, valid, w, b, log_sig):
  """plane, any, scores, weights: softmax over the valid levels (all when none is valid) with shift
  max(0, max selected score); zero weight on invalid levels; zero plane for a column without a valid level."""
  x = f64(vol)
  raw = x @ f64(w) + float(f64(b).reshape(-1)[0])
  s = log_sigmoid64(raw) if log_sig else raw
  any_ = valid.any(-1)
  use = np.where(any_[:, None], valid, True)
  shift = np.maximum(np.where(use, s, -np.inf).max(-1, keepdims=True), 0)
  e = np.where(use, np.exp(s - shift), 0.0)
  p = np.where(valid, e / e.sum(-1, keepdims=True), 0.0)
  plane = (x * p[..., None]).sum(-2)
  return np.where(any_[:, None], plane, 0.0), any_, s, p, raw


def conf_pool_vjp_64(vol, w, b, weights, g, log_sig):
  """VJP of conf_pool_64's plane at the weights p it was given: ds_z = p_z (g.f_z - sum_k p_k g.f_k) [sigmoid(-raw_z)],
  d f_z = p_z g + ds_z w, d w = sum ds f, d b = sum ds."""
  x, p, g, w = f64(vol), f64(weights), f64(g), f64(w)
  dp = (x * g[:, None, :]).sum(-1)
  ds = p * (dp - (p * dp).sum(-1, keepdims=True))
  if log_sig:
    ds = ds * sigmoid64(-(x @ w + float(f64(b).reshape(-1)[0])))
  dvol = p[..., None] * g[:, None, :] + ds[..., None] * w
  return dvol, (ds[..., None] * x).sum((0, 1)), ds.sum(keepdims=True).reshape(1), ds


def stack_valids(valids, M):
  return np.stack([np.ones(M, bool) if v is None else np.asarray(v, bool) for v in valids], -1)


# ----------------------------------------------------------------------------------------------------
# f32 models in the kernels' order
# ----------------------------------------------------------------------------------------------------
def half_sum32(v):
  """The xor butterfly 16, 8, 4, 2, 1 over the 32 lanes of axis -1 (zeros beyond the given width): lane 0's bits."""
  v = np.asarray(v, f32)
  pad = np.zeros(v.shape[:-1] + (32,), f32)
  pad[..., :v.shape[-1]] = v
  lanes = np.arange(32)
  for o in (16, 8, 4, 2, 1):
    pad = pad + pad[..., lanes ^ o]
  return pad[..., 0]


def dot32(x, w):
  """A row's dot product as the confidence kernels form it: lane q takes bev_dot4 of the quads q, q + 32, ... (the
  128-channel stride), left to right, added in sequence from +0, then the butterfly."""
  x, w = np.asarray(x, f32), np.asarray(w, f32)
  D = x.shape[-1]
  acc = np.zeros(x.shape[:-1] + (32,), f32)
  for c0 in range(0, D, 128):
    xs, ws = x[..., c0:c0 + 128], w[c0:c0 + 128]
    nq = xs.shape[-1] // 4
    xs = xs.reshape(xs.shape[:-1] + (nq, 4))
    ws = ws.reshape(nq, 4)
    d4 = ((xs[..., 0] * ws[:, 0] + xs[..., 1] * ws[:, 1]) + xs[..., 2] * ws[:, 2]) + xs[..., 3] * ws[:, 3]
    acc[..., :nq] = acc[..., :nq] + d4
  return half_sum32(acc)


def log_sigmoid32(x):
  x = np.asarray(x, f32)
  return np.minimum(x, f32(0)) - np.log1p(np.exp(-np.abs(x)))


def _seq(rows, pooling):
  """Plain ascending sequence from the reduce's neutral element (rows: list of [D] f32)."""
  if pooling == 'max':
    acc = np.full(rows[0].shape, -np.inf, f32) if rows else None
    for r in rows:
      acc = np.maximum(acc, r)          # NaN-propagating, as snap_max_nan
    return acc
  acc = np.zeros(rows[0].shape, f32) if rows else None
  for r in rows:
    acc = acc + r
  return acc


def pool_32(vol, valid, pooling, mutant=None):
  """plane [M, D] f32, pvalid [M].  Z <= 64: valid levels by rank, ranks 4t, 4t+2 -> half 0 and 4t+1, 4t+3 -> half 1
  (the even and the odd ranks, each in sequence from +0; a missing slot adds +0), result half 0 + half 1.
  Z > 64: plain ascending sequence."""
  vol = np.asarray(vol, f32)
  M, Z, D = vol.shape
  out = np.zeros((M, D), f32)
  pv = np.zeros(M, bool)
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    for m in range(M):
      vm = valid[m].copy()
      if mutant == 'level63_masked' and Z > 63:
        vm[63] = False
      lev = list(np.nonzero(vm)[0])
      count = len(lev)
      if mutant == 'last_level_dropped' and lev:
        lev = lev[:-1]
      if mutant == 'invalid_in_sum' and pooling != 'max' and count and not valid[m].all():
        lev = sorted(lev + [int(np.nonzero(~valid[m])[0][0])])
      pv[m] = count > 0
      if not count:
        continue
      if not lev:
        acc = np.full(D, -np.inf if pooling == 'max' else 0, f32)
      elif Z <= 64:
        h0, h1 = [vol[m, z] for z in lev[0::2]], [vol[m, z] for z in lev[1::2]]
        acc = _seq(h0, pooling)
        if h1:
          acc = np.maximum(acc, _seq(h1, pooling)) if pooling == 'max' else acc + _seq(h1, pooling)
      else:
        acc = _seq([vol[m, z] for z in lev], pooling)
      if pooling == 'mean':
        acc = acc / f32(Z if mutant == 'mean_by_Z' else count)
      out[m] = acc
  return out, pv


def share_32(x, valid, g, pooling, mutant=None):
  """The VJP of a masked reduce over axis -2 in f32: g, g / (float)count, or g / cnt to the holders."""
  x, g = np.asarray(x, f32), np.asarray(g, f32)[..., None, :]
  w = valid[..., None]
  zero = np.zeros(x.shape, f32)
  with np.errstate(invalid='ignore', divide='ignore'):
    if pooling == 'sum':
      return np.where(w, g, zero)
    if pooling == 'mean':
      return np.where(w, g / valid.sum(-1).astype(f32)[..., None, None], zero)
    best, hold, cnt = holders_64(x, valid)
    if mutant == 'noncover_ties':
      cnt = (f64(x) == best[..., None, :]).sum(-2)
    share = g + zero if mutant == 'full_grad_holders' else g / cnt.astype(f32)[..., None, :]
    return np.where(hold, share, zero).astype(f32)


def head_32(x, Wm, bm, mutant=None):
  """y_j = bm_j, then y_j += x_c * Wm[c, j] for ascending c (shuffle form and register-column form alike)."""
  x, Wm = np.asarray(x, f32), np.asarray(Wm, f32)
  y = np.broadcast_to(np.asarray(bm, f32), (x.shape[0], Wm.shape[1])).copy()
  if mutant == 'no_bias':
    y[:] = 0
  D = min(x.shape[1], 128) if mutant == 'head_128_only' else x.shape[1]
  with np.errstate(invalid='ignore', over='ignore'):
    for c in range(D):
      y = y + x[:, c, None] * Wm[c]
  return y


def normalize_32(y, eps, mutant=None):
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    nrm = np.sqrt(half_sum32(y * y))[:, None]
    invalid = nrm <= f32(eps) if mutant == 'norm_le_eps' else nrm < f32(eps)
    return np.where(invalid, f32(0), y / nrm), nrm


def fuse_32(planes, valids, pooling, Wm=None, bm=None, normalize=True, eps=1e-5, mutant=None):
  """fused [M, D], fvalid [M], matching [M, Dm] or None: planes in ascending order over the covering ones."""
  M, D = planes[0].shape
  v = stack_valids(valids, M)
  count = v.sum(-1)
  any_ = count > 0
  x = [np.asarray(p, f32) for p in planes]
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    if pooling == 'max':
      acc = np.full((M, D), -np.inf, f32)
      for p in range(len(x)):
        acc = np.where(v[:, p, None], np.maximum(acc, x[p]), acc)
    else:
      acc = np.zeros((M, D), f32)
      for p in range(len(x)):
        acc = np.where(v[:, p, None], acc + x[p], acc)
      if pooling == 'mean':
        acc = acc / np.maximum(count, 1).astype(f32)[:, None]
    fused = np.where(any_[:, None], acc, f32(0))
    matching = None
    if Wm is not None:
      y = head_32(fused, Wm, bm, mutant)
      if normalize:
        y = normalize_32(y, eps, mutant)[0]
      matching = y if mutant == 'uncovered_bias' else np.where(any_[:, None], y, f32(0))
      if mutant == 'persistent_first_trip_only' and D == 128 and M >= PERSISTENT_M:
        matching = matching.copy()
        matching[PERSISTENT_M:] = 0
  return fused, any_, matching


def fuse_vjp_32(planes, valids, pooling, Wm, bm, normalize, eps, dmatching, dfused, mutant=None):
  """(d planes [P, M, D] f32, dy [M, Dm] f32 or None) in the order of plane_fuse_match_bwd_kernel."""
  M, D = planes[0].shape
  v = stack_valids(valids, M)
  count = v.sum(-1)
  any_ = count > 0
  x = np.stack([np.asarray(p, f32) for p in planes], -2)
  with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
    if pooling == 'max':
      fused = np.where(any_[:, None], holders_64(x, v)[0], 0.0).astype(f32)
    else:
      fused = fuse_32(planes, valids, pooling)[0]
    df = np.zeros((M, D), f32)
    dy = None
    if dmatching is not None:
      Wm = np.asarray(Wm, f32)
      y = head_32(fused, Wm, bm)
      dz = np.where(any_[:, None], np.asarray(dmatching, f32), f32(0))
      dy = dz
      if normalize:
        nrm = np.sqrt(half_sum32(y * y))[:, None]
        z = y / nrm
        zdz = half_sum32(z * dz)[:, None]
        dy = np.where(nrm >= f32(eps), (dz - z * zdz) / nrm, f32(0)).astype(f32)
      for j in range(Wm.shape[1]):
        df = df + Wm[None, :, j] * dy[:, j, None]
    if dfused is not None:
      df = np.where(any_[:, None], df + np.asarray(dfused, f32), df)
    dx = share_32(x, v, df, pooling, mutant=mutant)
    if mutant == 'persistent_first_trip_only' and D == 128 and M >= PERSISTENT_M and dmatching is not None:
      dx[PERSISTENT_M:] = 0
  return np.moveaxis(dx, -2, 0), dy


def conf_head_32(f, valid, w, b):
  s = dot32(f, w) + np.asarray(b, f32).reshape(-1)[0]
  out = log_sigmoid32(s)
  return (out if valid is None else np.where(valid, out, f32(0))), s


def conf_head_vjp_32(f, valid, w, b, g):
  """(d f, prod = ds f [M, D], ds [M]): the column sums of prod / ds leave through another kernel family."""
  s = conf_head_32(f, None, w, b)[1]
  with np.errstate(over='ignore'):
    ds = np.asarray(g, f32) / (f32(1) + np.exp(s))
  if valid is not None:
    ds = np.where(valid, ds, f32(0))
  return ds[:, None] * np.asarray(w, f32), ds[:, None] * np.asarray(f, f32), ds


def conf_pool_32(vol, valid, w, b, log_sig, mutant=None):
  """conf_pool_kernel's online softmax: the levels in ascending order, the running shift starting at 0."""
  vol = np.asarray(vol, f32)
  M, Z, D = vol.shape
  s = dot32(vol, w) + np.asarray(b, f32).reshape(-1)[0]
  if log_sig:
    s = log_sigmoid32(s)
  any_ = valid.any(-1)
  use = np.where(any_[:, None], valid, True)
  if mutant == 'softmax_over_invalid':
    use = np.ones_like(use)
  run_max = np.zeros(M, f32)
  if mutant == 'softmax_no_floor':
    run_max = np.where(use, s, -np.inf).max(-1).astype(f32)
  run_sum = np.zeros(M, f32)
  acc = np.zeros((M, D), f32)
  with np.errstate(invalid='ignore', over='ignore', divide='ignore', under='ignore'):
    for z in range(Z):
      u = use[:, z]
      nm = np.where(u, np.maximum(run_max, s[:, z]), run_max)
      scale = np.where(u, np.exp(run_max - nm), f32(1))
      e = np.where(u, np.exp(s[:, z] - nm), f32(0))
      run_sum = np.where(u, run_sum * scale + e, run_sum)
      ev = np.where(valid[:, z] & u, e, f32(0))
      acc = np.where(u[:, None], acc * scale[:, None] + ev[:, None] * vol[:, z], acc)
      run_max = nm
    plane = np.where(any_[:, None], acc / run_sum[:, None], f32(0))
    wz = np.exp(s - run_max[:, None]) / run_sum[:, None]
    keep = valid if mutant != 'weight_on_invalid' else np.where(any_[:, None], True, valid)
    weights = np.where(keep, wz, f32(0))
  return plane.astype(f32), any_, s, weights.astype(f32)


def conf_pool_vjp_32(vol, w, b, weights, g, log_sig):
  """(dvol, ds [M, Z]) in conf_pool_bwd_kernel's order; levels of weight 0 are skipped."""
  vol, p, g, w = np.asarray(vol, f32), np.asarray(weights, f32), np.asarray(g, f32), np.asarray(w, f32)
  M, Z, D = vol.shape
  # g . f_z with bev_dot4(g, f): the products g_k f_k, associated as dot32 does
  dp = _dot_rows32(g[:, None, :], vol)
  pdp = np.zeros(M, f32)
  for z in range(Z):
    pdp = np.where(p[:, z] != 0, pdp + p[:, z] * dp[:, z], pdp)
  ds = p * (dp - pdp[:, None])
  if log_sig:
    s = dot32(vol, w) + np.asarray(b, f32).reshape(-1)[0]
    with np.errstate(over='ignore'):
      ds = ds * (f32(1) / (f32(1) + np.exp(s)))
  on = (p != 0)
  ds = np.where(on, ds, f32(0))
  dvol = np.where(on[..., None], p[..., None] * g[:, None, :] + ds[..., None] * w, f32(0))
  return dvol.astype(f32), ds.astype(f32)


def _dot_rows32(a, b):
  a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
  nq = a.shape[-1] // 4
  a = a.reshape(a.shape[:-1] + (nq, 4))
  b = b.reshape(b.shape[:-1] + (nq, 4))
  return half_sum32(((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3])


# ----------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------
def reduce_bound(x, valid, pooling):
  n = valid.sum(-1)[..., None]
  if pooling == 'max':
    return np.zeros(x.shape[:-2] + x.shape[-1:])
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    a = np.where(valid[..., None], np.abs(f64(x)), 0).sum(-2)
    b = g_(n) * a if pooling == 'sum' else g_(n + 1) * a / n
  return np.where(n > 0, b, 0.0)


def reduce_vjp_bound(x, valid, g, pooling, e_g=0.0):
  """Bound of reduce_vjp_64 for a gradient known to e_g."""
  g, e_g = np.abs(f64(g))[..., None, :], np.broadcast_to(e_g, np.shape(g))[..., None, :]
  w = valid[..., None]
  with np.errstate(invalid='ignore', divide='ignore'):
    if pooling == 'sum':
      return np.where(w, e_g, 0.0) + np.zeros(x.shape)
    n = valid.sum(-1)[..., None, None] if pooling == 'mean' else holders_64(x, valid)[2][..., None, :]
    hold = w if pooling == 'mean' else holders_64(x, valid)[1]
    return np.where(hold, (e_g + g_(1) * g) / n, 0.0)


def matching_bound(fused, e_fused, Wm, bm, normalize, eps, covered):
  """Bounds of head_64 on a fused vector known to e_fused: e_y, and e_z of the matching output; y, nrm, z with them."""
  W = np.abs(f64(Wm))
  D = fused.shape[-1]
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    e_y = g_(D + 1) * (np.abs(f64(bm)) + np.abs(fused) @ W) + e_fused @ W
    _, y, nrm = head_64(fused, Wm, bm, False, eps, covered)
    nrm = nrm[:, None]
    out = dict(e_y=e_y, y=y, nrm=nrm)
    if not normalize:
      out['e_z'] = np.where(covered[:, None], e_y, 0.0)
      return out
    e_ss = g_(6) * nrm ** 2 + 2 * (np.abs(y) * e_y).sum(-1, keepdims=True)
    e_n = e_ss / (2 * nrm) + U * nrm
    z = y / nrm
    e_z = e_y / nrm + np.abs(z) * e_n / nrm + g_(1) * np.abs(z)
    ok = covered[:, None] & (nrm >= float(f32(eps)))
    out.update(e_n=e_n, z=z, e_z=np.where(ok, e_z, 0.0))
  return out


def fuse_vjp_bound(planes, valids, pooling, Wm, bm, normalize, eps, dmatching, dfused):
  """(bound of d planes [P, M, D], bound of dy)."""
  x = np.stack([f64(p) for p in planes], -2)
  M, _, D = x.shape
  v = stack_valids(valids, M)
  any_ = v.any(-1)
  with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
    fused = np.where(any_[:, None], holders_64(x, v)[0], 0.0) if pooling == 'max' else reduce_64(x, v, pooling)[0]
    e_df = np.zeros((M, D))
    e_dy = None
    df = np.zeros((M, D))
    if dmatching is not None:
      W = np.abs(f64(Wm))
      Dm = W.shape[1]
      hb = matching_bound(fused, reduce_bound(x, v, pooling), Wm, bm, normalize, eps, any_)
      dz = np.where(any_[:, None], f64(dmatching), 0.0)
      dy, e_dy = dz, np.zeros_like(dz)
      if normalize:
        nrm, z, e_z, e_n = hb['nrm'], hb['z'], hb['e_z'], hb['e_n']
        zdz = (z * dz).sum(-1, keepdims=True)
        e_zdz = (np.abs(dz) * e_z).sum(-1, keepdims=True) + g_(6) * np.abs(z * dz).sum(-1, keepdims=True)
        t = z * zdz
        e_t = np.abs(zdz) * e_z + np.abs(z) * e_zdz + U * np.abs(t)
        num = dz - t
        e_num = e_t + U * (np.abs(dz) + np.abs(t))
        dy = num / nrm
        e_dy = e_num / nrm + np.abs(dy) * e_n / nrm + g_(1) * np.abs(dy)
        ok = nrm >= float(f32(eps))
        dy, e_dy = np.where(ok, dy, 0.0), np.where(ok, e_dy, 0.0)
      df = dy @ f64(Wm).T
      e_df = e_dy @ W.T + g_(Dm + 1) * (np.abs(dy) @ W.T)
    if dfused is not None:
      gd = np.where(any_[:, None], f64(dfused), 0.0)
      e_df = e_df + g_(1) * (np.abs(df) + np.abs(gd))
      df = df + gd
    e_dx = reduce_vjp_bound(x, v, df, pooling, e_df)
  return np.moveaxis(e_dx, -2, 0), e_dy


def score_bound(f, w, b):
  D = f.shape[-1]
  n = 4 + -(-D // 128) + 5 + 1
  return g_(n) * (np.abs(f64(f)) @ np.abs(f64(w)) + abs(float(f64(b).reshape(-1)[0])))


def log_sigmoid_bound(s, e_s):
  t = np.exp(-np.abs(s))
  L = np.log1p(t)
  return sigmoid64(-s) * e_s + ULP_EXP * 2 * U * (t / (1 + t) + L) + g_(1) * np.abs(np.minimum(s, 0) - L) + TINY


def recip_bound(s, e_s):
  """Relative bound of 1 / (1 + expf(s)): the exponential's argument and allowance, the sum, the reciprocal."""
  return sigmoid64(s) * (e_s + ULP_EXP * 2 * U) + 3 * U


def conf_head_bound(f, valid, w, b):
  s = conf_head_64(f, None, w, b)[1]
  e = log_sigmoid_bound(s, score_bound(f, w, b))
  return e if valid is None else np.where(valid, e, 0.0)


def conf_head_vjp_bound(f, valid, w, b, g):
  """Bounds of (d f, d w, d b); the column sums over M rows are charged M roundings."""
  s = conf_head_64(f, None, w, b)[1]
  ds = conf_head_vjp_64(f, valid, w, b, g)[3]
  M = f.shape[0]
  e_ds = np.abs(ds) * (recip_bound(s, score_bound(f, w, b)) + U) + TINY * np.abs(f64(g))
  if valid is not None:
    e_ds = np.where(valid, e_ds, 0.0)
  W, F = np.abs(f64(w)), np.abs(f64(f))
  e_df = e_ds[:, None] * W + g_(1) * np.abs(ds)[:, None] * W
  e_dw = (e_ds[:, None] * F).sum(0) + g_(M + 1) * (np.abs(ds)[:, None] * F).sum(0)
  e_db = e_ds.sum(keepdims=True) + g_(M) * np.abs(ds).sum(keepdims=True)
  return e_df, e_dw, e_db


def conf_pool_bound(vol, valid, w, b, log_sig):
  """Bounds of conf_pool_64's (plane, scores, weights)."""
  plane, any_, s, p, raw = conf_pool_64(vol, valid, w, b, log_sig)
  Z = vol.shape[1]
  e_s = score_bound(vol, w, b)
  if log_sig:
    e_s = log_sigmoid_bound(raw, e_s)
  use = np.where(any_[:, None], valid, True)
  m = np.maximum(np.where(use, s, -np.inf).max(-1), 0)
  span = np.where(use, np.abs(s - m[:, None]), 0).max(-1) + m
  rho = 2 * np.where(use, e_s, 0).max(-1) + 2 * U * span + (Z + 2) * ULP_EXP * 2 * U + 3 * (Z + 1) * U
  e_w = np.where(valid, p * (2 * rho[:, None] + 2 * U), 0.0) + np.where(valid & any_[:, None], TINY, 0.0)
  e_plane = (2 * rho + g_(Z + 2))[:, None] * (p[..., None] * np.abs(f64(vol))).sum(-2) + TINY
  return np.where(any_[:, None], e_plane, 0.0), e_s, e_w


def conf_pool_vjp_bound(vol, w, b, weights, g, log_sig):
  """Bounds of conf_pool_vjp_64's (dvol, d w, d b); rows = ceil(M / 8) partial rows leave through the column sums."""
  x, p, gg, ww = f64(vol), f64(weights), f64(g), f64(w)
  M, Z, D = x.shape
  ax, ag, aw = np.abs(x), np.abs(gg), np.abs(ww)
  dp = (x * gg[:, None, :]).sum(-1)
  e_dp = g_(9) * (ax * ag[:, None, :]).sum(-1)
  pdp = (p * dp).sum(-1, keepdims=True)
  e_pdp = (p * e_dp).sum(-1, keepdims=True) + g_(Z + 1) * np.abs(p * dp).sum(-1, keepdims=True)
  e_ds = p * (e_dp + e_pdp + U * (np.abs(dp) + np.abs(pdp))) + U * np.abs(p * (dp - pdp))
  ds = p * (dp - pdp)
  if log_sig:
    raw = x @ ww + float(f64(b).reshape(-1)[0])
    q = sigmoid64(-raw)
    e_ds = q * e_ds + np.abs(ds * q) * (recip_bound(raw, score_bound(vol, w, b)) + U) + TINY * np.abs(ds)
    ds = ds * q
  e_dvol = aw * e_ds[..., None] + g_(3) * (p[..., None] * ag[:, None, :] + np.abs(ds)[..., None] * aw) + TINY
  n = Z + 8 + -(-M // 8) + 1
  e_dw = (e_ds[..., None] * ax).sum((0, 1)) + g_(n) * (np.abs(ds)[..., None] * ax).sum((0, 1)) + TINY
  e_db = (e_ds.sum() + g_(n) * np.abs(ds).sum()).reshape(1) + TINY
  return e_dvol, e_dw, e_db


# ----------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------
NONFINITE = np.array([np.nan, np.inf, -np.inf, 1e30], f32)
BITMASK_Z = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 70, 255)


def bitmask_patterns(Z):
  """name -> valid [Z]: exactly k valid levels (k = 0 .. 5, spread over the column), only level 0, only level Z - 1,
  only the odd levels, only levels >= 32, all."""
  pats = {}
  for k in range(6):
    v = np.zeros(Z, bool)
    if k and k <= Z:
      v[np.unique(np.linspace(0, Z - 1, k).round().astype(int))] = True
      if v.sum() != k:
        continue
    elif k:
      continue
    pats[f'k{k}'] = v
  for name, idx in (('first', slice(0, 1)), ('last', slice(Z - 1, Z)), ('odd', slice(1, Z, 2)), ('ge32', slice(32, Z)),
                    ('all', slice(0, Z))):
    v = np.zeros(Z, bool)
    v[idx] = True
    pats[name] = v
  return pats


@functools.lru_cache(maxsize=None)
def bitmask_case(Z):
  """Channel group g (four channels) carries 2^(z - 16 g) at level z in [16 g, 16 g + 16), zero elsewhere: the sum of
  any set of levels is exactly the bit mask of the set, whatever the order of the additions."""
  G = -(-Z // 16)
  pats = bitmask_patterns(Z)
  M, D = len(pats), 4 * G
  vol = np.zeros((M, Z, D), f32)
  for z in range(Z):
    vol[:, z, 4 * (z // 16):4 * (z // 16) + 4] = 2.0 ** (z % 16)
  valid = np.stack(list(pats.values()))
  vol[~valid] = NONFINITE[np.arange((~valid).sum()) % 4][:, None]      # (what an invalid level holds is not read)
  return dict(name=f'bitmask_Z{Z}', vol=vol, valid=valid, patterns=tuple(pats), exact=True)


def bitmask_expected(Z):
  """The masks themselves, from the patterns alone: [M, groups] integers."""
  pats = bitmask_patterns(Z)
  G = -(-Z // 16)
  out = np.zeros((len(pats), G), np.int64)
  for i, v in enumerate(pats.values()):
    for z in np.nonzero(v)[0]:
      out[i, z // 16] |= 1 << (z % 16)
  return out


def _rng(*key):
  return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _pollute(vol, valid, rng):
  bad = ~valid
  vol[bad] = NONFINITE[rng.integers(0, 4, (int(bad.sum()), vol.shape[-1]))]
  return vol


@functools.lru_cache(maxsize=None)
def pool_cases():
  cases = [bitmask_case(Z) for Z in BITMASK_Z]
  # integer-valued columns: few distinct values, so maxima are tied within and across the two half-waves, in invalid
  # levels, in one channel of a quad only; then the planted columns
  for Z, D, M in ((5, 8, 9), (33, 4, 5), (64, 8, 9), (70, 8, 5)):
    rng = _rng('ties', Z, D, M)
    vol = rng.integers(-3, 4, (M, Z, D)).astype(f32)
    valid = rng.random((M, Z)) < 0.6
    valid[0] = True
    vol[0] = 2.0                                         # a constant column: ties = Z
    valid[1] = False
    valid[1, [0, Z - 1]] = True                          # first and last level valid, nothing between
    vol[1, 0], vol[1, Z - 1] = 1.0, 5.0                  # the maximum in the last valid level
    vol[1, 1:Z - 1] = 9.0                                # (larger values in invalid levels: not the maximum, not counted)
    valid[2] = True
    vol[2] = -np.inf                                     # every valid level -inf: plane -inf, valid 1
    valid[3, :4] = True
    vol[3, :4] = 0.0
    vol[3, 1, 0] = vol[3, 2, 0] = 7.0                    # ranks 1 (half 1) and 2 (half 0) tie in channel 0 alone
    vol[3, 0, 1] = np.inf
    vol[3, 3, 2] = -np.inf
    vol[3, 4:] = -5.0
    valid[4] = False                                     # nothing valid
    vol = _pollute(vol, valid, rng)
    vol[1, 1:Z - 1] = 9.0
    best = holders_64(vol, valid)[0]
    for m in range(5, M):                                # the maximum once more in an invalid level: not counted
      if valid[m].any() and not valid[m].all():
        vol[m, np.nonzero(~valid[m])[0][0]] = best[m]
    cases.append(dict(name=f'ties_Z{Z}_D{D}_M{M}', vol=vol, valid=valid, exact=True))
  # a NaN in a valid level reaches exactly its channel of its column
  rng = _rng('nan')
  for Z in (7, 64, 70):
    vol = rng.standard_normal((5, Z, 8)).astype(f32)
    valid = rng.random((5, Z)) < 0.7
    valid[:, 2] = True
    vol = _pollute(vol, valid, rng)
    vol[3, 2, 5] = np.nan
    cases.append(dict(name=f'nan_Z{Z}', vol=vol, valid=valid, exact=False, nan_at=(3, 5)))
  # shapes: every D on both kernels, ragged workgroups of 4 and 8 columns
  for i, D in enumerate((4, 8, 124, 128, 132, 252, 256)):
    for Z in (6, 66):
      M = (1, 3, 5, 9)[(i + (Z > 64)) % 4]
      rng = _rng('shape', D, Z)
      vol = rng.standard_normal((M, Z, D)).astype(f32)
      valid = rng.random((M, Z)) < 0.7
      cases.append(dict(name=f'shape_D{D}_Z{Z}_M{M}', vol=_pollute(vol, valid, rng), valid=valid, exact=False))
  # model-like widths, few cells; the same with offset features
  for Z in (60, 12):
    for off in (0.0, 1000.0):
      rng = _rng('scene', Z)
      vol = (off + rng.standard_normal((40, Z, 128))).astype(f32)
      valid = rng.random((40, Z)) < 0.5
      valid[:2] = False
      cases.append(dict(name=f'scene_Z{Z}_off{int(off)}', vol=vol, valid=valid, exact=False, random=True))
  rngs = _rng('dplane')
  for c in cases:
    M, _, D = c['vol'].shape
    c['dplane'] = rngs.integers(-4, 5, (M, D)).astype(f32) if c['exact'] else rngs.standard_normal((M, D)).astype(f32)
  return tuple(cases)


EPS17 = 2.0 ** -17


def _dyadic(rng, shape, lo=-2, hi=2):
  return (rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.integers(lo, hi + 1, shape)).astype(f32)


@functools.lru_cache(maxsize=None)
def fuse_cases():
  cases = []

  def add(name, planes, valids, Wm=None, bm=None, normalize=True, eps=1e-5, poolings=POOLINGS, dyadic=False, **kw):
    rng = _rng('fusegrad', name)
    M, D = planes[0].shape
    draw = (lambda s: rng.integers(-4, 5, s).astype(f32)) if dyadic else (lambda s: rng.standard_normal(s).astype(f32))
    cases.append(dict(name=name, planes=planes, valids=valids, Wm=Wm, bm=bm, normalize=normalize, eps=eps,
                      poolings=poolings, dyadic=dyadic, dfused=draw((M, D)),
                      dmatching=None if Wm is None else draw((M, Wm.shape[1])), **kw))

  # shapes x plane counts x a None mask in every position x Dm; cells covered by 0, 1, all planes; integer-valued
  # planes so that rows tie between planes (covering and not)
  for i, D in enumerate((4, 8, 124, 128, 132, 252, 256)):
    n = 1 + i % 4
    M = (1, 3, 5, 9)[i % 4]
    Dm = (1, 5, 31, 32)[(i + 1) % 4]
    rng = _rng('fuse', D)
    planes = [rng.integers(-2, 3, (M, D)).astype(f32) for _ in range(n)]
    valids = [rng.random(M) < 0.6 for _ in range(n)]
    if n > 1:
      valids[i % n] = None
      planes[0][-1] = planes[n - 1][-1]                  # equal rows in two planes of the last cell
    for p, v in zip(planes, valids):
      if v is not None:
        p[~v] = NONFINITE[np.arange(D) % 4]              # what a non-covering plane holds is not read ...
    if n > 1 and valids[0] is not None and M > 1:
      valids[0][0] = False
      planes[0][0] = planes[1][0]                        # ... not even when it equals the maximum
    add(f'int_D{D}_n{n}_M{M}_Dm{Dm}', planes, valids, _dyadic(rng, (D, Dm)), _dyadic(rng, (Dm,)), normalize=False, dyadic=True)
    planes = [(p + np.where(np.isfinite(p), 0.25 * rng.standard_normal(p.shape), 0)).astype(f32) for p in planes]
    add(f'float_D{D}_n{n}_M{M}_Dm{Dm}', planes, valids, (rng.standard_normal((D, Dm)) / np.sqrt(D)).astype(f32),
        rng.standard_normal(Dm).astype(f32))
  # four planes, every coverage count
  rng = _rng('cover')
  M, D = 16, 8
  planes = [rng.integers(-2, 3, (M, D)).astype(f32) for _ in range(4)]
  valids = [np.array([(m >> p) & 1 for m in range(M)], bool) for p in range(4)]
  planes[2][:] = planes[1]                               # planes 1 and 2 hold equal rows everywhere
  add('cover_n4', planes, valids, _dyadic(rng, (D, 5)), _dyadic(rng, (5,)), normalize=False, dyadic=True)
  add('cover_n4_nohead', planes, valids, dyadic=True)
  # the normalisation at eps = 2^-17: y = x (identity head, zero bias).  Row 0: the norm is exactly eps, not invalid,
  # 0.5 each.  Row 1, one component an ulp smaller: the ulp is half an ulp of the f32 sum of squares and rounds
  # away (ties to even), the f32 norm is eps again and the row is NOT invalid, although its float64 norm is below
  # eps -- the branch is the f32 norm's (module docstring).  Row 2, two ulps smaller: below eps in both, zero.
  a = f32(2.0 ** -18)
  a1 = np.nextafter(a, f32(0))
  x = np.array([[a, a, a, a], [a, a, a, a1], [a, a, np.nextafter(a1, f32(0)), a],
                [np.nextafter(a, f32(1)), a, a, a], [0, 0, 0, 0], [1, 0, 0, 0]], f32)
  add('norm_at_eps_Dm4', [x], [None], np.eye(4, dtype=f32), np.zeros(4, f32), eps=EPS17, poolings=('sum',), norm_case=True)
  x1 = np.array([[EPS17, 0, 0, 0], [np.nextafter(f32(EPS17), f32(0)), 0, 0, 0], [3, 0, 0, 0]], f32)
  add('norm_at_eps_Dm1', [x1], [None], np.eye(4, dtype=f32)[:, :1].copy(), np.zeros(1, f32), eps=EPS17, poolings=('sum',),
      norm_case=True)
  add('zero_vector_default_eps', [np.zeros((3, 8), f32)], [None], _dyadic(rng, (8, 5)), np.zeros(5, f32), poolings=('max', 'sum'))
  # model-like widths, with and without an offset
  for off in (0.0, 1000.0):
    rng = _rng('fscene')
    planes = [(off + rng.standard_normal((48, 128))).astype(f32) for _ in range(3)]
    valids = [rng.random(48) < 0.6, None if off else rng.random(48) < 0.6, rng.random(48) < 0.6]
    valids[0][:2] = False
    valids[2][:2] = False
    if valids[1] is not None:
      valids[1][:2] = False
    add(f'scene_off{int(off)}', planes, valids, (rng.standard_normal((128, 32)) / np.sqrt(128)).astype(f32),
        rng.standard_normal(32).astype(f32), random=True)
  return tuple(cases)


PERSISTENT_SIZES = (8191, 8192, 8193, 8192 + 8 + 1, 16385)


@functools.lru_cache(maxsize=None)
def persistent_case(M):
  """D = 128 with a head at the persistent threshold: two planes of small integers (dyadic head: exact), cells
  covered by 0, 1, 2 planes in turn, one NaN row in a covering plane; the last cells carry distinct rows."""
  rng = _rng('persistent', M)
  planes = [rng.integers(-2, 3, (M, 128)).astype(f32) for _ in range(2)]
  valids = [np.arange(M) % 3 != 0, np.arange(M) % 4 != 0]
  nan_cell = 7                                           # covered by both planes
  planes[0][nan_cell] = np.nan
  for m in (M - 1, min(8191, M - 1), min(8192, M - 1)):
    valids[0][m] = valids[1][m] = True
  return dict(name=f'persistent_M{M}', planes=planes, valids=valids, Wm=_dyadic(rng, (128, 32)), bm=_dyadic(rng, (32,)),
              normalize=True, eps=1e-5, poolings=('max', 'mean'), dyadic=True, nan_cell=nan_cell,
              dfused=rng.integers(-4, 5, (M, 128)).astype(f32), dmatching=rng.integers(-4, 5, (M, 32)).astype(f32))


CONF_HEAD_SCORES = (0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0)


@functools.lru_cache(maxsize=None)
def conf_head_cases():
  cases = []
  for i, D in enumerate((4, 128, 132, 256, 260)):
    rng = _rng('chead', D)
    M = len(CONF_HEAD_SCORES) + (2, 4, 6, 10, 3)[i]
    w = rng.standard_normal(D).astype(f32)
    f = rng.standard_normal((M, D)).astype(f32)
    b = np.array([0.25], f32)
    for k, s in enumerate(CONF_HEAD_SCORES):             # rows whose score is (about) s
      f[k] = ((s - 0.25) * f64(w) / (f64(w) ** 2).sum()).astype(f32)
    valid = None if i % 2 else rng.random(M) < 0.7
    if valid is not None:
      valid[:len(CONF_HEAD_SCORES)] = True
      valid[-1] = False
      f[-1] = 1e30                                       # (finite: 0 * NaN would reach d w, as it does in the reference's VJP)
    cases.append(dict(name=f'chead_D{D}_M{M}', f=f, valid=valid, w=w, b=b, g=rng.standard_normal(M).astype(f32)))
  return tuple(cases)


@functools.lru_cache(maxsize=None)
def conf_pool_cases():
  """Levels f_z = a_z u + noise orthogonal to w with u = w / |w|^2, so that the raw score of level z is a_z."""
  cases = []
  shapes = [(1, 4, 1), (2, 124, 8), (31, 128, 9), (32, 4, 17), (33, 124, 9), (64, 128, 17)]
  for Z, D, M in shapes:
    rng = _rng('cpool', Z, D, M)
    w = rng.standard_normal(D)
    u = w / (w ** 2).sum()
    noise = rng.standard_normal((M, Z, D))
    if D > 1:
      noise -= (noise @ w)[..., None] * u
    a = rng.uniform(-4, 4, (M, Z))
    valid = rng.random((M, Z)) < 0.6
    cols = np.arange(M)
    a[cols % 8 == 1] = np.linspace(-80, 80, Z)           # rising along z: the running shift moves at every level
    a[cols % 8 == 2] = np.linspace(80, -80, Z)           # falling: it is set once
    a[cols % 8 == 3] = np.linspace(-80, -1, Z)           # all negative: the shift stays at its floor 0
    valid[(cols % 8 >= 1) & (cols % 8 <= 3)] = True
    a[cols % 8 == 4] = 1.5                               # equal scores: weights 1 / n
    valid[cols % 8 == 4, 0] = True
    valid[cols % 8 == 5] = False
    valid[cols % 8 == 5, Z // 2] = True                  # one valid level: weight exactly 1
    valid[cols % 8 == 6] = False                         # no valid level
    if Z >= 2:
      a[cols % 8 == 7, 0], a[cols % 8 == 7, 1:] = 60.0, -60.0     # weights that underflow to exactly 0
      valid[cols % 8 == 7, :2] = True
    vol = (a[..., None] * u + noise).astype(f32)
    vol[(cols % 8 == 4)] = (1.5 * u).astype(f32)         # (equal rows, so the scores are equal bit for bit)
    cases.append(dict(name=f'cpool_Z{Z}_D{D}_M{M}', vol=vol, valid=valid, w=w.astype(f32), b=np.array([0.0], f32),
                      dplane=rng.standard_normal((M, D)).astype(f32), kinds=cols % 8))
  for Z in (60, 12):
    for off in (0.0, 1000.0):
      rng = _rng('cscene', Z)
      vol = (off + rng.standard_normal((24, Z, 128))).astype(f32)
      valid = rng.random((24, Z)) < 0.5
      valid[0] = False
      w = (rng.standard_normal(128) / (np.sqrt(128) * (1 + off / 10))).astype(f32)
      cases.append(dict(name=f'cscene_Z{Z}_off{int(off)}', vol=vol, valid=valid, w=w, b=np.array([-0.5], f32),
                        dplane=rng.standard_normal((24, 128)).astype(f32), kinds=None))
  return tuple(cases)


def kernels_reached():
  """Which kernel each case of the table takes, by the dispatch rule: kernel -> case names."""
  hit = {k: [] for k in KERNELS}
  for c in pool_cases():
    _, Z, D = c['vol'].shape
    hit[pool_kernel(Z, D)].append(c['name'])
    hit[pool_kernel(Z, D, 'max', True)].append(c['name'])
    hit[pool_bwd_kernel(False)].append(c['name'])
    if pool_kernel(Z, D, 'max', True) == 'vertical_pool_max_arg_kernel':
      hit[pool_bwd_kernel(True)].append(c['name'])
  for c in list(fuse_cases()) + [persistent_case(M) for M in PERSISTENT_SIZES]:
    M, D = c['planes'][0].shape
    for bwd in (False, True):
      hit[fuse_kernel(M, D, c['Wm'] is not None, bwd)].append(c['name'])
  for c in conf_head_cases():
    hit['confidence_head_kernel'].append(c['name'])
    hit['confidence_head_bwd_kernel'].append(c['name'])
  for c in conf_pool_cases():
    hit['conf_pool_kernel'].append(c['name'])
    hit['conf_pool_bwd_kernel'].append(c['name'])
  return hit
