"""The VJP kernels of ``encoder_bwd.hip`` (and the forward multi-launch of weight standardisation) in float64, with
per-element bounds that come from the reference alone, float32 restatements in the kernels' own summation order, the
restated launcher decisions and the cases `test_encoder_vjp_reference.py` (CPU) and `test_gpu_encoder_vjp.py` (GPU)
share.  numpy / torch float64; imports nothing of ``snap_amd``.

Bounds.  ``U = 2^-24``; a sum of n f32 terms t_i is held to ``gamma(n) sum abs(t_i)`` with n the longest chain the kernel
can form for the shape, propagated to first order through the formulas; every bound is a sum of MAGNITUDES.  The bound
of an operation is multiplied by ``MULT[op]``, the smallest power of two that keeps the f32 restatement at or below 0.5
over all cases (the CPU file asserts that it is that power of two); a GPU result passes at ``ratio <= 1``.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GN_RELU, RELU_GN = 'gn_relu', 'relu_gn'
GATE_MARGIN = 2.0 ** -10
F32 = np.float32

# smallest power of two with (f32 restatement's worst error / (MULT * bound)) <= 0.5 -- measured by the CPU file, which
# fails if an entry is not that power of two
MULT = {
    'gn_dx': 2.0 ** -1, 'gn_dgamma': 2.0 ** 0, 'gn_dbeta': 2.0 ** -1,
    'ws_fwd': 2.0 ** 1, 'ws_bwd': 2.0 ** 0,
    'colsum': 2.0 ** -4, 'wsum': 2.0 ** -5, 'dtail': 2.0 ** -2,
    'upsample': 2.0 ** -1, 'maxpool': 2.0 ** 0,
}


def gamma_n(n):
  n = np.asarray(n, np.float64)
  return n * U / (1.0 - n * U)


def f64(a):
  return np.asarray(a, np.float64)


def ratio(got, ref, bound, op):
  """max abs(got - ref) / (MULT[op] * bound); an error where the bound is 0 counts as inf (the element is exact)."""
  err = np.abs(f64(got) - f64(ref))
  b = MULT[op] * f64(bound)
  with np.errstate(divide='ignore', invalid='ignore'):
    r = np.where(err == 0, 0.0, err / b)
  r = np.where(np.isfinite(r), r, np.inf)
  return float(r.max()) if r.size else 0.0


def bits_equal(a, b):
  a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
  return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def same_values(a, b):
  """Equal as numbers (+0 == -0): what 'bit for bit' means for a sum that may come out as either zero."""
  return a.shape == b.shape and bool((np.asarray(a) == np.asarray(b)).all())


# ----------------------------------------------------------------------------------------------------
# the launchers, restated
# ----------------------------------------------------------------------------------------------------
def cdiv(a, b):
  return (a + b - 1) // b


def gn_plan_b(N, HW, C):
  """(slabs per image, pixels per slab) of gn_bwd_partial_kernel."""
  chunks = cdiv(C, 1024)
  S = cdiv(1024, N * chunks)
  S = max(1, min(S, cdiv(HW, 8), 256))
  ppb = cdiv(HW, S)
  return cdiv(HW, ppb), ppb


def quad_layout(C):
  """(QW, PW): column quads and row phases of a 256-thread workgroup over a chunk of <= 1024 columns."""
  QW = min(C, 1024) // 4
  return QW, 256 // QW


def gn_reduce_path(N, C, groups):
  if N <= 0 or C <= 0 or groups <= 0 or C % groups or C % 4:
    return 'rejected'
  chunks = cdiv(C, 1024)
  if chunks > 1 and C % 1024:
    return 'rejected'
  if 256 % (min(C, 1024) // 4):
    return 'rejected'
  cpg = C // groups
  if cpg <= 16 and 16 % cpg == 0 and C % 16 == 0 and N * 16 * 8 <= 64 * 1024:
    return 'group16'
  if cpg <= 64 and 64 % cpg == 0 and C % 64 == 0 and N * 64 * 8 <= 64 * 1024:
    return 'group64'
  return 'two_kernel'


def gn_lds_bytes(N, C, groups):
  return {'group16': N * 16 * 8, 'group64': N * 64 * 8}.get(gn_reduce_path(N, C, groups), 0)


def colsum_slabs(M):
  return int(max(1, min(cdiv(M, 512), 2048)))


def epilogue_colsum_path(C):
  """'fused' (epilogue_bwd_colsum_kernel) or 'fallback' (epilogue_bwd + colsum) of ops_bwd.epilogue_bwd_colsum (f32)."""
  if C % 4:
    return 'rejected'
  q = C // 4 if C < 1024 else 256
  return 'fallback' if (256 % q or (C > 1024 and C % 1024)) else 'fused'


def colsum_kernel(C):
  """The partial kernel of snap_colsum_rows_f32 (16-byte aligned tensor)."""
  return 'v4' if (C % 4 == 0 and C <= 1024) else 'scalar'


def maxpool_path(N, C, aligned=True):
  v4 = C % 4 == 0 and aligned
  if v4 and N <= 65535 and cdiv(C, 64) <= 65535:
    return 'tiled'
  return 'vec4' if v4 else 'scalar'


def wstd_table(shapes, cols=32):
  """block_begin of every item and the total workgroup count of a multi launch over HWIO shapes."""
  begin, blk = [], 0
  for s in shapes:
    begin.append(blk)
    blk += cdiv(s[3], cols)
  return begin, blk


def wstd_lookup(begin, blk, mutant=None):
  """The item a workgroup serves: the kernels' binary search (last item with block_begin <= blk)."""
  lo, hi = 0, len(begin) - 1
  while lo < hi:
    mid = (lo + hi + 1) >> 1
    ok = begin[mid] < blk if mutant == 'table_off_by_one' else begin[mid] <= blk
    if ok:
      lo = mid
    else:
      hi = mid - 1
  return lo


# ----------------------------------------------------------------------------------------------------
# GroupNorm VJP
# ----------------------------------------------------------------------------------------------------
def gn_stats_f32(x, groups, relu_first, eps=1e-5):
  """float64 two-pass statistics of x [N, HW, C], rounded to f32 and spread over the channels -> mu, rstd [N, C]."""
  v = f64(x)
  if relu_first:
    v = np.maximum(v, 0)
  N, HW, C = v.shape
  g = v.reshape(N, HW, groups, C // groups)
  mean = g.mean(axis=(1, 3))
  var = ((g - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
  rep = lambda t: np.repeat(t, C // groups, axis=1).astype(F32)
  return rep(mean), rep(1.0 / np.sqrt(var + eps))


def gn_gate_offenders(x, gam, beta, mode, groups, mu, rstd):
  """Elements whose ReLU decision lies within GATE_MARGIN of its scale (float64) -> boolean [N, HW, C]."""
  x, mu, rstd, gam, beta = f64(x), f64(mu)[:, None, :], f64(rstd)[:, None, :], f64(gam), f64(beta)
  if mode == GN_RELU:
    t = (x - mu) * rstd * gam
    return np.abs(t + beta) < GATE_MARGIN * (np.abs(t) + np.abs(beta))
  N, HW, C = x.shape
  spread = x.reshape(N, HW, groups, C // groups).std(axis=(1, 3))
  spread = np.repeat(spread, C // groups, axis=1)[:, None, :]
  return np.abs(x) < GATE_MARGIN * spread


def gn_settle_gate(x, gam, beta, mode, groups, stats):
  """Nudge x [N, HW, C] (f32) until no element sits within the gate margin under the statistics ``stats(x)`` returns
  (they move with x, hence the loop) -> x, mu, rstd, nudged count."""
  x = np.array(x, F32)
  moved = 0
  for _ in range(8):
    mu, rstd = stats(x)
    bad = gn_gate_offenders(x, gam, beta, mode, groups, mu, rstd)
    if not bad.any():
      return x, mu, rstd, moved
    moved += int(bad.sum())
    if mode == GN_RELU:
      xh = (f64(x) - f64(mu)[:, None, :]) * f64(rstd)[:, None, :]
      need = 8 * GATE_MARGIN * (np.abs(xh * f64(gam)) + np.abs(f64(beta)))           # raise abs(z) to 8 margins
      step = need / (np.abs(f64(gam)) * f64(rstd)[:, None, :])
      x = np.where(bad, x + np.sign(f64(gam)) * step, x).astype(F32)
    else:
      N, HW, C = x.shape
      spread = np.repeat(f64(x).reshape(N, HW, groups, C // groups).std(axis=(1, 3)), C // groups, axis=1)[:, None, :]
      x = np.where(bad, np.where(x < 0, -1.0, 1.0) * 8 * GATE_MARGIN * spread, x).astype(F32)
  raise AssertionError('gate margin not reached')


def gn_chain(N, HW, C, chain=None):
  """Longest f32 chain of a per-(n, c) partial sum: rows per phase + phases + slabs."""
  if chain is not None:
    return chain
  S, ppb = gn_plan_b(N, HW, C)
  _, PW = quad_layout(C)
  return cdiv(ppb, PW) + PW + S


def gn_vjp_ref(x, dz, add, gam, beta, mode, groups, mu, rstd, chain=None):
  """float64 VJP as the header of encoder_bwd.hip defines it, with the f32 mu / rstd [N, C] the kernel is given.
  x, dz, add [N, HW, C].  -> {name: (ref, bound)} for dx, dgamma, dbeta."""
  x, dz, gam, beta = f64(x), f64(dz), f64(gam), f64(beta)
  N, HW, C = x.shape
  cpg = C // groups
  m, r = f64(mu)[:, None, :], f64(rstd)[:, None, :]
  if mode == GN_RELU:
    xh = (x - m) * r
    dyp = np.where(xh * gam + beta > 0, dz, 0.0)
  else:
    xh = (np.maximum(x, 0) - m) * r
    dyp = dz
  A, Bs = dyp.sum(axis=1), (dyp * xh).sum(axis=1)                                  # [N, C]
  absA, absB = np.abs(dyp).sum(axis=1), np.abs(dyp * xh).sum(axis=1)
  grp = lambda t: np.repeat(t.reshape(N, groups, cpg).sum(axis=2), cpg, axis=1)[:, None, :]
  S1, S2 = grp(gam * A), grp(gam * Bs)
  absS1, absS2 = grp(np.abs(gam) * absA), grp(np.abs(gam) * absB)
  inv = 1.0 / (HW * cpg)
  core = r * (dyp * gam - S1 * inv - xh * (S2 * inv))
  if mode == RELU_GN:
    core = np.where(x > 0, core, 0.0)
  dx = core + (0.0 if add is None else f64(add))
  n = gn_chain(N, HW, C, chain)
  # xh carries two roundings and dyp * xh one more: three extra links in the chain of Bs
  bS1 = gamma_n(n + cpg + 1) * absS1
  bS2 = gamma_n(n + 3 + cpg + 1) * absS2
  # apply expression: dyp * g (1), S * inv_cnt (inv_cnt 1 + product 1), xh (2) * (.) (1), two subtractions, times rstd
  mag = np.abs(dyp * gam) + absS1 * inv + np.abs(xh) * absS2 * inv
  b = np.abs(r) * (bS1 * inv + np.abs(xh) * bS2 * inv + 8 * U * mag)
  if mode == RELU_GN:
    b = np.where(x > 0, b, 0.0)
  if add is not None:
    b = b + U * (np.abs(core) + np.abs(f64(add)))
  return {
      'dx': (dx, b),
      'dgamma': (Bs.sum(axis=0), gamma_n(n + 3 + N) * absB.sum(axis=0)),
      'dbeta': (A.sum(axis=0), gamma_n(n + N) * absA.sum(axis=0)),
  }


def gn_vjp_f32(x, dz, add, gam, beta, mode, groups, mu, rstd, mutant=None):
  """The kernels' arithmetic in numpy f32, in their order: gn_bwd_partial_kernel (a phase sums every PW-th pixel of its
  slab, phases ascending), the reduce pass (slabs ascending; channels of a group ascending; images ascending) and
  gn_bwd_apply_kernel.  Both reduce paths take these orders.  mutant: 'drop_phase' (phase 1 of every slab is left out),
  'drop_last_slab', 'wrong_inv_cnt' (1 / (N HW cpg)), 'gate_ge'."""
  x, dz = np.asarray(x, F32), np.asarray(dz, F32)
  gam, beta, mu, rstd = (np.asarray(t, F32) for t in (gam, beta, mu, rstd))
  N, HW, C = x.shape
  cpg = C // groups
  S, ppb = gn_plan_b(N, HW, C)
  _, PW = quad_layout(C)
  m, r = mu[:, None, :], rstd[:, None, :]
  if mode == GN_RELU:
    xh = (x - m) * r
    z = xh * gam + beta
    dyp = np.where(z >= 0 if mutant == 'gate_ge' else z > 0, dz, F32(0))
  else:
    xh = (np.maximum(x, F32(0)) - m) * r
    dyp = dz
  t2 = dyp * xh
  a1 = np.zeros((N, C), F32)
  a2 = np.zeros((N, C), F32)
  for s in range(S - 1 if mutant == 'drop_last_slab' else S):
    lo, hi = s * ppb, min((s + 1) * ppb, HW)
    steps = cdiv(hi - lo, PW)
    pad = np.zeros((N, steps * PW - (hi - lo), C), F32)
    b1 = np.concatenate([dyp[:, lo:hi], pad], axis=1).reshape(N, steps, PW, C)
    b2 = np.concatenate([t2[:, lo:hi], pad], axis=1).reshape(N, steps, PW, C)
    s1 = np.zeros((N, PW, C), F32)
    s2 = np.zeros((N, PW, C), F32)
    for k in range(steps):
      s1 += b1[:, k]
      s2 += b2[:, k]
    p1 = np.zeros((N, C), F32)
    p2 = np.zeros((N, C), F32)
    for pp in range(min(PW, hi - lo)):                     # (the idle phases add zeros)
      if mutant == 'drop_phase' and pp == 1:
        continue
      p1 += s1[:, pp]
      p2 += s2[:, pp]
    a1 += p1
    a2 += p2
  S1 = np.zeros((N, groups), F32)
  S2 = np.zeros((N, groups), F32)
  g1, g2 = (gam * a1).reshape(N, groups, cpg), (gam * a2).reshape(N, groups, cpg)
  for c in range(cpg):
    S1 += g1[:, :, c]
    S2 += g2[:, :, c]
  dgamma = np.zeros(C, F32)
  dbeta = np.zeros(C, F32)
  for n in range(N):
    dgamma += a2[n]
    dbeta += a1[n]
  S1 = np.repeat(S1, cpg, axis=1)[:, None, :]
  S2 = np.repeat(S2, cpg, axis=1)[:, None, :]
  cnt = F32(HW) * F32(cpg) * (F32(N) if mutant == 'wrong_inv_cnt' else F32(1))
  inv = F32(1) / cnt
  d = r * (dyp * gam - S1 * inv - xh * (S2 * inv))
  if mode == RELU_GN:
    d = np.where(x >= 0 if mutant == 'gate_ge' else x > 0, d, F32(0))
  if add is not None:
    d = d + np.asarray(add, F32)
  return {'dx': d.astype(F32), 'dgamma': dgamma, 'dbeta': dbeta}


# name, N, H, W, C, groups, reduce path, (S, ppb), with add
GN_CASES = [
    ('cpg1-slabs5+4', 3, 3, 3, 32, 32, 'group16', (2, 5), True),
    ('cpg16-one-slab', 2, 7, 1, 512, 32, 'group16', (1, 7), False),
    ('c1024-one-phase', 2, 3, 3, 1024, 32, 'group64', (2, 5), True),
    ('c2048-two-chunks', 2, 3, 2, 2048, 32, 'group64', (1, 6), False),
    ('groups1-c128', 2, 9, 7, 128, 1, 'two_kernel', (8, 8), True),
    ('groups2-c8', 3, 5, 4, 8, 2, 'two_kernel', (3, 7), False),
    ('c4-256-phases', 2, 20, 15, 4, 1, 'two_kernel', (38, 8), True),
    ('lds16-at-64K', 512, 2, 1, 32, 32, 'group16', (1, 2), False),
    ('lds16-above-64K', 513, 2, 1, 32, 32, 'two_kernel', (1, 2), False),
    ('lds64-at-64K', 128, 1, 2, 1024, 32, 'group64', (1, 2), False),
    ('lds64-above-64K', 129, 1, 2, 1024, 32, 'two_kernel', (1, 2), False),
    ('hw2049-capped-ragged', 1, 3, 683, 32, 32, 'group16', (228, 9), True),
    ('n1025-one-slab', 1025, 2, 1, 32, 32, 'two_kernel', (1, 2), False),
]
GN_CASE_IDS = [c[0] for c in GN_CASES]
GN_MODES = (GN_RELU, RELU_GN)
GN_FUSED_SHAPES = [(3, 17, 17, 64, 256, 1, GN_RELU, False), (2, 13, 11, 128, 128, 3, GN_RELU, True)]
GN_OFFSET_SHAPE = (2, 9, 7, 64)


def _seed(name):
  return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def gn_case(name, mode):
  """The random case `name` under `mode`: x is settled against the statistics of float64 rounded to f32 (the mu / rstd
  the kernel is handed) -> dict."""
  _, N, H, W, C, groups, path, plan, with_add = next(c for c in GN_CASES if c[0] == name)
  rng = np.random.default_rng(_seed(name) + (0 if mode == GN_RELU else 1000))
  HW = H * W
  x = (rng.standard_normal((N, HW, C)) * 1.5 + 0.4).astype(F32)
  gam = (rng.standard_normal(C) * 0.3 + 1).astype(F32)
  beta = (rng.standard_normal(C) * 0.2).astype(F32)
  dz = rng.standard_normal((N, HW, C)).astype(F32)
  add = rng.standard_normal((N, HW, C)).astype(F32) if with_add else None
  relu_first = mode == RELU_GN
  x, mu, rstd, moved = gn_settle_gate(x, gam, beta, mode, groups, lambda v: gn_stats_f32(v, groups, relu_first))
  return dict(name=name, mode=mode, shape=(N, H, W, C), groups=groups, path=path, plan=plan, x=x, dz=dz, add=add,
              gamma=gam, beta=beta, mu=mu, rstd=rstd, moved=moved)


def gn_offset_inputs(mode, offset_field):
  """The offset field of `groupnorm_reference` (group means at up to 256 standard deviations, constant groups, under
  RELU_GN a group that is negative throughout) with parameters and cotangents; statistics are the caller's."""
  N, H, W, C = GN_OFFSET_SHAPE
  x, planted = offset_field(N, H * W, C, 811, relu_first=mode == RELU_GN)
  rng = np.random.default_rng(812)
  gam = (rng.standard_normal(C) * 0.3 + 1).astype(F32)
  beta = (rng.standard_normal(C) * 0.2).astype(F32)
  dz = rng.standard_normal((N, H * W, C)).astype(F32)
  add = rng.standard_normal((N, H * W, C)).astype(F32)
  return dict(name='offset', mode=mode, shape=(N, H, W, C), groups=32, path='group16', x=x.astype(F32), dz=dz, add=add,
              gamma=gam, beta=beta, planted=planted)


GN_EXACT = [(64, 32), (8, 2)]          # (C, groups): group16 and two_kernel


def gn_exact_case(mode, C=64, groups=32, N=3, H=4, W=4):
  """mu = 0, rstd = 1, gamma in {1, 0, -1}, beta = 0, small-integer x (with +0.0 and -0.0) and dz, cnt = HW * cpg a
  power of two: every product, sum and quotient is exactly representable, so f32 in any order equals float64."""
  rng = np.random.default_rng(77 + (mode == RELU_GN) + C)
  HW = H * W
  assert (HW * (C // groups)) & (HW * (C // groups) - 1) == 0
  x = rng.integers(-3, 4, (N, HW, C)).astype(F32)
  x[:, ::3, ::5] = F32(0.0)
  x[:, 1::3, ::5] = -F32(0.0)
  gam = np.array([1, 0, -1, 1], F32)[np.arange(C) % 4]
  gam[1::8] = F32(-1)
  beta = np.zeros(C, F32)
  dz = rng.integers(-4, 5, (N, HW, C)).astype(F32)
  mu = np.zeros((N, C), F32)
  rstd = np.ones((N, C), F32)
  return dict(name=f'exact-c{C}', mode=mode, shape=(N, H, W, C), groups=groups, path=gn_reduce_path(N, C, groups), x=x,
              dz=dz, add=None, gamma=gam, beta=beta, mu=mu, rstd=rstd)


def gn_args(c):
  return (c['x'], c['dz'], c['add'], c['gamma'], c['beta'], c['mode'], c['groups'], c['mu'], c['rstd'])


# ----------------------------------------------------------------------------------------------------
# weight standardisation
# ----------------------------------------------------------------------------------------------------
WS_EPS = 1e-10
WS_SHAPES = [(1, 1, 1, 5), (1, 1, 31, 33), (1, 1, 32, 32), (1, 1, 33, 31), (3, 3, 20, 36), (7, 7, 3, 64), (1, 1, 64, 200)]
WS_OFFSET_SHAPE = (3, 3, 20, 36)
WS_OFFSETS = (0.0, 1e2, 1e4)
# multi launches: indices into WS_SHAPES; one-block items next to many-block items, first and last
WS_MULTI = {'one': [4], 'two': [6, 0], 'seven': [0, 6, 1, 4, 5, 3, 2]}


def ws_case(shape, offset=0.0, seed=0):
  rng = np.random.default_rng(9000 + seed + sum(shape) + int(offset))
  K = shape[0] * shape[1] * shape[2]
  s = 0.05
  w = (offset * s + s * rng.standard_normal((K, shape[3]))).astype(F32)
  dws = rng.standard_normal((K, shape[3])).astype(F32)
  return dict(shape=shape, w=w, dws=dws, offset=offset)


def ws_ref(w, dws=None, eps=WS_EPS):
  """w, dws [K, Cout].  -> {'fwd': (ws, bound), 'bwd': (dw, bound), 'mean_round': [Cout]}.  The statistics are the
  kernels' one-pass sums around the pivot w[0, col], f32 per k-slice and combined in double; the f32 mean then carries
  the rounding ``mean_round = abs(mean) 2^-24 / sigma`` (in units of ws), stated on its own: it shifts every ws of the
  column by the same amount and enters dw through ``ws * mean(dws ws)`` and ``mean(dws ws)``."""
  w = f64(w)
  K, Cout = w.shape
  mean = w.mean(axis=0)
  var = ((w - mean) ** 2).mean(axis=0)
  sigma = np.sqrt(var + eps)
  ws = (w - mean) / sigma
  t = w - w[0]
  n = cdiv(K, 32) + 2                                     # a slice's chain, t itself rounded, t * t rounded
  err_m = gamma_n(n) * np.abs(t).sum(axis=0) / K
  m = t.mean(axis=0)
  err_var = gamma_n(n) * (t * t).sum(axis=0) / K + 2 * np.abs(m) * err_m
  e_sig = 0.5 * err_var / (var + eps) + 3 * U             # (float)var, + eps, sqrtf
  mean_round = np.abs(mean) * U / sigma
  shift = mean_round + err_m / sigma                      # error of (w - mean) / sigma that is common to the column
  b_ws = shift + np.abs(ws) * (e_sig + 2 * U)            # (w - mean) and the division: one rounding each
  out = {'fwd': (ws, b_ws), 'mean_round': mean_round}
  if dws is not None:
    g = f64(dws)
    n1 = cdiv(K, 32) + 32 + 1                             # slice chain, 32 slices in order, times 1 / K
    mg, mgw = g.mean(axis=0), (g * ws).mean(axis=0)
    ag, agw = np.abs(g).mean(axis=0), np.abs(g * ws).mean(axis=0)
    b_mg = gamma_n(n1) * ag
    b_mgw = gamma_n(n1 + 1) * agw + ag * shift + agw * (e_sig + 2 * U)
    dw = (g - mg - ws * mgw) / sigma
    b = (b_mg + np.abs(ws) * b_mgw + b_ws * np.abs(mgw) + 4 * U * (np.abs(g) + np.abs(mg) + np.abs(ws * mgw))) / sigma \
        + np.abs(dw) * (e_sig + U)
    out['bwd'] = (dw, b)
  return out


def _ws_stats_f32(w, K, eps, slices, kdiv):
  Cout = w.shape[1]
  steps = cdiv(K, slices)
  live = (np.arange(steps * slices) < K).reshape(steps, slices, 1)
  piv = w[0]
  t = np.concatenate([w - piv, np.zeros((steps * slices - K, Cout), F32)]).reshape(steps, slices, Cout)
  s1 = np.zeros((slices, Cout), F32)
  s2 = np.zeros((slices, Cout), F32)
  for k in range(steps):
    s1 += np.where(live[k], t[k], F32(0))
    s2 += np.where(live[k], t[k] * t[k], F32(0))
  t1 = np.zeros(Cout)
  t2 = np.zeros(Cout)
  for i in range(slices):
    t1 += s1[i].astype(np.float64)
    t2 += s2[i].astype(np.float64)
  m = t1 / kdiv
  var = t2 / kdiv - m * m
  mean = (piv.astype(np.float64) + m).astype(F32)
  sigma = np.sqrt(np.maximum(var, 0.0).astype(F32) + F32(eps)).astype(F32)
  return mean, sigma


def ws_fwd_f32(w, eps=WS_EPS, mutant=None, quads=None):
  """weight_std_body_v4 (quads: the item's Cout % 4 == 0; 128 k-slices) / weight_std_body (32 k-slices) in f32."""
  w = np.asarray(w, F32)
  K, Cout = w.shape
  quads = Cout % 4 == 0 if quads is None else quads
  kdiv = cdiv(K, 32) * 32 if mutant == 'k_rounded_up' else K
  mean, sigma = _ws_stats_f32(w, K, eps, 128 if quads else 32, kdiv)
  return ((w - mean) / sigma).astype(F32)


def ws_bwd_f32(w, dws, eps=WS_EPS, mutant=None):
  """weight_std_bwd_body in f32: statistics over 32 k-slices, the two gradient means (a slice's sum in k order, the 32
  slices in order, times 1 / K) and the output.  mutant 'k_rounded_up': every mean divides by K rounded up to 32."""
  w, g = np.asarray(w, F32), np.asarray(dws, F32)
  K, Cout = w.shape
  kdiv = cdiv(K, 32) * 32 if mutant == 'k_rounded_up' else K
  mean, sigma = _ws_stats_f32(w, K, eps, 32, kdiv)
  ws = (w - mean) / sigma
  steps = cdiv(K, 32)
  padn = steps * 32 - K
  gp = np.concatenate([g, np.zeros((padn, Cout), F32)]).reshape(steps, 32, Cout)
  gw = np.concatenate([g * ws, np.zeros((padn, Cout), F32)]).reshape(steps, 32, Cout)
  s1 = np.zeros((32, Cout), F32)
  s2 = np.zeros((32, Cout), F32)
  for k in range(steps):
    s1 += gp[k]
    s2 += gw[k]
  t1 = np.zeros(Cout, F32)
  t2 = np.zeros(Cout, F32)
  for i in range(32):
    t1 += s1[i]
    t2 += s2[i]
  ik = F32(1) / F32(kdiv)
  mg, mgw = t1 * ik, t2 * ik
  return ((g - mg - ws * mgw) / sigma).astype(F32)


def ws_multi_f32(ws_list, dws_list=None, eps=WS_EPS, mutant=None):
  """A multi launch: every workgroup looks its item up in the table and runs the single-kernel body on its 32 columns.
  Outputs start as NaN: a column no workgroup reaches stays NaN."""
  shapes = [(1, 1) + w.shape for w in ws_list]
  begin, total = wstd_table(shapes)
  outs = [np.full(w.shape, np.nan, F32) for w in ws_list]
  for blk in range(total):
    it = wstd_lookup(begin, blk, mutant)
    lo = (blk - begin[it]) * 32
    w = ws_list[it]
    if lo >= w.shape[1]:
      continue
    if dws_list is None:
      # (the body is chosen by the ITEM's column count; the columns themselves are independent)
      outs[it][:, lo:lo + 32] = ws_fwd_f32(w[:, lo:lo + 32], eps, quads=w.shape[1] % 4 == 0)
    else:
      outs[it][:, lo:lo + 32] = ws_bwd_f32(w[:, lo:lo + 32], dws_list[it][:, lo:lo + 32], eps)
  return outs


# ----------------------------------------------------------------------------------------------------
# gate + column sums
# ----------------------------------------------------------------------------------------------------
COLSUM_C_FUSED = (4, 256, 1024, 2048)
COLSUM_C_FALLBACK = (12, 1028)
COLSUM_M = (1, 511, 513, 1025)
COLSUM_RAGGED = (2051, 4)
HALF_C = (4, 256, 1024)


def round_half(a, kind):
  """f32 -> bf16 / fp16 -> float32 (round to nearest even; torch's conversion)."""
  t = torch.from_numpy(np.ascontiguousarray(a, F32))
  return t.to(torch.bfloat16 if kind == 'bf16' else torch.float16).float().numpy()


def colsum_case(M, C, seed=0, exact=False):
  """dy, y [M, C], a row mask: y holds +0.0, -0.0 and NaN (all gated off) besides random signs."""
  rng = np.random.default_rng(4000 + 7 * M + C + seed)
  if exact:
    dy = rng.integers(-8, 9, (M, C)).astype(F32)
    y = rng.integers(-2, 3, (M, C)).astype(F32)
  else:
    dy = rng.standard_normal((M, C)).astype(F32)
    y = rng.standard_normal((M, C)).astype(F32)
  flat = y.reshape(-1)
  flat[0::7] = F32(0.0)
  flat[3::11] = -F32(0.0)
  flat[5::13] = np.nan
  mask = (rng.random(M) < 0.7).astype(np.uint8)
  return dict(M=M, C=C, dy=dy, y=y, mask=mask)


def row_counts(M):
  return [None, 0, 1, M, M + 5]


def colsum_chain(M, C, kernel='fused'):
  S = colsum_slabs(M)
  rpb = cdiv(M, S)
  if kernel == 'scalar':
    return rpb + cdiv(S, 8) + 8
  QW, PW = (C // 4, 256 // (C // 4)) if kernel == 'v4' else quad_layout(C)
  return cdiv(rpb, PW) + PW + cdiv(S, 8) + 8


def gate_ref(dy, y, mask, relu, row_count, kernel='fused', weight=None):
  """-> out [M, C] (exact: an element is kept or zeroed), Msum, (sums, bound) over the first Msum rows; with `weight`
  [M] (already rounded) also (wsum, bound)."""
  dy = f64(dy)
  M, C = dy.shape
  out = dy.copy()
  if mask is not None:
    out = out * (np.asarray(mask) != 0)[:, None]
  if relu:
    with np.errstate(invalid='ignore'):
      out = np.where(f64(y) > 0, out, 0.0)
  Msum = M if row_count is None else min(int(row_count), M)
  n = colsum_chain(M, C, kernel)
  res = dict(out=out, Msum=Msum, sums=(out[:Msum].sum(axis=0), gamma_n(n) * np.abs(out[:Msum]).sum(axis=0)))
  if weight is not None:
    t = f64(weight)[:Msum, None] * out[:Msum]
    res['wsum'] = (t.sum(axis=0), gamma_n(n + 1) * np.abs(t).sum(axis=0))
  return res


def _phase_sums(rows, tree4):
  """rows [cnt, P, C] f32: every phase's sum over its cnt rows, in order (tree4: colsum_partial_v4_kernel's
  t += (v0 + v1) + (v2 + v3) while four rows remain)."""
  cnt = rows.shape[0]
  t = np.zeros(rows.shape[1:], F32)
  k = 0
  if tree4:
    while k + 3 < cnt:
      t = t + ((rows[k] + rows[k + 1]) + (rows[k + 2] + rows[k + 3]))
      k += 4
  while k < cnt:
    t = t + rows[k]
    k += 1
  return t


def colsum_f32(out, Msum, kernel='fused', mutant=None):
  """Column sums of out[:Msum] (f32 values) in the order of epilogue_bwd_colsum_kernel ('fused'), of
  colsum_partial_v4_kernel ('v4') or of colsum_partial_kernel ('scalar'), then colsum_reduce_kernel (slab s in group
  s % 8, a group in order, the eight groups in order).  mutant: 'drop_phase' (phase 1), 'drop_last_slab'."""
  out = np.asarray(out, F32)
  M, C = out.shape
  S = colsum_slabs(M)
  rpb = cdiv(M, S)
  partial = np.zeros((S, C), F32)
  for s in range(S):
    r0, r1 = s * rpb, min(Msum, (s + 1) * rpb)
    if r1 <= r0:
      continue
    if kernel == 'scalar':
      partial[s] = _phase_sums(out[r0:r1, None, :], False)[0]
      continue
    PW = 256 // (C // 4) if kernel == 'v4' else quad_layout(C)[1]
    acc = np.zeros(C, F32)
    for pp in range(min(PW, r1 - r0)):
      if mutant == 'drop_phase' and pp == 1:
        continue
      acc = acc + _phase_sums(out[r0 + pp:r1:PW, None, :], kernel == 'v4')[0]
    partial[s] = acc
  if mutant == 'drop_last_slab':
    partial = partial[:-1]
    S -= 1
  red = np.zeros((8, C), F32)
  for s in range(S):
    red[s % 8] += partial[s]
  r = np.zeros(C, F32)
  for i in range(8):
    r = r + red[i]
  return r


def dtail_ref(out, wtail):
  """(dot [M], bound): out [M, 256] (rounded gate output) . wtail [256] (rounded): per thread ((g0 w0 + g1 w1) + (g2 w2
  + g3 w3)), then 4 rotations in a row of 16 lanes and a tree over the four rows: 1 + 2 + 4 + 2 links."""
  t = f64(out) * f64(wtail)[None, :]
  return t.sum(axis=1), gamma_n(9) * np.abs(t).sum(axis=1)


def dtail_f32(out, wtail):
  p = (np.asarray(out, F32) * np.asarray(wtail, F32)[None, :]).reshape(out.shape[0], 64, 4)
  v = (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])               # [M, 64 lanes]
  v = v.reshape(-1, 4, 16)
  for rot in (8, 4, 2, 1):
    v = v + np.roll(v, rot, axis=2)
  return ((v[:, 0, 0] + v[:, 1, 0]) + (v[:, 2, 0] + v[:, 3, 0])).astype(F32)


# ----------------------------------------------------------------------------------------------------
# bilinear x2 up-sample VJP
# ----------------------------------------------------------------------------------------------------
UP_SHAPES = [(1, 1, 1, 4), (2, 1, 5, 8), (1, 4, 1, 4), (2, 3, 5, 20), (1, 2, 2, 4)]


def up_matrix(Hp, mutant=None, dtype=np.float64):
  """A [2 Hp, Hp]: fine = A coarse for F.interpolate(scale_factor=2, 'bilinear', align_corners=False), by the kernel's
  rule (two taps, both clamped; at a border both land on one pixel and BOTH count).  mutant 'border_once'."""
  A = np.zeros((2 * Hp, Hp), dtype)
  for ho in range(2 * Hp):
    sh = (ho + 0.5) * 0.5 - 0.5
    fh = math.floor(sh)
    w1 = sh - fh
    h0, h1 = min(max(fh, 0), Hp - 1), min(max(fh + 1, 0), Hp - 1)
    if mutant == 'border_once' and h0 == h1:
      A[ho, h0] += 1 - w1
    else:
      A[ho, h0] += 1 - w1
      A[ho, h1] += w1
  return A


def up_ref(dy):
  """dy [N, 2 Hp, 2 Wp, C] -> (dprev, bound): at most 4 x 4 taps per coarse pixel, weights exact, one rounding per
  product."""
  dy = f64(dy)
  N, Ho, Wo, C = dy.shape
  Ah, Aw = up_matrix(Ho // 2), up_matrix(Wo // 2)
  ref = np.einsum('hp,nhwc,wq->npqc', Ah, dy, Aw)
  mass = np.einsum('hp,nhwc,wq->npqc', Ah, np.abs(dy), Aw)
  return ref, gamma_n(17) * mass


def up_f32(dy, mutant=None):
  """upsample2x_bwd_kernel: acc += (wh * ww) * g over ho = 2 hp - 2 ... 2 hp + 2, wo likewise, zero weights skipped."""
  dy = np.asarray(dy, F32)
  N, Ho, Wo, C = dy.shape
  Hp, Wp = Ho // 2, Wo // 2
  Ah, Aw = up_matrix(Hp, mutant, F32), up_matrix(Wp, mutant, F32)
  acc = np.zeros((N, Hp, Wp, C), F32)
  for hp in range(Hp):
    for wp in range(Wp):
      a = np.zeros((N, C), F32)
      for ho in range(max(2 * hp - 2, 0), min(2 * hp + 2, Ho - 1) + 1):
        if Ah[ho, hp] == 0:
          continue
        for wo in range(max(2 * wp - 2, 0), min(2 * wp + 2, Wo - 1) + 1):
          if Aw[wo, wp] == 0:
            continue
          a = a + F32(Ah[ho, hp] * Aw[wo, wp]) * dy[:, ho, wo, :]
      acc[:, hp, wp, :] = a
  return acc


# ----------------------------------------------------------------------------------------------------
# 3 x 3 / 2 max-pool VJP
# ----------------------------------------------------------------------------------------------------
POOL_SHAPES = [((1, 1, 1, 4), 'tiled'), ((1, 2, 1, 4), 'tiled'), ((1, 16, 17, 4), 'tiled'), ((2, 33, 32, 68), 'tiled'),
               ((1, 9, 9, 3), 'scalar')]


def pool_case(shape, seed=0, ties=True):
  N, H, W, C = shape
  rng = np.random.default_rng(600 + seed + H * 37 + W)
  Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  if ties:
    x = rng.integers(-3, 4, shape).astype(F32)
    dy = rng.integers(-5, 6, (N, Ho, Wo, C)).astype(F32)
  else:
    x = rng.permutation(N * H * W * C).reshape(shape).astype(F32)
    dy = rng.standard_normal((N, Ho, Wo, C)).astype(F32)
  return x, dy


def pool_special_planes(shape, seed=0):
  """x with channel 0 = -inf in whole windows (the top-left 5 x 5 pixels and the last two rows), channel 1 constant;
  integer dy."""
  x, dy = pool_case(shape, seed + 1)
  x[:, :5, :5, 0] = -np.inf
  x[:, -2:, :, 0] = -np.inf
  if shape[3] > 1:
    x[..., 1] = F32(2.0)
  return x, dy


def _pool_routes(x, last=False):
  """For every window and channel the flat input pixel that takes the gradient: the first (mutant: last) maximum among
  the window's in-bounds positions in scan order -> idx [N, Ho, Wo, C] into H * W."""
  N, H, W, C = x.shape
  Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  vals = np.full((9, N, Ho, Wo, C), -np.inf)
  ok = np.zeros((9, 1, Ho, Wo, 1), bool)
  pix = np.zeros((9, 1, Ho, Wo, 1), np.int64)
  ho, wo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing='ij')
  for p in range(9):
    h2, w2 = 2 * ho - 1 + p // 3, 2 * wo - 1 + p % 3
    inb = (h2 >= 0) & (h2 < H) & (w2 >= 0) & (w2 < W)
    hc, wc = np.clip(h2, 0, H - 1), np.clip(w2, 0, W - 1)
    vals[p] = np.where(inb[None, :, :, None], x[:, hc, wc, :], -np.inf)
    ok[p, 0, :, :, 0] = inb
    pix[p, 0, :, :, 0] = hc * W + wc
  best = vals.max(axis=0)
  hit = ok & (vals == best[None])
  order = hit[::-1] if last else hit
  sel = order.argmax(axis=0)
  if last:
    sel = 8 - sel
  return np.take_along_axis(np.broadcast_to(pix, vals.shape), sel[None], axis=0)[0]


def pool_ref(x, dy, dtype=np.float64, last=False):
  """dx: every window sends its dy to its first maximum; a pixel adds its windows in (ho, wo) order.  NaN-free x."""
  x = f64(x)
  N, H, W, C = x.shape
  idx = _pool_routes(x, last)
  dx = np.zeros((N, H * W, C), dtype)
  n = np.arange(N)[:, None, None, None]
  c = np.arange(C)[None, None, None, :]
  n, c = np.broadcast_to(n, idx.shape), np.broadcast_to(c, idx.shape)
  np.add.at(dx, (n.reshape(-1), idx.reshape(-1), c.reshape(-1)), np.asarray(dy, dtype).reshape(-1))
  return dx.reshape(N, H, W, C)


def pool_bound(x, dy):
  return gamma_n(4) * pool_ref(x, np.abs(f64(dy)))


def pool_autograd(x, dy):
  xd = torch.from_numpy(f64(x)).requires_grad_(True)
  F.max_pool2d(xd.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).backward(torch.from_numpy(f64(dy)))
  return xd.grad.numpy()


# ----------------------------------------------------------------------------------------------------
# torch autograd restatements (the CPU file pins the float64 formulas to them)
# ----------------------------------------------------------------------------------------------------
def gn_autograd(x, dz, gam, beta, mode, groups, eps=1e-5):
  """-> dx, dgamma, dbeta, mu, rstd [N, C] (float64) through a hand-written GroupNorm(+ReLU)."""
  xd = torch.from_numpy(f64(x)).requires_grad_(True)
  gd = torch.from_numpy(f64(gam)).requires_grad_(True)
  bd = torch.from_numpy(f64(beta)).requires_grad_(True)
  N, HW, C = xd.shape
  v = torch.relu(xd) if mode == RELU_GN else xd
  g = v.reshape(N, HW, groups, C // groups)
  mean = g.mean((1, 3), keepdim=True)
  var = ((g - mean) ** 2).mean((1, 3), keepdim=True)
  z = ((g - mean) / torch.sqrt(var + eps)).reshape(N, HW, C) * gd + bd
  if mode == GN_RELU:
    z = torch.relu(z)
  z.backward(torch.from_numpy(f64(dz)))
  rep = lambda t: t.detach().reshape(N, groups).repeat_interleave(C // groups, dim=1).numpy()
  return xd.grad.numpy(), gd.grad.numpy(), bd.grad.numpy(), rep(mean), rep(1 / torch.sqrt(var + eps))


def ws_autograd(w, dws, eps=WS_EPS):
  wd = torch.from_numpy(f64(w)).requires_grad_(True)
  mean = wd.mean(0, keepdim=True)
  var = ((wd - mean) ** 2).mean(0, keepdim=True)
  ws = (wd - mean) / torch.sqrt(var + eps)
  ws.backward(torch.from_numpy(f64(dws)))
  return ws.detach().numpy(), wd.grad.numpy()


def up_autograd(dy):
  N, Ho, Wo, C = dy.shape
  p = torch.zeros((N, C, Ho // 2, Wo // 2), dtype=torch.float64, requires_grad=True)
  up = F.interpolate(p, scale_factor=2, mode='bilinear', align_corners=False)
  up.backward(torch.from_numpy(f64(dy)).permute(0, 3, 1, 2))
  return p.grad.permute(0, 2, 3, 1).numpy()


# ----------------------------------------------------------------------------------------------------
# shared inputs of the smaller cases
# ----------------------------------------------------------------------------------------------------
def colsum_kernel_of(C):
  """The summation order a width takes through ops_bwd.epilogue_bwd_colsum (f32)."""
  return 'fused' if epilogue_colsum_path(C) == 'fused' else colsum_kernel(C)


def half_case(M, C, kind, exact=False):
  """dy, y rounded to `kind`, the row weights source x2 [M + 3, 260] (channel 256 read through a shuffled row list,
  ReLU'd by the kernel) and the tail weights [C]."""
  c = colsum_case(M, C, seed=1, exact=exact)
  rng = np.random.default_rng(31 * M + C)
  x2 = (rng.integers(-3, 4, (M + 3, 260)) if exact else rng.standard_normal((M + 3, 260))).astype(F32)
  rows = rng.permutation(M + 3)[:M].astype(np.int32)
  wt = (rng.integers(-2, 3, C) if exact else rng.standard_normal(C)).astype(F32)
  return dict(M=M, C=C, dy=round_half(c['dy'], kind), y=round_half(c['y'], kind), x2=x2, rows=rows, wtail=wt)


def half_weight(h, kind, wrelu):
  w = h['x2'][h['rows'], 256]
  if wrelu:
    w = np.maximum(w, F32(0))
  return round_half(w, kind)


def up_case(shape, exact=False):
  N, Hp, Wp, C = shape
  rng = np.random.default_rng(50 + 7 * Hp + Wp)
  if exact:
    return rng.integers(-8, 9, (N, 2 * Hp, 2 * Wp, C)).astype(F32)
  return rng.standard_normal((N, 2 * Hp, 2 * Wp, C)).astype(F32)


def gate_variants_f32(C):
  """Every (M, case, use_mask, row_count, relu) both test files run at width C."""
  Ms = list(COLSUM_M) + ([COLSUM_RAGGED[0]] if C == COLSUM_RAGGED[1] else [])
  for M in Ms:
    c = colsum_case(M, C)
    for use_mask in (False, True):
      for rc in row_counts(M):
        for relu in (False, True):
          yield M, c, use_mask, rc, relu


def gate_variants_half(C, kind):
  """Every (M, exact, case, row_count, relu) of the half kernels at width C."""
  for M in COLSUM_M:
    for exact in (False, True):
      h = half_case(M, C, kind, exact=exact)
      for rc in ([None] if exact else row_counts(M)):
        for relu in (False, True):
          yield M, exact, h, rc, relu


def ws_multi_cases(name):
  return [ws_case(WS_SHAPES[i], seed=j) for j, i in enumerate(WS_MULTI[name])]
