"""A float64 numpy restatement of ``snap_vote_pairs_f32`` (include/snap_hip.h), written from the contract, not from the
kernel, in two parts.

(a) ``vote_pairs``: the separable form, plain slices over whole planes
----------------------------------------------------------------------
``belief``, ``nxt`` f32 [R, Ho, Wo], ``taps`` the filter's tuple for the step, ``uniform_mix`` = eps, n = R Ho Wo.

* PREDICT: p, M (``vote_filter_reference.masses``, the f32 decisions exactly); t0, t1, t2 the three tap passes, each
  a float64 sum rounded to f32 ONCE where the kernel stores it (the kernel's are f32 fma chains); S = sum t2;
  prior = ((1 - eps) t2) / S + eps / n (first term 0 when S == 0).
* RATIO as ``vote_smooth_reference``: lg = nxt - log(prior) where nxt is finite and prior > 0, G = max lg,
  q = fl32(exp(lg - G)) iff fl32(lg - G) >= -40, Q = sum q.
* ADJOINT: c0 = the b gather of q, c1 = the a gather of c0 (``vote_smooth_reference``'s c1 and c0), rounded to f32 once.
* HISTOGRAMS: Hb[r, tb] = taps_b[r, tb] sum q[r, a, b] t1[r, a, b + lb[r] + tb]; Ha[r, ta] = taps_a[r, ta] sum
  c0[r, a, b] t0[r, a + la[r] + ta, b]; Hk[tk] = taps_k[tk] sum c1[r, a, b] p[(r + lk + tk) mod R, a, b]; float64,
  the products not rounded (the kernel rounds each term's two products to f32).
* FINISH, the contract's float64 expressions in the contract's order: H = sum_tk Hk in index order, c = (1 - eps) / S,
  stay_raw = c H, jump_raw = (eps / n) Q, total = stay_raw + jump_raw, hist = (c Hraw) / total, stay, jump,
  log_norm = G + log(total), mass_kept = fl32(S / sum p); all 0 and log_norm -inf when total == 0.
* count = (cells of belief with mass, NaN / +inf cells of belief, NaN / +inf cells of nxt, cells of nxt with ratio
  mass).

With ``rounded=False`` nothing above the masses is rounded to f32 (q and the intermediates stay float64): the form the
brute-force enumeration (b) is compared with at float64 noise.

The error bound (``bounds``), derived, not measured
--------------------------------------------------
u = 2^-24, gamma(m) = m u / (1 - m u).  Every term is non-negative (no cancellation), so relative errors pass through
the sums and absolute errors through the linear maps.

* t0, t1, t2, S: the kernel's chains are within gamma(Tk + Ta + Tb + 2) of exact (``vote_filter_reference``), this
  file's three single roundings and numpy's exp within gamma(5): the two sides differ by at most g_t = gamma(Tk + Ta +
  Tb + 7) relative, on every intermediate and on S.
* q: as ``vote_smooth_reference``: rho = 2 g_t / (1 - g_t), e_p = -log(1 - rho A / prior), e_G = max e_p,
  e_q = e_p + e_G, dq = q (expm1(e_q) (1 + 2 u) + 2 u) + [within e_q + 2^-18 of the cut] exp(-40 + e_q + 2^-18).
* A raw histogram is linear in its ratio-side operand and in its predict-side operand: with the ratio side off by d
  (absolute, per cell) and the predict side by g_t (relative), and each term's two f32 products by 2 u (4 u allowed):
  dH = (1 + pe) H[d] + pe H[.], pe = g_t + 4 u, H[d] the same histogram with d in place of the ratio-side operand.
  d = dq for Hb; for Ha the adjoint column pass adds its chain (Tb links) and this file's rounding: dc0 = adj_b(dq)
  (1 + gamma(Tb + 2)) + gamma(Tb + 2) c0; for Hk likewise dc1 = adj_a(dc0) (1 + gamma(Ta + 2)) + gamma(Ta + 2) c1.
* c = (1 - eps) / S is off by g_S = g_t / (1 - g_t): dN = c (dH (1 + g_S) + g_S H) for N = c H.  dJ = (eps / n) sum dq.
  total T = c sum Hk + J: dT = sum dN_k + dJ.  A normalised value v = N / T is off by at most (dN + v dT) / (T - dT)
  (no bound where dT >= T).  log_norm: e_G + dT / (T - dT).  mass_kept: the filter's bound with g_t.
* float64 noise: 2^-50 relative per value, n 2^-53 on the sums.

The tests allow twice the bound.  With ``exact=True`` (``vote_smooth_reference.exact_case``: p, t0, t1, t2, q, c0, c1
and every product are dyadic and exact on both sides, eps = 0) the histograms, stay and jump are the same float64
operations on the same numbers: their bound is 0; log_norm keeps the float64 noise of G and log.

(b) ``dense_pairs``: brute-force enumeration
--------------------------------------------
Every (x', tk, ta, tb) of a tiny lattice, one Python loop each: the joint N[r', tk, ta, tb], the jump mass J and the
full xi[x, x'] (row = the pose at t, column = the pose at t + 1), from ``belief`` and gamma_{t+1} given in LINEAR
space as float64.  Nothing of the separable structure, the adjoint or the max-shift G is in it.
"""
import math

import numpy as np

import vote_filter_reference as flt
import vote_smooth_reference as smo
from vote_filter_reference import CUT, U, _F64, masses


def _tables(taps):
  taps_k, lk, taps_a, taps_b, offsets = taps
  taps_k, taps_a, taps_b = (np.asarray(t, np.float32).astype(np.float64) for t in (taps_k, taps_a, taps_b))
  return taps_k, int(lk), taps_a, taps_b, np.asarray(offsets, np.int64)


def _fl32(x):
  return x.astype(np.float32).astype(np.float64)


def _span(s, n):
  """Destination range [x0, x1) with sources x + s inside [0, n)."""
  return max(0, -s), min(n, n - s)


def passes(p, taps, rounded=True):
  """-> (t0, t1, t2), each rounded to f32 once where ``rounded``."""
  taps_k, lk, taps_a, taps_b, offsets = _tables(taps)
  rnd = _fl32 if rounded else (lambda x: x)
  R, Ho, Wo = p.shape
  t0 = np.zeros_like(p)
  for r in range(R):
    for tk in range(len(taps_k)):
      t0[r] += taps_k[tk] * p[(r + lk + tk) % R]
  t0 = rnd(t0)
  t1 = np.zeros_like(p)
  for r in range(R):
    for ta in range(taps_a.shape[1]):
      a0, a1 = _span(int(offsets[r, 0]) + ta, Ho)
      if a0 < a1:
        s = int(offsets[r, 0]) + ta
        t1[r, a0:a1] += taps_a[r, ta] * t0[r, a0 + s:a1 + s]
  t1 = rnd(t1)
  t2 = np.zeros_like(p)
  for r in range(R):
    for tb in range(taps_b.shape[1]):
      s = int(offsets[r, 1]) + tb
      b0, b1 = _span(s, Wo)
      if b0 < b1:
        t2[r, :, b0:b1] += taps_b[r, tb] * t1[r, :, b0 + s:b1 + s]
  return t0, t1, rnd(t2)


def adj_b(q, taps):
  """c0[r, a, b] = sum_tb taps_b[r, tb] q[r, a, b - lb[r] - tb], float64."""
  _, _, _, taps_b, offsets = _tables(taps)
  Wo = q.shape[2]
  out = np.zeros_like(q)
  for r in range(q.shape[0]):
    for tb in range(taps_b.shape[1]):
      s = int(offsets[r, 1]) + tb
      b0, b1 = _span(s, Wo)                                 # sources b0 .. b1 scatter to b0 + s .. b1 + s
      if b0 < b1:
        out[r, :, b0 + s:b1 + s] += taps_b[r, tb] * q[r, :, b0:b1]
  return out


def adj_a(c, taps):
  """c1[r, a, b] = sum_ta taps_a[r, ta] c0[r, a - la[r] - ta, b], float64."""
  _, _, taps_a, _, offsets = _tables(taps)
  Ho = c.shape[1]
  out = np.zeros_like(c)
  for r in range(c.shape[0]):
    for ta in range(taps_a.shape[1]):
      s = int(offsets[r, 0]) + ta
      a0, a1 = _span(s, Ho)
      if a0 < a1:
        out[r, a0 + s:a1 + s] += taps_a[r, ta] * c[r, a0:a1]
  return out


def hist_b(q, t1, taps):
  _, _, _, taps_b, offsets = _tables(taps)
  R, _, Wo = q.shape
  out = np.zeros((R, taps_b.shape[1]))
  for r in range(R):
    for tb in range(taps_b.shape[1]):
      s = int(offsets[r, 1]) + tb
      b0, b1 = _span(s, Wo)
      if b0 < b1:
        out[r, tb] = taps_b[r, tb] * (q[r, :, b0:b1] * t1[r, :, b0 + s:b1 + s]).sum()
  return out


def hist_a(c0, t0, taps):
  _, _, taps_a, _, offsets = _tables(taps)
  R, Ho, _ = c0.shape
  out = np.zeros((R, taps_a.shape[1]))
  for r in range(R):
    for ta in range(taps_a.shape[1]):
      s = int(offsets[r, 0]) + ta
      a0, a1 = _span(s, Ho)
      if a0 < a1:
        out[r, ta] = taps_a[r, ta] * (c0[r, a0:a1] * t0[r, a0 + s:a1 + s]).sum()
  return out


def hist_k(c1, p, taps):
  taps_k, lk, _, _, _ = _tables(taps)
  R = c1.shape[0]
  out = np.zeros(len(taps_k))
  for tk in range(len(taps_k)):
    out[tk] = taps_k[tk] * sum((c1[r] * p[(r + lk + tk) % R]).sum() for r in range(R))
  return out


def _finish(w):
  """The contract's FINISH, its float64 expressions in its order."""
  Hk, Ha, Hb, S, eps, n = w['Hk'], w['Ha'], w['Hb'], w['S'], w['eps'], w['n']
  H = 0.0
  for v in Hk:
    H += float(v)
  c = (1.0 - eps) / S if S > 0 else 0.0
  stay_raw, jump_raw = c * H, (eps / n) * w['Q']
  total = stay_raw + jump_raw
  kept = float(np.float32(S / w['sum_p'])) if w['sum_p'] > 0 else 0.0
  if total > 0:
    out = ((c * Hk) / total, (c * Ha) / total, (c * Hb) / total,
           np.array([stay_raw / total, jump_raw / total, w['G'] + math.log(total), kept]))
  else:
    out = (np.zeros_like(Hk), np.zeros_like(Ha), np.zeros_like(Hb), np.array([0.0, 0.0, -np.inf, kept]))
  w.update(c=c, total=total)
  return out


def _walk(belief, nxt, taps, uniform_mix, rounded=True):
  belief, nxt = np.asarray(belief), np.asarray(nxt)
  assert belief.dtype == np.float32 and nxt.dtype == np.float32 and belief.shape == nxt.shape and belief.ndim == 3
  n = belief.size
  eps = float(np.float32(uniform_mix))
  rnd = _fl32 if rounded else (lambda x: x)
  p, M, bad, mass = masses(belief)
  t0, t1, t2 = passes(p, taps, rounded)
  S, sum_p = t2.sum(), p.sum()
  A = ((1.0 - eps) * t2) / S if S > 0 else np.zeros(belief.shape)
  prior = A + eps / n
  nx = nxt.astype(np.float64)
  bad_next = int((np.isnan(nx) | (nx == np.inf)).sum())
  has = np.isfinite(nx) & (prior > 0)
  with np.errstate(divide='ignore', invalid='ignore'):
    lg = np.where(has, nx - np.log(prior), -np.inf)
  G = lg[has].max() if has.any() else -np.inf
  q = np.zeros(belief.shape)
  d = np.full(belief.shape, -np.inf)
  if has.any():
    d[has] = lg[has] - G
    keep = has & (d.astype(np.float32) >= CUT)
    q[keep] = rnd(np.exp(d[keep]))
  c0 = rnd(adj_b(q, taps))
  c1 = rnd(adj_a(c0, taps))
  w = dict(p=p, t0=t0, t1=t1, t2=t2, S=S, sum_p=sum_p, A=A, prior=prior, nx=nx, has=has, d=d, q=q, Q=q.sum(), G=G,
           c0=c0, c1=c1, eps=eps, n=n, Hb=hist_b(q, t1, taps), Ha=hist_a(c0, t0, taps), Hk=hist_k(c1, p, taps))
  hk, ha, hb, stats = _finish(w)
  count = np.array([mass, bad, bad_next, has.sum()], np.int64)
  return hk, ha, hb, stats, count, w


def vote_pairs(belief, nxt, taps, uniform_mix=0.0, rounded=True):
  """-> (hist_k [Tk], hist_a [R, Ta], hist_b [R, Tb], stats [4] = (stay, jump, log_norm, mass_kept) float64, count
  int64 [4])."""
  return _walk(belief, nxt, taps, uniform_mix, rounded)[:5]


def _gamma(m):
  return m * U / (1 - m * U)


def bounds(belief, nxt, taps, uniform_mix=0.0, exact=False):
  """-> (b_k [Tk], b_a [R, Ta], b_b [R, Tb], b_stats [4]): the derived bounds of |kernel - reference| (module
  docstring); inf where the bound of the total reaches the total."""
  hk, ha, hb, stats, _, w = _walk(belief, nxt, taps, uniform_mix)
  Tk, Ta, Tb = len(hk), ha.shape[1], hb.shape[1]
  kept_g = 0.0 if exact else _gamma(Tk + Ta + Tb + 7)
  b_kept = ((kept_g + 2 * U) / (1 - 2 * U) + U) * abs(stats[3]) * 1.0001
  if not w['total'] > 0:
    return np.zeros_like(hk), np.zeros_like(ha), np.zeros_like(hb), np.array([0.0, 0.0, 0.0, b_kept])
  noise_ln = _F64 * (abs(w['G']) + abs(math.log(w['total'])) + 1.0) + w['n'] * 2.0 ** -53
  if exact:
    return np.zeros_like(hk), np.zeros_like(ha), np.zeros_like(hb), np.array([0.0, 0.0, noise_ln, b_kept])
  has, n, eps, c, T = w['has'], w['n'], w['eps'], w['c'], w['total']
  g_t = _gamma(Tk + Ta + Tb + 7)
  rho = 2 * g_t / (1 - g_t)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    share = np.where(has, w['A'] / w['prior'], 0.0)
    e_p = np.where(has, -np.log1p(-rho * share), 0.0)
    e_G = e_p.max()
    e_q = e_p + e_G + _F64 * (np.abs(np.where(has, w['nx'], 0.0)) + np.abs(np.where(has, np.log(w['prior']), 0.0))
                              + abs(w['G']))
    near = has & (np.abs(w['d'] - float(CUT)) <= e_q + 2.0 ** -18)
    dq = w['q'] * (np.expm1(e_q) * (1 + 2 * U) + 2 * U) + np.where(near, np.exp(float(CUT) + e_q + 2.0 ** -18), 0.0)
  pe = g_t + 4 * U
  g0, g1 = _gamma(Tb + 2), _gamma(Ta + 2)
  dc0 = adj_b(dq, taps) * (1 + g0) + g0 * w['c0']
  dc1 = adj_a(dc0, taps) * (1 + g1) + g1 * w['c1']
  dHb = (1 + pe) * hist_b(dq, w['t1'], taps) + pe * w['Hb']
  dHa = (1 + pe) * hist_a(dc0, w['t0'], taps) + pe * w['Ha']
  dHk = (1 + pe) * hist_k(dc1, w['p'], taps) + pe * w['Hk']
  g_S = g_t / (1 - g_t) + _F64
  f64 = _F64 + n * 2.0 ** -53
  dN = lambda dH, H: c * (dH * (1 + g_S) + (g_S + f64) * H)
  dNk, dNa, dNb = dN(dHk, w['Hk']), dN(dHa, w['Ha']), dN(dHb, w['Hb'])
  J = (eps / n) * w['Q']
  dJ = (eps / n) * (dq.sum() + f64 * w['Q'])
  dT = dNk.sum() + dJ
  if not dT < T:
    inf = lambda x: np.full_like(x, np.inf)
    return inf(hk), inf(ha), inf(hb), np.array([np.inf, np.inf, np.inf, b_kept])
  rel = lambda dNx, v: (dNx + v * dT) / (T - dT) + _F64 * v
  b_stats = np.array([rel(dNk.sum(), stats[0]), rel(dJ, stats[1]), e_G + dT / (T - dT) + noise_ln, b_kept])
  return rel(dNk, hk), rel(dNa, ha), rel(dNb, hb), b_stats


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def big_case():
  """[64, 97, 89]: R at its limit, P = 8633 (no multiple of 256), 64 * 34 = 2176 tiles > 2048 workgroups, so the
  predict launches stride and the reductions have 32 workgroups per rotation on 34 tiles; Tk = 16, Ta = Tb = 32, the
  tables' limits, with zero taps and offsets of both signs."""
  rng = np.random.default_rng(20261022)
  shape = (64, 97, 89)
  assert shape[0] * -(-shape[1] * shape[2] // flt.TILE) > flt.MAX_GROUPS
  belief = flt._belief(rng, shape, masked=0.1)
  votes = (rng.standard_normal(shape) * 0.25).astype(np.float32)
  votes[:, ~flt.border_mask(shape[1], shape[2])] = -np.inf
  off = np.stack([rng.integers(-28, 4, 64), rng.integers(-30, 2, 64)], -1).astype(np.int32)
  taps = (flt.rand_taps(rng, 1, 16, zeros=0.2)[0], -9, flt.rand_taps(rng, 64, 32, zeros=0.2),
          flt.rand_taps(rng, 64, 32, zeros=0.2), off)
  nxt = flt.vote_filter(belief, votes, taps, 8.0, 1e-3)[0].astype(np.float32)
  return dict(name='big', belief=belief, next=nxt, taps=taps, uniform_mix=1e-3)


def still_case():
  """[3, 4, 5] with one tap of weight 1 per axis (Tk = Ta = Tb = 1) and eps = 0: every histogram is a single 1."""
  rng = np.random.default_rng(3)
  shape = (3, 4, 5)
  still = smo.still_taps(3)
  belief = flt.vote_filter(None, rng.standard_normal(shape).astype(np.float32), still, 3.0, 0.0)[0].astype(np.float32)
  nxt = flt.vote_filter(belief, rng.standard_normal(shape).astype(np.float32), still, 1.0, 0.0)[0].astype(np.float32)
  return dict(name='still', belief=belief, next=nxt, taps=still, uniform_mix=0.0)


def all_inputs():
  """``vote_smooth_reference.all_inputs()`` (``exact`` last among them), then ``still`` and ``big``."""
  return smo.all_inputs() + [still_case(), big_case()]


# ---------------------------------------------------------------------------------------------------------------
# (b) brute force
# ---------------------------------------------------------------------------------------------------------------
def dense_pairs(belief, gamma_next, taps, uniform_mix):
  """``belief`` f32 [R, Ho, Wo] (log alpha_t), ``gamma_next`` float64 [R, Ho, Wo] (gamma_{t+1}, linear) -> (N
  [R, Tk, Ta, Tb] by destination rotation and tap triple, J, xi [n, n] with xi[x, x'] the mass of the pair (pose x at
  t, pose x' at t + 1)); N.sum() + J == xi.sum() == the sum of gamma_next over the cells with a prior."""
  taps_k, lk, taps_a, taps_b, offsets = _tables(taps)
  R, Ho, Wo = belief.shape
  n = belief.size
  eps = float(np.float32(uniform_mix))
  p = masses(belief)[0]
  sum_p = p.sum()
  lin = lambda r, a, b: (r * Ho + a) * Wo + b
  # the prior by the same enumeration: t2 first
  t2 = np.zeros((R, Ho, Wo))
  for r in range(R):
    for a in range(Ho):
      for b in range(Wo):
        for tk in range(len(taps_k)):
          for ta in range(taps_a.shape[1]):
            for tb in range(taps_b.shape[1]):
              sa, sb = a + int(offsets[r, 0]) + ta, b + int(offsets[r, 1]) + tb
              if 0 <= sa < Ho and 0 <= sb < Wo:
                t2[r, a, b] += taps_k[tk] * taps_a[r, ta] * taps_b[r, tb] * p[(r + lk + tk) % R, sa, sb]
  S = t2.sum()
  N = np.zeros((R, len(taps_k), taps_a.shape[1], taps_b.shape[1]))
  xi = np.zeros((n, n))
  J = 0.0
  for r in range(R):
    for a in range(Ho):
      for b in range(Wo):
        prior = ((1 - eps) * t2[r, a, b]) / S + eps / n if S > 0 else eps / n
        if not prior > 0:
          continue
        ratio = gamma_next[r, a, b] / prior
        J += (eps / n) * ratio
        if sum_p > 0:
          xi[:, lin(r, a, b)] += (eps / n) * ratio * (p.reshape(n) / sum_p)
        if not S > 0:
          continue
        for tk in range(len(taps_k)):
          for ta in range(taps_a.shape[1]):
            for tb in range(taps_b.shape[1]):
              k, sa, sb = (r + lk + tk) % R, a + int(offsets[r, 0]) + ta, b + int(offsets[r, 1]) + tb
              if 0 <= sa < Ho and 0 <= sb < Wo:
                m = ((1 - eps) / S) * ratio * taps_k[tk] * taps_a[r, ta] * taps_b[r, tb] * p[k, sa, sb]
                N[r, tk, ta, tb] += m
                xi[lin(k, sa, sb), lin(r, a, b)] += m
  return N, J, xi
