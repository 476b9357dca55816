"""A float64 numpy restatement of ``snap_vote_smooth_f32`` (include/snap_hip.h), written from the contract, not from the
kernel: plain slices over whole planes, one rotation at a time.  Step 1 is ``vote_filter_reference``'s.

The contract, restated
----------------------
``belief [R, Ho, Wo]`` f32 = log alpha_t, ``nxt [R, Ho, Wo]`` f32 = log gamma_{t+1}, ``taps`` the filter's tuple for the
step t -> t + 1, ``uniform_mix`` = eps, n = R Ho Wo.

* PREDICT as the filter: p, M (``masses``), t2 (``predict``), S = sum t2, prior = ((1 - eps) t2) / S + eps / n (first
  term 0 when S == 0).
* RATIO: where nxt is finite and prior > 0, lg = nxt - log(prior); G = max lg; q = fl32(exp(lg - G)) iff
  fl32(lg - G) >= -40, else 0 (the f32 rounding of q is part of the definition, as that of p is); Q = sum q.
* ADJOINT: c1[r, a, b] = sum_tb taps_b[r, tb] q[r, a, b - lb[r] - tb]; c0[r, a, b] = sum_ta taps_a[r, ta] c1[r, a -
  la[r] - ta, b]; u[k, a, b] = sum_tk taps_k[tk] c0[(k - lk - tk) mod R, a, b]; sources outside contribute 0.  Here
  the sums are float64 (every product of two f32 numbers is exact); the kernel's are f32 fma chains.
* COMBINE: h = ((1 - eps) (sum p / S)) u + (eps / n) Q (first term 0 when S == 0); w = (belief + G) + log(h); -inf for
  a -inf belief or h == 0, NaN for a NaN / +inf belief; log_norm = logsumexp over the finite w; smoothed = w - log_norm
  (not rounded here).
* stats = (log_norm, S / sum p (0 when sum p == 0), G, max smoothed); count = (finite cells of smoothed, NaN / +inf
  cells of belief, NaN / +inf cells of nxt, cells of nxt with ratio mass).

The error bound (``bound``), derived, not measured
--------------------------------------------------
u = 2^-24; taps obey the filter's precondition, so nothing is subnormal and every term is non-negative (no
cancellation: absolute errors pass through the linear maps below by applying the maps to them).

* t2, S, sum p as in ``vote_filter_reference``: g = m u / (1 - m u), m = Tk + Ta + Tb + 2, on t2 and on S; 2 u on
  sum p.  A = (1 - eps) t2 / S is off by rho = 2 g / (1 - g) relative, B = eps / n by nothing:
  e_p = |d log(prior)| <= -log(1 - rho A / (A + B)) per cell.
* lg is off by e_p, G (a maximum) by e_G = max e_p, so lg - G by e_q = e_p + e_G (+ float64 noise).  q carries that as
  a RELATIVE error expm1(e_q), plus 2 u (the kernel's and numpy's float64 exp may round to neighbouring f32 numbers).
  Near the cut the decision fl32(lg - G) >= -40 itself can differ: a cell within e_q + 2^-18 (the f32 spacing at 40) of
  the cut may have mass on one side and 0 on the other, an ABSOLUTE error of at most exp(-40 + e_q + 2^-18).
  dq = q (expm1(e_q) (1 + 2 u) + 2 u) + [near the cut] exp(-40 + e_q + 2^-18).
* u: the adjoint is linear with non-negative weights: the kernel's exact-arithmetic u is within adj(dq) of the
  reference's, and its three f32 chains (Tb, Ta, Tk links, every link one rounding) add g_u = m_u u / (1 - m_u u),
  m_u = Tk + Ta + Tb: du = adj(dq) (1 + g_u) + g_u u.  Q is a float64 sum: dQ = sum dq (+ n 2^-53 Q).
* The carried factor (1 - eps) (sum p / S) is off by r_c = (g + 2 u) / (1 - g) relative:
  dh = carried (du + r_c (u + du)) + (eps / n) dQ.  log(h) is then low by at most -log(1 - dh / h) (infinite where
  dh >= h: such a cell may legitimately come out -inf and gets no bound) and high by at most log(1 + dh / h).
* w = belief + G + log(h): e_w = e_G + the error of log(h) (+ float64 noise of the magnitudes).
* log_norm is a logsumexp: with pi = exp(smoothed) it is high by at most log sum pi exp(up_w) and low by at most
  -log sum pi exp(-down_w): e_norm, the larger.  (Not max e_w: a cell of vanishing mass has a large e_w and no weight.)
* The final rounding to f32: u |smoothed|.

bound = e_w + e_norm + float64 terms + u |smoothed| per finite cell.  The tests allow twice that.  ``stats_bound``
gives the same for the four statistics.  With ``exact=True`` (``exact_case``: p, t2, S, q, u, Q are the same bits on
both sides) every term but the float64 noise and the final rounding is dropped.
"""
import math

import numpy as np

import vote_filter_reference as flt
from vote_filter_reference import CUT, U, _F64, _logsumexp, masses, predict

PASSES = 22           # snap_vote_smooth_f32: passes over the volume (include/snap_hip.h)


def adjoint(q, taps):
  """The three adjoint gathers on the ratio masses, float64 -> (c1, c0, u) [R, Ho, Wo]."""
  taps_k, lk, taps_a, taps_b, offsets = taps
  taps_k, taps_a, taps_b = (np.asarray(t, np.float32).astype(np.float64) for t in (taps_k, taps_a, taps_b))
  offsets = np.asarray(offsets, np.int64)
  R, Ho, Wo = q.shape
  c1 = np.zeros_like(q)
  c0 = np.zeros_like(q)
  for r in range(R):
    la, lb = int(offsets[r, 0]), int(offsets[r, 1])
    for tb in range(taps_b.shape[1]):
      s = lb + tb                                           # c1[b] += w * q[b - s]
      b0, b1 = max(0, s), min(Wo, Wo + s)
      if b0 < b1:
        c1[r, :, b0:b1] += taps_b[r, tb] * q[r, :, b0 - s:b1 - s]
    for ta in range(taps_a.shape[1]):
      s = la + ta
      a0, a1 = max(0, s), min(Ho, Ho + s)
      if a0 < a1:
        c0[r, a0:a1] += taps_a[r, ta] * c1[r, a0 - s:a1 - s]
  u = np.zeros_like(q)
  for k in range(R):
    for tk in range(len(taps_k)):
      u[k] += taps_k[tk] * c0[(k - int(lk) - tk) % R]
  return c1, c0, u


def _walk(belief, nxt, taps, uniform_mix):
  belief, nxt = np.asarray(belief), np.asarray(nxt)
  assert belief.dtype == np.float32 and nxt.dtype == np.float32 and belief.shape == nxt.shape and belief.ndim == 3
  n = belief.size
  eps = float(np.float32(uniform_mix))
  p, M, bad, _ = masses(belief)
  t2 = predict(p, taps)
  S, sum_p = t2.sum(), p.sum()
  kept = S / sum_p if sum_p > 0 else 0.0
  A = ((1.0 - eps) * t2) / S if S > 0 else np.zeros(belief.shape)
  B = eps / n
  prior = A + B
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
    q[keep] = np.exp(d[keep]).astype(np.float32).astype(np.float64)
  Q = q.sum()
  _, _, u = adjoint(q, taps)
  carried = (1.0 - eps) * (sum_p / S) if S > 0 else 0.0
  h = carried * u + (eps / n) * Q
  b = belief.astype(np.float64)
  bad_b = np.isnan(b) | (b == np.inf)
  with np.errstate(divide='ignore', invalid='ignore'):
    w = (b + G) + np.log(h)
  w = np.where(bad_b, np.nan, np.where((b == -np.inf) | ~(h > 0), -np.inf, w))
  fin = np.isfinite(w)
  log_norm = _logsumexp(w[fin])
  with np.errstate(invalid='ignore'):
    out = np.where(fin, w - log_norm, w)
  stats = np.array([log_norm, kept, G, out[fin].max() if fin.any() else -np.inf])
  count = np.array([fin.sum(), bad, bad_next, has.sum()], np.int64)
  return out, stats, count, dict(A=A, B=B, prior=prior, nx=nx, has=has, d=d, q=q, Q=Q, u=u, G=G, h=h, b=b, fin=fin,
                                 log_norm=log_norm, n=n, eps=eps, carried=carried, p=p, t2=t2, S=S, sum_p=sum_p)


def vote_smooth(belief, nxt, taps, uniform_mix=0.0):
  """-> (smoothed float64 [R, Ho, Wo], stats float64 [4], count int64 [4])."""
  return _walk(belief, nxt, taps, uniform_mix)[:3]


def smooth_track(beliefs, taps_list, uniform_mix, rounded=True):
  """The backward recursion: beliefs [N] f32 volumes, taps_list[t] the filter's taps INTO frame t (entry 0 unused) ->
  list of N volumes; frame t + 1's result is rounded to f32 before it is frame t's input (as the kernel's is)."""
  out = [None] * len(beliefs)
  out[-1] = np.asarray(beliefs[-1])
  for t in range(len(beliefs) - 2, -1, -1):
    g = vote_smooth(beliefs[t], np.asarray(out[t + 1], np.float32), taps_list[t + 1], uniform_mix)[0]
    out[t] = g.astype(np.float32) if rounded else g
  return out


def _taps_T(taps):
  return len(taps[0]) + np.asarray(taps[2]).shape[1] + np.asarray(taps[3]).shape[1]


def _errors(taps, w, exact):
  """-> (down_w, up_w, e_norm, e_G): how far the kernel's w may lie below / above the reference's per finite cell (0
  elsewhere), the error of log_norm and that of G."""
  shape, fin, has = w['b'].shape, w['fin'], w['has']
  zero = np.zeros(shape)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    noise = _F64 * (np.abs(np.where(fin, w['b'], 0.0)) + abs(w['G']) + np.abs(np.where(fin, np.log(w['h']), 0.0)))
  if exact or not fin.any():
    return noise, noise, w['n'] * 2.0 ** -53 + (noise[fin].max() if fin.any() else 0.0), 0.0
  m = _taps_T(taps)
  g = (m + 2) * U / (1 - (m + 2) * U)
  rho = 2 * g / (1 - g)
  with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
    share = np.where(has, w['A'] / w['prior'], 0.0)
    e_p = np.where(has, -np.log1p(-rho * share), 0.0)
    e_G = e_p.max()
    e_q = e_p + e_G + _F64 * (np.abs(np.where(has, w['nx'], 0.0)) + np.abs(np.where(has, np.log(w['prior']), 0.0))
                              + abs(w['G']))
    near = has & (np.abs(w['d'] - float(CUT)) <= e_q + 2.0 ** -18)
    dq = w['q'] * (np.expm1(e_q) * (1 + 2 * U) + 2 * U) + np.where(near, np.exp(float(CUT) + e_q + 2.0 ** -18), 0.0)
    g_u = m * U / (1 - m * U)
    du = adjoint(dq, taps)[2] * (1 + g_u) + g_u * w['u']
    dQ = dq.sum() + w['n'] * 2.0 ** -53 * w['Q']
    r_c = (g + 2 * U) / (1 - g) + _F64
    dh = w['carried'] * (du + r_c * (w['u'] + du)) + (w['eps'] / w['n']) * dQ + _F64 * w['h']
    rel = np.where(fin, dh / w['h'], 0.0)
    down_h = np.where(rel < 1, -np.log1p(-np.minimum(rel, 1 - 2.0 ** -52)), np.inf)
    down = np.where(fin, down_h + e_G + noise, 0.0)
    up = np.where(fin, np.log1p(rel) + e_G + noise, 0.0)
    pi = np.exp(np.where(fin, w['b'] + w['G'] + np.log(w['h']) - w['log_norm'], -np.inf))
    hi = math.log((pi * np.exp(up))[fin].sum())
    lo_sum = (pi * np.exp(-down))[fin].sum()
    lo = -math.log(lo_sum) if lo_sum > 0 else np.inf
  return down, up, max(hi, lo, 0.0) + w['n'] * 2.0 ** -53, e_G


def bounds(belief, nxt, taps, uniform_mix=0.0, exact=False):
  """-> (the derived bound of |fl32 result - reference| per cell (module docstring), 0 where the result is not
  finite; the bounds of the four statistics: log_norm (e_norm, the f32 rounding); S / sum p (the filter's: g for S,
  2 u for sum p, the quotient's rounding); G (e_G, float64 noise, the f32 rounding); the largest smoothed (the largest
  cell bound))."""
  out, stats, _, w = _walk(belief, nxt, taps, uniform_mix)
  fin = w['fin']
  down, up, e_norm, e_G = _errors(taps, w, exact)
  with np.errstate(invalid='ignore'):
    cell = np.where(fin, np.maximum(down, up) + e_norm + _F64 * abs(w['log_norm']) + U * np.abs(out), 0.0)
  m = _taps_T(taps) + 2
  g = 0.0 if exact else m * U / (1 - m * U)
  b_ln = e_norm + (_F64 + U) * abs(stats[0]) if np.isfinite(stats[0]) else 0.0
  b_kept = ((g + 2 * U) / (1 - 2 * U) + U) * abs(stats[1]) * 1.0001
  b_G = e_G + (_F64 + U) * abs(stats[2]) if np.isfinite(stats[2]) else 0.0
  return cell, np.array([b_ln, b_kept, b_G, cell[np.isfinite(cell)].max(initial=0.0)])


def bound(belief, nxt, taps, uniform_mix=0.0, exact=False):
  return bounds(belief, nxt, taps, uniform_mix, exact)[0]


def stats_bound(belief, nxt, taps, uniform_mix=0.0, exact=False):
  return bounds(belief, nxt, taps, uniform_mix, exact)[1]


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _case(name, belief, nxt, taps, uniform_mix=0.0):
  return dict(name=name, belief=belief, next=nxt, taps=taps, uniform_mix=uniform_mix)


def exact_case():
  """Every quantity below the final float64 expression is exact: the filter's ``exact_case`` belief and taps (masses
  in {0, 1}, power-of-two taps, integer shifts of both signs, the k wrap), eps = 0, and ``next`` = 0 on the cells of
  ONE value of t2 (the most frequent), -inf elsewhere: lg is one number, so lg - G = 0 and q is in {0, 1} whatever the
  last bit of log; u is a sum of power-of-two taps and Q a count.  The kernel's result is the reference's float64
  expression rounded once."""
  c = flt.exact_case()
  t2 = predict(masses(c['belief'])[0], c['taps'])
  vals, cnt = np.unique(t2[t2 > 0], return_counts=True)
  nxt = np.where(t2 == vals[cnt.argmax()], 0.0, -np.inf).astype(np.float32)
  return _case('exact', c['belief'], nxt, c['taps'], 0.0)


def all_inputs():
  """-> list of case dicts (name, belief, next, taps, uniform_mix); seeded: the same arrays in every process.  Belief,
  taps and eps are the filter's cases'; ``next`` is the reference filter's result one step further, rounded to f32."""
  src = {c['name']: c for c in flt.all_inputs()}
  rng = np.random.default_rng(20261020)
  cases = []
  for name in ('tiny', 'wrap', 'wrap_far', 'wrap_neg', 'ragged', 'mix0', 'mix1', 'bad', 'wide', 'tall', 'tk16', 'tiles',
               'empty_belief'):
    c = src[name]
    nxt = flt.vote_filter(c['belief'], c['votes'], c['taps'], c['scale'], c['uniform_mix'])[0].astype(np.float32)
    if name == 'bad':                                       # (the filter writes NaN for a +inf vote: put one +inf back)
      assert np.isnan(nxt[7, 15, 16]) and np.isnan(nxt[8, 15, 16])
      nxt[8, 15, 16] = np.inf
    cases.append(_case(name, c['belief'], nxt, c['taps'], c['uniform_mix']))
  by = {c['name']: c for c in cases}
  r = by['ragged']
  cases.append(_case('no_mass', r['belief'], np.full(r['belief'].shape, -np.inf, np.float32), r['taps'], 1e-3))
  # a `next` that does not come from the filter: ratios spread over more than the cut, some cells just around it
  nxt = r['next'].copy()
  lower = rng.random(nxt.shape) < 0.3
  nxt[lower] -= rng.uniform(25, 50, int(lower.sum())).astype(np.float32)
  cases.append(_case('cut', r['belief'], nxt, r['taps'], 1e-3))
  cases.append(exact_case())
  return cases


# ---------------------------------------------------------------------------------------------------------------
# the independent formulation: dense alpha-beta on a tiny lattice
# ---------------------------------------------------------------------------------------------------------------
def still_taps(R):
  """One tap of weight 1 at offset 0 on every axis: the tables of a filter step without a predict."""
  return (np.ones(1, np.float32), 0, np.ones((R, 1), np.float32), np.ones((R, 1), np.float32),
          np.zeros((R, 2), np.int32))


def tiny_track(seed=5):
  """-> (votes [3] f32 [3, 4, 5], taps [3] (entry 0 None), scale): n = 60 cells, three frames, xy shifts of both signs,
  the k wrap from both sides."""
  rng = np.random.default_rng(seed)
  R, Ho, Wo, N = 3, 4, 5, 3
  votes = [rng.standard_normal((R, Ho, Wo)).astype(np.float32) for _ in range(N)]
  taps = [None]
  for t in range(1, N):
    off = np.array([[-1, 1], [1, -2], [0, 1]], np.int32) * (1 if t == 1 else -1)
    taps.append((flt.rand_taps(rng, 1, 2)[0], -1 if t == 1 else 1, flt.rand_taps(rng, R, 2), flt.rand_taps(rng, R, 3),
                 off))
  return votes, taps, 2.0


def dense_kernel(belief, taps, eps):
  """K [n, n] (column = source cell), the kernel the filter applied to the normalised alpha behind ``belief``:
  (1 - eps) (sum p / S) T + eps / n, T by pushing unit masses through ``predict``, the factor from ``belief``."""
  shape, n = belief.shape, belief.size
  T = np.zeros((n, n))
  for x in range(n):
    e = np.zeros(n)
    e[x] = 1.0
    T[:, x] = predict(e.reshape(shape), taps).reshape(n)
  p = masses(belief)[0]
  return (1 - eps) * (p.sum() / predict(p, taps).sum()) * T + eps / n


def dense_smoothing(votes, taps, scale, eps, beliefs):
  """Textbook alpha-beta from the RAW votes with dense kernels (their factors sum p / S from the filtered ``beliefs``)
  -> list of gamma_t [n] (normalised, linear space).  Nothing of the ratio / adjoint / combine structure is in it."""
  N, n = len(votes), votes[0].size
  eps = float(np.float32(eps))
  K = [None] + [dense_kernel(beliefs[t - 1], taps[t], eps) for t in range(1, N)]
  ev = [np.exp(scale * v.astype(np.float64)).reshape(n) for v in votes]
  alpha = [ev[0] / ev[0].sum()]
  for t in range(1, N):
    a = ev[t] * (K[t] @ alpha[-1])
    alpha.append(a / a.sum())
  beta = [None] * N
  beta[-1] = np.ones(n)
  for t in range(N - 2, -1, -1):
    beta[t] = K[t + 1].T @ (ev[t + 1] * beta[t + 1])
  gamma = [alpha[t] * beta[t] for t in range(N)]
  return [g / g.sum() for g in gamma]
