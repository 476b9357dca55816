"""A float64 numpy restatement of ``snap_vote_sample_f32`` and ``snap_vote_sample_back_f32`` (include/snap_hip.h),
written from the contract, not from the kernels: DENSE cumulative sums in lattice order, no hierarchy.

The contract, restated
----------------------
* Philox4x32-10 on (counter, key); draw i of a call takes the counter (i, stream, purpose, 0) and the key (seed low
  word, seed high word); u0 = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53, u1 likewise from x2, x3.  purpose 0: ``vote_sample``,
  1: ``vote_sample_back``.
* The mass of a cell: s = fl32(scale * v), M = the largest finite s, d = fl32(s - M), p = fl32(exp(float64(d))) iff s is
  finite and d >= -40, else 0 (``vote_filter_reference.masses`` on s: the f32 decisions exactly).
* A draw: the first cell, linear index ascending, whose inclusive prefix of p exceeds u * Z, Z = sum p; -1 without mass.
  log_prob = (s - M) - log Z.
* The backward step of a chain at x = (r, a, b): window entry (tk, ta, tb), ascending lexicographic, has the cell
  ((r + lk + tk) mod R, a + la[r] + ta, b + lb[r] + tb) and the weight taps_k[tk] taps_a[r, ta] taps_b[r, tb] p[cell]
  (0 outside the volume); W = their sum; A = (1 - eps) W / S, S = sum t2 of the filter's predict step (0 when S == 0);
  J = eps / n (0 when sum p == 0).  u0 (A + J) < J: the jump, a draw as above from p with u1; else the cell of the
  first entry whose inclusive prefix exceeds u1 W.  -1 / -1 where the chain's cell is outside [0, n) or A + J == 0.

The kernels evaluate the same CDFs through plane, row and cell sums in another order of float64 additions, and their
masses may differ from numpy's in the last f32 bit (two float64 exp's rounded to f32).  ``TOL`` = 2^-22 of the total
covers both: 2^-23 relative on every mass, hence on every prefix, and n 2^-53 <= 2^-33 for n <= 5.5e5 terms.
"""
import math

import numpy as np

import vote_filter_reference as flt
from vote_filter_reference import masses, predict

TOL = 2.0 ** -22
MAX_DRAWS = 1 << 20


# ---------------------------------------------------------------------------------------------------------------
# Philox4x32-10 and the uniforms
# ---------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
  """counter uint32 [..., 4], key uint32 [..., 2] (broadcast) -> uint32 [..., 4]."""
  c = np.asarray(counter, np.uint64) & np.uint64(0xFFFFFFFF)
  k = np.asarray(key, np.uint64) & np.uint64(0xFFFFFFFF)
  c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
  k0, k1 = np.broadcast_to(k[..., 0], c0.shape).copy(), np.broadcast_to(k[..., 1], c0.shape).copy()
  M0, M1, W0, W1, mask = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
  for _ in range(10):
    p0, p1 = M0 * c0, M1 * c2                                 # 32 x 32 -> 64 bits: exact in uint64
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
    k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
  return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def uniforms(num, seed, stream, purpose):
  """-> float64 [num, 2] in [0, 1): (u0, u1) of draws 0 .. num - 1."""
  counter = np.zeros((num, 4), np.uint64)
  counter[:, 0] = np.arange(num)
  counter[:, 1] = np.uint64(int(stream) & 0xFFFFFFFF)
  counter[:, 2] = purpose
  seed = int(seed)
  x = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)).astype(np.float64)
  hi = np.floor(x[:, 0::2] / 32.0)                            # x >> 5
  lo = np.floor(x[:, 1::2] / 64.0)                            # x >> 6
  return (hi * 2.0 ** 26 + lo) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------
# entry point (a)
# ---------------------------------------------------------------------------------------------------------------
def scaled(votes, scale):
  votes = np.asarray(votes)
  assert votes.dtype == np.float32 and votes.ndim == 3
  with np.errstate(invalid='ignore', over='ignore'):
    return (np.float32(scale) * votes).astype(np.float32)    # one f32 product


def model(votes, scale=1.0):
  """-> dict: s (scaled votes), p [n] float64, cdf [n] (inclusive, lattice order), Z, M, bad, mass."""
  s = scaled(votes, scale)
  p, M, bad, mass = masses(s)
  p = p.reshape(-1)
  cdf = np.cumsum(p)
  return dict(s=s.reshape(-1), p=p, cdf=cdf, Z=float(cdf[-1]), M=M, bad=bad, mass=mass)


def draw(m, u):
  """The dense inverse CDF: u float64 [B] -> linear index int64 [B] (-1 without mass)."""
  u = np.asarray(u, np.float64)
  if not m['Z'] > 0:
    return np.full(u.shape, -1, np.int64)
  idx = np.searchsorted(m['cdf'], u * m['Z'], side='right')
  last = int(np.nonzero(m['p'] > 0)[0][-1])
  return np.minimum(idx, last).astype(np.int64)


def vote_sample(votes, num, seed, stream=0, scale=1.0, uni=None):
  """-> (index int64 [num], log_prob float64 [num], stats float64 [2], count int64 [2])."""
  m = model(votes, scale)
  uni = uniforms(num, seed, stream, 0) if uni is None else np.asarray(uni, np.float64)
  idx = draw(m, uni[:, 0])
  lp = np.full(num, -np.inf)
  if m['Z'] > 0:
    lp = (m['s'][idx].astype(np.float64) - float(m['M'])) - math.log(m['Z'])
  with np.errstate(divide='ignore'):
    stats = np.array([float(m['M']) + np.log(m['Z']) if m['Z'] > 0 else -np.inf, float(m['M'])])
  return idx, lp, stats, np.array([m['mass'], m['bad']], np.int64)


def member(m, idx, u, tol=TOL):
  """Whether cell idx [B] is an admissible answer for u [B]: it has mass and u Z lies in its interval of the dense
  CDF widened by tol Z on both sides -> bool [B]."""
  idx = np.asarray(idx, np.int64)
  ok = (idx >= 0) & (idx < m['p'].size)
  i = np.clip(idx, 0, m['p'].size - 1)
  lo = np.where(i > 0, m['cdf'][np.maximum(i - 1, 0)], 0.0)
  t, slack = np.asarray(u) * m['Z'], tol * m['Z']
  return ok & (m['p'][i] > 0) & (lo - slack <= t) & (t <= m['cdf'][i] + slack)


# ---------------------------------------------------------------------------------------------------------------
# entry point (b)
# ---------------------------------------------------------------------------------------------------------------
def back_model(belief, taps, eps):
  """What every chain of one backward step shares."""
  belief = np.asarray(belief)
  m = model(belief, 1.0)
  p3 = m['p'].reshape(belief.shape)
  S = float(predict(p3, taps).sum())
  sum_p = float(m['p'].sum())
  taps_k, lk, taps_a, taps_b, offsets = taps
  m.update(shape=belief.shape, n=belief.size, S=S, sum_p=sum_p, eps=float(np.float32(eps)), lk=int(lk),
           taps_k=np.asarray(taps_k, np.float32).astype(np.float64),
           taps_a=np.asarray(taps_a, np.float32).astype(np.float64),
           taps_b=np.asarray(taps_b, np.float32).astype(np.float64), offsets=np.asarray(offsets, np.int64),
           kept=S / sum_p if sum_p > 0 else 0.0)
  return m


def window(bm, x):
  """The chain at linear index x -> (weights float64 [Tk Ta Tb], cells int64 [Tk Ta Tb] (-1 outside), W, A, J)."""
  R, Ho, Wo = bm['shape']
  r, a, b = np.unravel_index(int(x), bm['shape'])
  Tk, Ta, Tb = len(bm['taps_k']), bm['taps_a'].shape[1], bm['taps_b'].shape[1]
  tk, ta, tb = np.meshgrid(np.arange(Tk), np.arange(Ta), np.arange(Tb), indexing='ij')
  k = (r + bm['lk'] + tk) % R
  sa = a + bm['offsets'][r, 0] + ta
  sb = b + bm['offsets'][r, 1] + tb
  inside = (sa >= 0) & (sa < Ho) & (sb >= 0) & (sb < Wo)
  cells = np.where(inside, (k * Ho + np.clip(sa, 0, Ho - 1)) * Wo + np.clip(sb, 0, Wo - 1), -1).reshape(-1)
  w = (bm['taps_k'][tk] * bm['taps_a'][r][ta] * bm['taps_b'][r][tb]).reshape(-1)
  w = np.where(cells >= 0, w * bm['p'][np.maximum(cells, 0)], 0.0)
  W = float(np.cumsum(w)[-1])
  A = (1.0 - bm['eps']) * W / bm['S'] if bm['S'] > 0 else 0.0
  J = bm['eps'] / bm['n'] if bm['sum_p'] > 0 else 0.0
  return w, cells, W, A, J


def conditional(bm, x):
  """q(x' | x) over all n predecessors, float64 [n] summing to 1 (zeros when nothing can precede x)."""
  w, cells, W, A, J = window(bm, x)
  q = np.zeros(bm['n'])
  if not A + J > 0:
    return q
  if A > 0:
    np.add.at(q, cells[cells >= 0], (A / W) * w[cells >= 0])
  if J > 0:
    q += J * bm['p'] / bm['Z']
  return q / (A + J)


def back_one(bm, x, u0, u1):
  """-> (prev, jumped) of one chain."""
  if not 0 <= x < bm['n']:
    return -1, -1
  seen = bm.setdefault('_windows', {})                       # (chains that share a cell share its window)
  if x not in seen:
    w, cells, W, A, J = window(bm, x)
    seen[x] = (w, cells, W, A, J, np.cumsum(w), int(np.nonzero(w > 0)[0][-1]) if W > 0 else -1)
  w, cells, W, A, J, cdf, last = seen[x]
  if not A + J > 0:
    return -1, -1
  if u0 * (A + J) < J:
    return int(draw(bm, np.array([u1]))[0]), 1
  e = min(int(np.searchsorted(cdf, u1 * W, side='right')), last)
  return int(cells[e]), 0


def vote_sample_back(belief, nxt, taps, eps, seed, stream=0, uni=None):
  """-> (prev int64 [B], jumped int64 [B], stats float64 [2], count int64 [3])."""
  bm = back_model(belief, taps, eps)
  nxt = np.asarray(nxt, np.int64)
  uni = uniforms(len(nxt), seed, stream, 1) if uni is None else np.asarray(uni, np.float64)
  out = np.array([back_one(bm, int(x), u[0], u[1]) for x, u in zip(nxt, uni)], np.int64).reshape(-1, 2)
  stats = np.array([bm['kept'], float(bm['M'])])
  count = np.array([(out[:, 0] >= 0).sum(), (out[:, 1] == 1).sum(), bm['bad']], np.int64)
  return out[:, 0], out[:, 1], stats, count


def back_admissible(bm, x, u0, u1, prev, jumped, tol=TOL):
  """Whether (prev, jumped) is an admissible answer of the chain at x for (u0, u1) -> (bool, why)."""
  if not 0 <= x < bm['n']:
    return (prev, jumped) == (-1, -1), 'an ended chain'
  w, cells, W, A, J = window(bm, x)
  if not A + J > 0:
    return (prev, jumped) == (-1, -1), 'nothing precedes the cell'
  side = u0 * (A + J) - J
  want = 1 if side < 0 else 0
  if jumped != want and abs(side) > tol * (A + J):
    return False, f'branch {jumped}, want {want}: u0 (A + J) - J = {side}, A + J = {A + J}'
  if jumped == 1:
    return bool(member(bm, np.array([prev]), np.array([u1]), tol)[0]), 'the jump\'s cell'
  if jumped != 0:
    return False, f'jumped = {jumped}'
  cdf = np.cumsum(w)
  lo = np.concatenate([[0.0], cdf[:-1]])
  t, slack = u1 * W, tol * W
  ok = (cells == prev) & (w > 0) & (lo - slack <= t) & (t <= cdf + slack)
  return bool(ok.any()), 'the window entry'


def sample_tracks(beliefs, taps_list, eps, num, seed):
  """Forward-filter / backward-sample on f32 beliefs [N], taps_list[t] the filter's taps INTO frame t (entry 0
  unused) -> (linear int64 [N, num], jumps bool [N, num])."""
  N = len(beliefs)
  cur = vote_sample(beliefs[-1], num, seed, N - 1)[0]
  linear, jumps = [cur], []
  for t in range(N - 2, -1, -1):
    cur, jumped = vote_sample_back(beliefs[t], cur, taps_list[t + 1], eps, seed, t)[:2]
    linear.append(cur)
    jumps.append(jumped == 1)
  jumps.append(np.zeros(num, bool))
  return np.stack(linear[::-1]), np.stack(jumps[::-1])


def max_abs_z(linear, prob, min_expected=20.0):
  """The largest |count - B pi| / sqrt(B pi (1 - pi)) over the cells with B pi >= min_expected -> (z, cells used)."""
  B = linear.size
  prob = np.asarray(prob, np.float64).reshape(-1)
  counts = np.bincount(linear[linear >= 0], minlength=prob.size).astype(np.float64)
  use = B * prob >= min_expected
  z = (counts[use] - B * prob[use]) / np.sqrt(B * prob[use] * (1 - prob[use]))
  return float(np.abs(z).max()), int(use.sum())


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def given_uniforms(m, rng, strata=256):
  """The uniforms of the membership tests for one volume: 0, 1 - 2^-53, exact CDF boundaries, ``strata`` stratified
  values -> float64 [B] (the same value serves as u0 and u1)."""
  u = [0.0, 1.0 - 2.0 ** -53]
  if m['Z'] > 0:
    has = np.nonzero(m['p'] > 0)[0]
    pick = has[rng.integers(0, len(has), min(16, len(has)))]
    u += [min(float(m['cdf'][c] / m['Z']), 1.0 - 2.0 ** -53) for c in pick]
  u += ((np.arange(strata) + rng.random(strata)) / strata).tolist()
  return np.array(u, np.float64)


def sample_inputs():
  """-> list of dicts (name, votes, scale) for ``vote_sample``: the volumes of the filter tests' cases."""
  f = {c['name']: c for c in flt.all_inputs()}
  rng = np.random.default_rng(20261020)
  cases = [dict(name='tiny', votes=f['tiny']['belief'], scale=1.0),
           dict(name='small', votes=f['wrap']['belief'], scale=1.0)]
  ragged = f['bad']['belief'].copy()                        # [36, 31, 33]: 30 % -inf, one NaN, one +inf
  ragged[rng.integers(0, 36, 5), rng.integers(0, 31, 5), rng.integers(0, 33, 5)] = np.nan
  cases.append(dict(name='ragged', votes=ragged, scale=1.0))
  cases.append(dict(name='wide', votes=f['wide']['belief'], scale=1.0))
  cases.append(dict(name='tall', votes=f['tall']['belief'], scale=1.0))
  cases.append(dict(name='tiles', votes=f['tiles']['belief'], scale=1.0))
  one = np.full((3, 5, 70), -np.inf, np.float32)
  one[1, 3, 66] = -2.5
  cases.append(dict(name='one_cell', votes=one, scale=1.0))
  cases.append(dict(name='no_mass', votes=np.full((3, 5, 6), -np.inf, np.float32), scale=1.0))
  cases.append(dict(name='scaled', votes=f['ragged']['belief'], scale=0.25))
  return cases


def back_inputs():
  """-> list of dicts (name, belief, taps, eps) for ``vote_sample_back``: the filter tests' own cases."""
  f = {c['name']: c for c in flt.all_inputs()}
  names = dict(wrap='wrap', wrap_far='wrap_far', wrap_neg='wrap_neg', tk16='tk16', ragged='ragged', wide='wide',
               never_jumps='mix0', always_jumps='mix1')
  cases = [dict(name=k, belief=f[v]['belief'], taps=f[v]['taps'], eps=f[v]['uniform_mix']) for k, v in names.items()]
  cases[3]['eps'] = 0.05                                    # (the filter's tk16 has eps = 0)
  return cases


def all_inputs():
  return dict(sample=sample_inputs(), back=back_inputs())


def back_chains(bm, rng, num=24):
  """Chain cells for a backward case: random cells, the corners, and the two ends outside [0, n)."""
  n = bm['n']
  return np.concatenate([[0, n - 1, -1, n], rng.integers(0, n, num)]).astype(np.int64)


def stat_scene():
  """The track of the seeded statistical test: [4, 5, 6], three frames, eps = 1e-2, non-trivial increments; the tap
  tables are the host's own (``motion_taps``, built on the CPU: imported here, nothing else in this module needs the
  package) -> dict(votes [3] f32, incs, taps [3] numpy tuples (entry 0 None), grid, kw, R)."""
  import torch
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import geometry, grids
  rng = np.random.default_rng(77)
  R, Ho, Wo = 4, 5, 6
  grid = grids.Grid2D((3, 3), 0.5)
  kw = dict(sigma_xy=0.3, sigma_yaw=0.5, temperature=1.5, uniform_mix=1e-2)
  votes = [rng.standard_normal((R, Ho, Wo)).astype(np.float32) for _ in range(3)]
  t = lambda a, x, y: geometry.Transform2D(torch.tensor(a, dtype=torch.float64), torch.tensor([x, y], dtype=torch.float64))
  incs = [None, t(0.4, 0.3, -0.2), t(-0.7, -0.35, 0.4)]
  taps = [None]
  for inc in incs[1:]:
    tp = pev.motion_taps(inc, grid, R, kw['sigma_xy'], kw['sigma_yaw'], device='cpu')
    taps.append(tuple(v.numpy() if isinstance(v, torch.Tensor) else v for v in tp))
  return dict(votes=votes, incs=incs, taps=taps, grid=grid, kw=kw, R=R)


def stat_reference(scene, num, seed):
  """The reference filter, smoother and sampler on the scene -> (max |z| of frame 0 against the smoothed marginal, of
  the last frame against the belief, cells used in each)."""
  import vote_smooth_reference as smo
  kw = scene['kw']
  beliefs = [flt.vote_filter(None, scene['votes'][0], smo.still_taps(scene['R']), kw['temperature'],
                             kw['uniform_mix'])[0].astype(np.float32)]
  for v, tp in zip(scene['votes'][1:], scene['taps'][1:]):
    beliefs.append(flt.vote_filter(beliefs[-1], v, tp, kw['temperature'], kw['uniform_mix'])[0].astype(np.float32))
  gamma = smo.smooth_track(beliefs, scene['taps'], kw['uniform_mix'])
  linear, _ = sample_tracks(beliefs, scene['taps'], kw['uniform_mix'], num, seed)
  z0, n0 = max_abs_z(linear[0], np.exp(gamma[0].astype(np.float64)))
  z2, n2 = max_abs_z(linear[-1], np.exp(beliefs[-1].astype(np.float64)))
  return z0, z2, n0, n2
