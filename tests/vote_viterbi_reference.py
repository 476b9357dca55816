"""numpy float32 restatement of ``snap_vote_viterbi_f32`` / ``snap_vote_backstep_i32``, written from the contract in
include/snap_hip.h (not from the kernel), and the inputs of the tests.

Every operation of the contract is one IEEE f32 addition, subtraction, product or comparison, so this file computes the
SAME BITS as the kernel, not an approximation of them: every array below is ``np.float32`` and every scalar that meets
one is an ``np.float32`` (numpy then rounds each elementwise operation to f32 once, as the contract asks; nothing is
contracted into an fma).  The GPU test compares bit for bit, with no tolerance.

  M = the largest finite score_prev, J = its lowest linear index (-1 without one); d = score_prev - M (-inf where the
  cell is not finite); three max-plus passes with the taps ascending and replacement on strict > (the lowest tap index
  among equals); stay = log_stay + m2, jump = log_jump if J >= 0; best = stay if stay >= jump else jump; score_out =
  fl32(scale * votes) + best; back = the composed predecessor, J for a jump, -1 where score_out is -inf.

``brute_force`` is the independent check of the passes; ``path_value`` that of ``back``; ``track`` / ``trace`` chain
the steps as ``pose_exhaustive_voting.viterbi_track`` does.
"""
import math

import numpy as np

import vote_filter_reference as flt

F = np.float32
NEG = F(-np.inf)
TILE = 256
MAX_GROUPS = 2048


def log_taps(taps):
  """A filter tap tuple -> its log-tap tuple: float32(log(float64(w))), -inf for w = 0; lk and the offsets unchanged."""
  tk, lk, ta, tb, off = taps
  with np.errstate(divide='ignore'):
    lg = lambda w: np.log(np.asarray(w, np.float32).astype(np.float64)).astype(np.float32)
    return lg(tk), int(lk), lg(ta), lg(tb), np.asarray(off, np.int32)


def log_weights(eps, n):
  """(log_stay, log_jump) as ``pose_exhaustive_voting.viterbi_votes`` forms them -> two np.float32."""
  with np.errstate(divide='ignore'):
    return F(np.log1p(-np.float64(eps))), F(np.log(np.float64(eps)) - math.log(n))


def peak(prev):
  """-> (M f32, J int, bad int): the largest finite value, its lowest linear index (-1), the NaN / +inf cells."""
  flat = prev.reshape(-1)
  fin = np.isfinite(flat)
  bad = int((~fin & ~(flat == NEG)).sum())
  if not fin.any():
    return NEG, -1, bad
  M = flat[fin].max()
  return F(M), int(np.flatnonzero(fin & (flat == M))[0]), bad


def _unpack(ltaps):
  ltk, lk, lta, ltb, off = ltaps
  ltk, lta, ltb = (np.asarray(t) for t in (ltk, lta, ltb))
  assert ltk.dtype == np.float32 and lta.dtype == np.float32 and ltb.dtype == np.float32
  return ltk, int(lk), lta, ltb, np.asarray(off, np.int64)


def relative(prev, M):
  """d = score_prev - M as f32, -inf where score_prev is not finite."""
  with np.errstate(invalid='ignore'):
    return np.where(np.isfinite(prev), prev - F(M), NEG).astype(np.float32)


def _keep(best, arg, c, t):
  upd = c > best
  best[...] = np.where(upd, c, best)
  arg[...] = np.where(upd, t, arg)


def passes(d, ltaps):
  """The three max-plus passes -> (m0, ck, m1, ca, m2, cb): f32 volumes and the chosen tap indices (0 where nothing
  was above -inf)."""
  ltk, lk, lta, ltb, off = _unpack(ltaps)
  R, Ho, Wo = d.shape
  m0, ck = np.full(d.shape, NEG), np.zeros(d.shape, np.int64)
  for tk in range(len(ltk)):
    _keep(m0, ck, ltk[tk] + d[(np.arange(R) + lk + tk) % R], tk)
  m1, ca = np.full(d.shape, NEG), np.zeros(d.shape, np.int64)
  m2, cb = np.full(d.shape, NEG), np.zeros(d.shape, np.int64)
  for r in range(R):
    la = int(off[r, 0])
    for ta in range(lta.shape[1]):
      s = la + ta
      lo, hi = max(0, -s), min(Ho, Ho - s)                  # output rows whose source row a + s is inside
      if lo < hi:
        _keep(m1[r, lo:hi], ca[r, lo:hi], lta[r, ta] + m0[r, lo + s:hi + s], ta)
  for r in range(R):
    lb = int(off[r, 1])
    for tb in range(ltb.shape[1]):
      s = lb + tb
      lo, hi = max(0, -s), min(Wo, Wo - s)
      if lo < hi:
        _keep(m2[r, :, lo:hi], cb[r, :, lo:hi], ltb[r, tb] + m1[r, :, lo + s:hi + s], tb)
  return m0, ck, m1, ca, m2, cb


def walk(score_prev, votes, ltaps, scale, log_stay, log_jump):
  """Everything of one step -> dict: score, back, stats f32 [2], count int64 [6], and the inner quantities M, J, d, m2,
  jumped (bool volume: the cell was entered by the jump), sv = fl32(scale * votes)."""
  votes = np.asarray(votes)
  assert votes.dtype == np.float32 and votes.ndim == 3
  R, Ho, Wo = votes.shape
  scale, log_stay, log_jump = F(scale), F(log_stay), F(log_jump)
  assert np.isfinite(scale) and scale > 0 and log_stay <= 0 and log_jump <= 0
  idx = np.arange(votes.size, dtype=np.int64).reshape(votes.shape)
  if score_prev is None:
    M, J, bad = NEG, -1, 0
    d = m2 = None
    best = np.zeros(votes.shape, np.float32)
    pred = np.full(votes.shape, -1, np.int64)
    jumped = np.zeros(votes.shape, bool)
  else:
    score_prev = np.asarray(score_prev)
    assert score_prev.dtype == np.float32 and score_prev.shape == votes.shape
    M, J, bad = peak(score_prev)
    d = relative(score_prev, M)
    ltk, lk, lta, ltb, off = _unpack(ltaps)
    m0, ck, m1, ca, m2, cb = passes(d, ltaps)
    stay = log_stay + m2
    jump = log_jump if J >= 0 else NEG
    jumped = ~(stay >= jump)
    best = np.where(jumped, jump, stay).astype(np.float32)
    # the composed predecessor: the column tap at (r, a, b) gives b', the row tap at (r, a, b') a', the rotation tap at
    # (r, a', b') k'
    r, a, b = np.unravel_index(idx, votes.shape)
    has = m2 > NEG
    bs = np.where(has, b + off[r, 1] + cb, 0)
    as_ = np.where(has, a + off[r, 0] + ca[r, a, bs], 0)
    ks = (r + lk + ck[r, as_, bs]) % R
    pred = np.where(jumped, J, np.where(has, (ks * Ho + as_) * Wo + bs, -1))
  with np.errstate(invalid='ignore', over='ignore'):
    sv = (scale * votes).astype(np.float32)
    bad_vote = ~(votes < F(np.inf))
    dead = bad_vote | (votes == NEG) | (best == NEG)
    score = np.where(dead, NEG, sv + best).astype(np.float32)
  out_dead = score == NEG
  back = np.where(out_dead, -1, pred).astype(np.int32)
  jumped = jumped & ~out_dead
  flat = score.reshape(-1)
  top = flat.max()
  top_at = int(np.flatnonzero(flat == top)[0]) if top > NEG else -1
  stats = np.array([M, top], np.float32)
  count = np.array([np.isfinite(score).sum(), bad, bad_vote.sum(), jumped.sum(), J, top_at], np.int64)
  return dict(score=score, back=back, stats=stats, count=count, M=M, J=J, d=d, m2=m2, jumped=jumped, sv=sv)


def vote_viterbi(score_prev, votes, ltaps, scale=1.0, log_stay=0.0, log_jump=-np.inf):
  """-> (score_out f32 [R, Ho, Wo], back int32 [R, Ho, Wo], stats f32 [2], count int64 [6])."""
  w = walk(score_prev, votes, ltaps, scale, log_stay, log_jump)
  return w['score'], w['back'], w['stats'], w['count']


def vote_backstep(back, cur):
  """prev[i] = back.flat[cur[i]] if 0 <= cur[i] < n else -1 -> int32 [B]."""
  flat, cur = np.asarray(back).reshape(-1), np.asarray(cur, np.int64)
  ok = (cur >= 0) & (cur < flat.size)
  return np.where(ok, flat[np.where(ok, cur, 0)], -1).astype(np.int32)


def _shifted(plane, sa, sb):
  """out[a, b] = plane[a + sa, b + sb], -inf outside."""
  Ho, Wo = plane.shape
  out = np.full(plane.shape, NEG)
  a0, a1, b0, b1 = max(0, -sa), min(Ho, Ho - sa), max(0, -sb), min(Wo, Wo - sb)
  if a0 < a1 and b0 < b1:
    out[a0:a1, b0:b1] = plane[a0 + sa:a1 + sa, b0 + sb:b1 + sb]
  return out


def brute_force(d, ltaps):
  """m2 by enumeration: per cell the maximum over ALL (tk, ta, tb) of fl32(ltb + fl32(lta + fl32(ltk + d[source]))),
  the source (k', a', b') = ((r + lk + tk) mod R, a + la[r] + ta, b + lb[r] + tb), -inf outside -> f32 [R, Ho, Wo].

  Why the separable passes must equal this joint maximum EXACTLY, not just within rounding: f32 addition of a fixed
  number is monotone non-decreasing (x <= y implies fl(c + x) <= fl(c + y): rounding to nearest is monotone), so
  fl(c + max_i x_i) = max_i fl(c + x_i).  Applied twice, max_tb fl(ltb + max_ta fl(lta + max_tk fl(ltk + d))) =
  max over the triples of the nested expression above.  Only the VALUE is compared: which of several equal triples the
  passes report is fixed by their tie rule, not by this enumeration."""
  ltk, lk, lta, ltb, off = _unpack(ltaps)
  R, Ho, Wo = d.shape
  out = np.full(d.shape, NEG)
  for r in range(R):
    la, lb = int(off[r, 0]), int(off[r, 1])
    for tk in range(len(ltk)):
      inner = ltk[tk] + d[(r + lk + tk) % R]
      for ta in range(lta.shape[1]):
        mid = lta[r, ta] + inner
        for tb in range(ltb.shape[1]):
          out[r] = np.maximum(out[r], ltb[r, tb] + _shifted(mid, la + ta, lb + tb))
  return out


def path_value(d, ltaps, cur, prev):
  """The transported value of the step from the cell ``prev`` (linear index at the previous frame) into ``cur``: the
  largest fl32(ltb + fl32(lta + fl32(ltk + d[prev]))) over the tap triples of ``cur``'s rotation that lead to ``prev``;
  -inf when none does.  Scalars."""
  ltk, lk, lta, ltb, off = _unpack(ltaps)
  R, Ho, Wo = d.shape
  r, a, b = np.unravel_index(int(cur), d.shape)
  k2, a2, b2 = np.unravel_index(int(prev), d.shape)
  ta, tb = a2 - a - int(off[r, 0]), b2 - b - int(off[r, 1])
  best = NEG
  if 0 <= ta < lta.shape[1] and 0 <= tb < ltb.shape[1]:
    for tk in range(len(ltk)):
      if (r + lk + tk) % R == k2:
        best = max(best, F(ltb[r, tb] + F(lta[r, ta] + F(ltk[tk] + d[k2, a2, b2]))))
  return F(best)


def track(volumes, ltaps_list, scale, eps):
  """The forward steps over N volumes (``ltaps_list[t]`` = the log-taps INTO frame t, entry 0 unused) -> list of
  ``walk`` dicts; log_stay / log_jump from ``log_weights(eps, n)``."""
  log_stay, log_jump = log_weights(eps, volumes[0].size)
  steps, score = [], None
  for t, v in enumerate(volumes):
    steps.append(walk(score, v, None if t == 0 else ltaps_list[t], scale, log_stay, log_jump))
    score = steps[-1]['score']
  return steps


def trace(steps, end=None):
  """The back-pointers from ``end`` (default: the last step's count[5]) -> (linear int64 [N], jumps bool [N],
  log_score float64 = the end cell's score + the sum of M over t >= 1)."""
  cur = int(steps[-1]['count'][5]) if end is None else int(end)
  n = steps[-1]['score'].size
  total = float(steps[-1]['score'].reshape(-1)[cur]) if 0 <= cur < n else -np.inf
  linear, jumps = [cur], []
  for s in reversed(steps[1:]):
    jumps.append(bool(s['jumped'].reshape(-1)[cur]) if 0 <= cur < n else False)
    cur = int(vote_backstep(s['back'], [cur])[0])
    total += float(s['M'])
    linear.append(cur)
  jumps.append(False)
  return np.array(linear[::-1], np.int64), np.array(jumps[::-1], bool), total


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _case(name, score_prev, votes, ltaps, scale=1.0, eps=1e-3, log_stay=None, log_jump=None):
  ls, lj = log_weights(eps, votes.size)
  return dict(name=name, score_prev=score_prev, votes=votes, ltaps=ltaps, scale=scale,
              log_stay=float(ls if log_stay is None else log_stay), log_jump=float(lj if log_jump is None else log_jump))


def all_inputs():
  """-> list of case dicts (name, score_prev, votes, ltaps, scale, log_stay, log_jump); seeded: the same arrays in
  every process.  Shapes and tap tables are those of ``vote_filter_reference.all_inputs``' cases of the same names,
  the taps replaced by their logarithms.  Votes are standard normals (times 0.25 where scale = 8): scale * vote is a
  normal f32 number or zero."""
  src = {c['name']: c for c in flt.all_inputs()}
  rng = np.random.default_rng(20261021)
  cases = []

  def from_filter(name, as_name=None, **kw):
    c = src[name]
    cases.append(_case(as_name or name, c['belief'], c['votes'], log_taps(c['taps']), c['scale'], **kw))

  for name in ('tiny', 'wrap', 'wrap_far', 'wrap_neg', 'tk16', 'ragged', 'wide', 'tall', 'tiles', 'bad'):
    from_filter(name)
  cases.append(_case('first', None, src['ragged']['votes'], log_taps(src['ragged']['taps']), 8.0))
  from_filter('wrap', 'stay_off', log_stay=-np.inf)
  from_filter('empty_belief', 'empty')
  # a constant volume with equal log-taps: the lowest tap index per pass (back[x] = x with offsets 0), the lowest
  # linear index for J and for count[5], and stay == jump exactly (-0.5 + (-1 - 1 - 1) = -3.5): stay wins
  shape = (3, 5, 6)
  R = shape[0]
  eq = (np.full(3, -1, np.float32), 0, np.full((R, 4), -1, np.float32), np.full((R, 2), -1, np.float32),
        np.zeros((R, 2), np.int32))
  cases.append(_case('ties', np.zeros(shape, np.float32), np.ones(shape, np.float32), eq, 1.0, log_stay=-0.5,
                     log_jump=-3.5))
  # every transported source outside the volume: every row source is below it
  shape = (4, 7, 7)
  w = src['wrap']
  tk, lk, ta, tb, off = log_taps(w['taps'])
  out_off = off.copy()
  out_off[:, 0] = shape[1]
  cases.append(_case('jump_only', w['belief'], w['votes'], (tk, lk, ta, tb, out_off), 1.0, eps=0.25))
  cases.append(_case('no_jump_outside', w['belief'], w['votes'], (tk, lk, ta, tb, out_off), 1.0, eps=0.0))
  return cases


def tiny_track(seed=9, shape=(2, 2, 3), frames=3):
  """-> (votes [frames] f32 ``shape``, ltaps [frames] (entry 0 None)): a lattice small enough to enumerate every path,
  shifts of both signs, the k wrap, one -inf log-tap."""
  rng = np.random.default_rng(seed)
  R = shape[0]
  votes = [rng.standard_normal(shape).astype(np.float32) for _ in range(frames)]
  ltaps = [None]
  for t in range(1, frames):
    taps = (flt.rand_taps(rng, 1, 2)[0], int(rng.integers(-2, 3)), flt.rand_taps(rng, R, 2),
            flt.rand_taps(rng, R, 3, zeros=0.3), rng.integers(-1, 1, (R, 2)).astype(np.int32))
    ltaps.append(log_taps(taps))
  return votes, ltaps


def path_score(path, votes, ltaps_list, steps, scale, eps):
  """The score of ONE pose sequence ``path`` (linear indices, one per frame) with the contract's f32 expressions:
  s_0 = fl32(scale * v_0) + 0; s_t = fl32(scale * v_t) + max(log_stay + transported value of s_{t-1} - M_t, log_jump if
  the predecessor is J_t), -inf when neither applies.  M_t and J_t are the forward recursion's (``steps``): they are
  properties of the frame, not of the path.  f32 addition is monotone, so the maximum of this over all paths that end
  in a cell is the recursion's score of that cell."""
  log_stay, log_jump = log_weights(eps, votes[0].size)
  s = F(F(scale) * votes[0].reshape(-1)[path[0]]) + F(0)
  for t in range(1, len(path)):
    M, J = steps[t]['M'], steps[t]['J']
    d = np.full(votes[0].shape, NEG)
    if np.isfinite(s):
      d.reshape(-1)[path[t - 1]] = F(s - M)
    stay = F(log_stay + path_value(d, ltaps_list[t], path[t], path[t - 1]))
    jump = log_jump if path[t - 1] == J else NEG
    best = max(stay, jump)
    v = votes[t].reshape(-1)[path[t]]
    s = F(F(F(scale) * v) + best) if best > NEG and v > NEG else NEG
  return F(s)
