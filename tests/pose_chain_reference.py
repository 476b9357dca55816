"""Inputs and float64 references of the RANSAC pose chain tests (TEST INFRASTRUCTURE).

Shared by ``test_pose_chain_reference.py`` (CPU: every input below satisfies its stated condition on
the reference alone) and ``test_gpu_pose_chain.py`` (the HIP kernels of ``pose.hip`` against these
references).  Everything here is numpy float64 written from ``oracle/`` and from the semantics the
kernels document; the constants of the launchers are restated because the library has no query for
them -- a dispatch change then fails the assertions instead of silently emptying a case.
"""
import itertools

import numpy as np


EPS = 2.0 ** -23           # spacing of f32 at 1: twice the rounding unit
MARGIN = 8.0               # over a first-order bound, for the order of operations (as the attention tests)
CELL = 0.25                # dyadic cell size of the planted cases

# ----------------------------------------------------------------------------------------------
# A. argmax_rows
# ----------------------------------------------------------------------------------------------
ARGMAX_WIDE_ABOVE = 4096   # snap_argmax_rows_f32: P - start > 4096 takes argmax_rows_kernel<1024>


def argmax_threads(width):
  return 1024 if width > ARGMAX_WIDE_ABOVE else 256


ARGMAX_WIDTHS = (ARGMAX_WIDE_ABOVE, ARGMAX_WIDE_ABOVE + 1)     # one row length on each side of the switch


def argmax_case_rows(width, start, seed=7):
  """scores [R, start + width] f32 and the row names.  Indices below are relative to ``start``."""
  NT = argmax_threads(width)
  P = start + width
  rng = np.random.default_rng(seed + width + start)
  nan, inf = np.float32(np.nan), np.float32(np.inf)
  rows, names = [], []

  def row(name, edits, fill=None):
    r = rng.standard_normal(P).astype(np.float32) if fill is None else np.full(P, fill, np.float32)
    for k, v in edits:
      r[start + k] = v
    rows.append(r)
    names.append(name)
  for k in (0, 1, NT - 1, NT, NT + 1, width - 1):
    row(f'nan@{k}', [(k, nan)])
  row('nan@NT behind a larger value of the same thread', [(0, 50.0), (NT, nan)])
  row('two nans, first wins', [(3, nan), (NT + 3, nan)])
  row('two nans in one thread', [(NT + 3, nan), (2 * NT + 3, nan)])
  row('two adjacent nans', [(5, nan), (6, nan)])
  row('nan before +inf', [(50, nan), (100, inf)])
  row('nan after +inf', [(50, inf), (100, nan)])
  row('nan in the last slot, +inf in the first', [(0, inf), (width - 1, nan)])
  row('all nan', [], fill=nan)
  row('all -inf', [], fill=-inf)
  row('-inf but one', [(NT + 7, -3.0)], fill=-inf)
  row('+inf twice, first wins', [(NT - 1, inf), (NT, inf)])
  row('finite tie, first wins', [(9, 40.0), (NT + 9, 40.0)])
  if start > 0:                       # what lies before ``start`` is not part of the row
    r = rng.standard_normal(P).astype(np.float32)
    r[0] = nan
    r[start - 1] = inf
    rows.append(r)
    names.append('nan and +inf before start')
  return np.stack(rows), names


def argmax_want(scores, start):
  return np.argmax(scores[:, start:], axis=-1).astype(np.int32)


# ----------------------------------------------------------------------------------------------
# B. poses_from_corr
# ----------------------------------------------------------------------------------------------
NEAR_TIE_REL = 2.0 ** -20


def corr_random(seed, B, Nq, P, retries, X, Y):
  rng = np.random.default_rng(seed)
  n = P * retries * 2
  corr = np.stack([rng.integers(0, Nq, (B, n)), rng.integers(0, X, (B, n)), rng.integers(0, Y, (B, n))],
                  -1).astype(np.int32)
  corr[0, 0] = corr[0, 1]            # identical correspondences: ratio 0, the degenerate pair is selected
  q_xy = rng.uniform(-5, 5, (B, Nq, 2)).astype(np.float32)
  return corr, q_xy


POSE_RANDOM_CASES = [        # seed, B, Nq, P, retries, X, Y, cell
    (100, 2, 50, 200, 4, 30, 28, 0.2),
    (101, 2, 50, 200, 1, 30, 28, 0.2),
]


def poses_ref64(corr, q_xy, P, retries, cell):
  """float64 from the f32 ``q_xy``, the integer cells and the f32 cell size.  Returns a dict of arrays over
  [B, P, retries]: ``ratio``, ``pose`` [..., 3] (closed-form two-point Kabsch of EVERY retry), the first-order
  f32 bounds ``b_ang`` / ``b_t`` (multiply by MARGIN), and ``sel`` [B, P] (argmin, first minimum)."""
  c = np.asarray(corr).astype(np.int64)
  B = c.shape[0]
  xy = np.asarray(q_xy, np.float32).astype(np.float64)
  cs = np.float64(np.float32(cell))
  c = c.reshape(B, P, retries, 2, 3)
  i_xy = np.stack([xy[b][c[b, ..., 0]] for b in range(B)])                     # [B, P, R, 2, 2]
  j_xy = (c[..., 1:].astype(np.float64) + 0.5) * cs
  dq, da = i_xy[..., 1, :] - i_xy[..., 0, :], j_xy[..., 1, :] - j_xy[..., 0, :]
  d_i, d_j = np.sqrt((dq ** 2).sum(-1)), np.sqrt((da ** 2).sum(-1))
  if retries > 1:
    ratio = np.maximum(d_i / np.maximum(d_j, 1e-5), d_j / np.maximum(d_i, 1e-5))
  else:
    ratio = np.zeros_like(d_i)
  mu, nu = j_xy.mean(-2), i_xy.mean(-2)
  dot = (da * dq).sum(-1)
  crs = dq[..., 0] * da[..., 1] - dq[..., 1] * da[..., 0]
  nrm = np.sqrt(dot * dot + crs * crs)
  ok = nrm > 0
  co = np.where(ok, dot / np.where(ok, nrm, 1), 1.0)
  si = np.where(ok, crs / np.where(ok, nrm, 1), 0.0)
  t = mu - np.stack([co * nu[..., 0] - si * nu[..., 1], si * nu[..., 0] + co * nu[..., 1]], -1)
  pose = np.concatenate([np.arctan2(si, co)[..., None], t], -1)
  # First-order f32 bound.  q_xy is exact; a map coordinate (c + 0.5) * cell carries one rounding, a difference
  # one more: every component of the two difference vectors is off by at most ~EPS * cmax, which turns a vector of
  # length d by EPS * cmax / d.  dot, crs, nrm, the division and atan2f add a few EPS of the angle itself (<= pi),
  # as does storing it.  A pair with a zero difference gives dot = crs = 0 exactly on both sides: angle 0, no error.
  cmax = np.maximum(np.abs(i_xy).max((-1, -2)), np.abs(j_xy).max((-1, -2)))
  dmin = np.minimum(d_i, d_j)
  geo = np.where(dmin > 0, EPS * cmax / np.where(dmin > 0, dmin, 1), 0.0)
  b_ang = np.where(dmin > 0, geo + EPS * np.pi, 0.0)
  # t = mu - R nu: the angle error moves R nu by geo * |nu|; the means, the products and the result are rounded
  n_mu, n_nu, n_t = (np.sqrt((v ** 2).sum(-1)) for v in (mu, nu, t))
  b_t = geo * np.maximum(n_mu, n_nu) + EPS * (n_mu + n_nu + n_t)
  return dict(ratio=ratio, pose=pose, b_ang=b_ang, b_t=b_t, sel=np.argmin(ratio, -1), d_i=d_i, d_j=d_j,
              i_xy=i_xy, j_xy=j_xy)


def near_tie_candidates(ratio):
  """[B, P, R] bool: retries whose float64 ratio is within a relative 2^-20 of the minimum."""
  m = ratio.min(-1, keepdims=True)
  return ratio <= m * (1.0 + NEAR_TIE_REL)


def wrap(a):
  return np.abs(np.angle(np.exp(1j * a)))


def match_poses(got, ref):
  """got [B, P, 3] against ``poses_ref64``'s dict.  Returns (matched retry [B, P] or -1, worst fraction of the
  bound among the matched).  A pose may match only a near-tie candidate, within MARGIN x that retry's own bound;
  the float64 argmin is tried first."""
  g = np.asarray(got, np.float64)
  cand = near_tie_candidates(ref['ratio'])
  B, P, R = cand.shape
  out = -np.ones((B, P), np.int64)
  worst = 0.0
  for b, p in itertools.product(range(B), range(P)):
    order = [int(ref['sel'][b, p])] + [r for r in range(R) if r != ref['sel'][b, p]]
    for r in order:
      if not cand[b, p, r]:
        continue
      w = ref['pose'][b, p, r]
      ea, et = wrap(g[b, p, 0] - w[0]), np.abs(g[b, p, 1:] - w[1:]).max()
      ta, tt = MARGIN * ref['b_ang'][b, p, r], MARGIN * ref['b_t'][b, p, r]
      if ea <= ta and et <= tt:
        out[b, p] = r
        frac = max(ea / ta if ta > 0 else 0.0, et / tt if tt > 0 else 0.0)
        worst = max(worst, frac)
        break
  return out, worst


def check_poses_rule_b(name, got, corr, q_xy, P, retries, cell):
  """Every pose equals the float64 pose of a retry whose float64 ratio is within 2^-20 (relative) of the minimum,
  within MARGIN x the first-order f32 bound of that retry; poses that match another retry than the float64 argmin
  are near-ties: counted, printed, at most 1 % of the poses."""
  ref = poses_ref64(corr, q_xy, P, retries, cell)
  m, frac = match_poses(got, ref)
  lost = np.argwhere(m < 0)
  assert len(lost) == 0, (
      f'{name}: {len(lost)} poses match no admissible retry; first {lost[0].tolist()}: got '
      f'{np.asarray(got)[tuple(lost[0])]} float64 {ref["pose"][tuple(lost[0])][ref["sel"][tuple(lost[0])]]} '
      f'ratios {ref["ratio"][tuple(lost[0])]}')
  near = int((m != ref['sel']).sum())
  print(f'[poses] {name}: {m.size} poses, {near} near-tie(s), worst error {frac:.3f} of the bound x {MARGIN:g}')
  assert near <= 0.01 * m.size
  return near, frac


def planted_pose_cases():
  """Dyadic inputs (cell 0.25, q_xy in multiples of 1/8): every coordinate, difference, dot and cross product
  is exact in f32.  Returns a list of (name, corr [1, retries*2, 3], q_xy [1, Nq, 2], retries, winner, kind)."""
  q = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [0.375, 0.5], [-1.0, 0.0], [2.0, 0.0], [0.375, 1.5],
                [3.0, 4.0]], np.float32)[None]
  cases = []

  def add(name, pairs, winner, kind):
    corr = np.array([c for pr in pairs for c in pr], np.int32)[None]
    cases.append((name, corr, q, len(pairs), winner, kind))
  # d_i = 1, d_j = 0.25 * 4 = 1 for retries 0 and 1 (bit-equal ratio 1), translated copies: first wins
  add('equal ratios, first wins',
      [((0, 2, 3), (1, 6, 3)), ((3, 9, 1), (6, 9, 5)), ((0, 1, 1), (2, 1, 2))], 0, 'regular')
  # ratios 8, 2, 1: the strictly smaller ratio sits in the last retry
  add('smaller ratio last',
      [((0, 0, 0), (2, 0, 1)), ((0, 0, 0), (1, 0, 8)), ((0, 4, 4), (1, 4, 8))], 2, 'regular')
  # the three degenerate pairs; identical correspondences have ratio 0 and win wherever they stand
  add('identical correspondences', [((0, 0, 0), (1, 0, 8)), ((3, 5, 6), (3, 5, 6))], 1, 'degenerate')
  add('degenerate pair as the only retry', [((3, 5, 6), (3, 5, 6))], 0, 'degenerate')
  add('one query point, two cells', [((3, 5, 6), (3, 7, 2))], 0, 'degenerate')
  add('two query points, one cell', [((3, 5, 6), (7, 5, 6))], 0, 'degenerate')
  # q1 - q0 = (1, 0); map difference (-4 cells, 0) = (-1, 0): dot < 0, crs = +-0
  add('antipodal pair', [((0, 8, 3), (1, 4, 3))], 0, 'antipodal')
  add('antipodal pair, reversed', [((1, 8, 3), (0, 12, 3))], 0, 'antipodal')
  add('antipodal pair behind a worse retry', [((0, 0, 0), (1, 0, 8)), ((4, 12, 3), (0, 8, 3))], 1, 'antipodal')
  return cases


# ----------------------------------------------------------------------------------------------
# C. ransac_sample
# ----------------------------------------------------------------------------------------------
SIM_CH = 64
SAMPLER_SHAPES = [(65, 64), (67, 63), (5, 7), (128, 66)]
BRACKET = 1e-5
SAMPLER_SCALE = float(np.exp(2.5))
SAMPLER_NQ, SAMPLER_S, SAMPLER_DM = 12, 600, 64


def chunks_per_lane(X, Y):
  NC = (X * Y + SIM_CH - 1) // SIM_CH
  return NC, (NC + 63) // 64


def fast_sampler_dispatch(X, Y):
  """snap_ransac_sample_sim_f32 takes ransac_sample_fast_kernel with a workspace, sim and row_unscale when
  (NC + 63) / 64 <= 64."""
  return chunks_per_lane(X, Y)[1] <= 64


def _unit(a):
  return a / np.linalg.norm(a, axis=-1, keepdims=True)


def sampler_random_inputs(X, Y, seed, B=2, Nq=SAMPLER_NQ, Dm=SAMPLER_DM, S=SAMPLER_S):
  """Random unit-norm features: a map of iid directions in which one cell per 64 (at random places) resembles
  the scene's query direction, and query rows scattered around that direction.  The rows are then as peaked as
  a localizer's: with iid rows the float64 CDF alone puts 2.5 - 8 % of all uniforms within 1e-5 of a cell edge
  at 4000 - 8000 cells (every cell holds ~1e-4 of the mass), which would leave the bracket rule no meaning."""
  rng = np.random.default_rng(seed)
  XY = X * Y
  fm = _unit(rng.standard_normal((B, XY, Dm)))
  fq = np.empty((B, Nq, Dm))
  K = max(2, XY // 64)
  for b in range(B):
    g = _unit(rng.standard_normal(Dm))
    fq[b] = _unit(g + 0.02 * rng.standard_normal((Nq, Dm)))
    idx = rng.choice(XY, K, replace=False)
    fm[b, idx] = _unit(g + 0.02 * rng.standard_normal((K, Dm)))
  u = rng.random((B, S, 2)).astype(np.float32)
  return fq.astype(np.float32), fm.reshape(B, X, Y, Dm).astype(np.float32), u


SAMPLER_SEEDS = {(65, 64): 401, (67, 63): 402, (5, 7): 403, (128, 66): 404}


def row_cdfs64(fq, fm, scale, clip):
  """[B, Nq, XY] float64: exp(x - max) cumulated, NOT normalised -- the oracle's own expression per row."""
  q, m = np.asarray(fq, np.float64), np.asarray(fm, np.float64)
  B, Nq = q.shape[:2]
  out = np.empty((B, Nq, m.shape[1] * m.shape[2]))
  for b in range(B):
    for n in range(Nq):
      x = np.einsum('d,ijd->ij', q[b, n], m[b])
      if clip:
        x = np.maximum(x, 0)
      x = (x * scale).reshape(-1)
      out[b, n] = np.cumsum(np.exp(x - x.max()))
  return out


def rows_from_cdf_f32(row_cdf, u1):
  """The kernel's documented row rule with confidence weights: first n whose f32 inclusive CDF exceeds the f32
  product u1 * cdf[-1]."""
  c = np.asarray(row_cdf, np.float32)
  tgt = (np.asarray(u1, np.float32) * c[:, -1:]).astype(np.float32)
  return np.minimum((c[:, None, :] <= tgt[:, :, None]).sum(-1), c.shape[1] - 1)


def sampler_ref(fq, fm, scale, clip, u, row_cdf=None):
  """Two-level-free float64 inverse CDF: rows [B, S], cells [B, S], and the CDFs used."""
  cdf = row_cdfs64(fq, fm, scale, clip)
  B, Nq, XY = cdf.shape
  u = np.asarray(u, np.float32)
  if row_cdf is None:
    rows = np.minimum((u[..., 0] * np.float32(Nq)).astype(np.int64), Nq - 1)
  else:
    rows = rows_from_cdf_f32(row_cdf, u[..., 0])
  cells = np.empty(rows.shape, np.int64)
  for b in range(B):
    for s in range(rows.shape[1]):
      c = cdf[b, rows[b, s]]
      cells[b, s] = min(int(np.searchsorted(c, np.float64(u[b, s, 1]) * c[-1], side='right')), XY - 1)
  return rows, cells, cdf


def edge_distance(cdf, rows, cells, u2):
  """Distance of every uniform from the nearer edge of its own float64 CDF cell, in units of the row mass."""
  B, S = rows.shape
  out = np.empty((B, S))
  for b in range(B):
    c = cdf[b, rows[b]]
    tot = c[:, -1]
    hi = c[np.arange(S), cells[b]] / tot
    lo = np.where(cells[b] > 0, c[np.arange(S), np.maximum(cells[b] - 1, 0)] / tot, 0.0)
    t = np.asarray(u2[b], np.float64)
    out[b] = np.minimum(np.abs(t - lo), np.abs(hi - t))
  return out


def bracketed(cdf, rows, got_cells, u2):
  """The acceptance rule of test_ransac_sample_given_uniforms: the float64 CDF at the returned cell brackets
  the uniform within 1e-5 of the row mass."""
  B, S = rows.shape
  ok = np.empty((B, S), bool)
  for b in range(B):
    c = cdf[b, rows[b]]
    tot = c[:, -1]
    hi = c[np.arange(S), got_cells[b]] / tot
    lo = np.where(got_cells[b] > 0, c[np.arange(S), np.maximum(got_cells[b] - 1, 0)] / tot, 0.0)
    t = np.asarray(u2[b], np.float64)
    ok[b] = (lo - BRACKET <= t) & (t <= hi + BRACKET)
  return ok


ONE_HOT_SCALE = 60.0


def one_hot_targets(X, Y):
  XY = X * Y
  NC, cpl = chunks_per_lane(X, Y)
  t = [0, XY - 1, 63, 64, 64 * cpl - 1, 64 * cpl]
  if (X, Y) == (65, 64):
    t.append(64 * 64 + 5)            # chunk 64: the single chunk of lane 32, the last non-empty lane
  return sorted({c for c in t if 0 <= c < XY})


def one_hot_inputs(X, Y, seed=11, per_row=48, Dm=8):
  """Row n: fq = e0, fm[target n] = e0 and e1 elsewhere (one scene per target, so B = number of targets and
  every scene has ONE query row).  u2 in [2^-20, 1 - 2^-20], both ends included."""
  tg = one_hot_targets(X, Y)
  B, XY = len(tg), X * Y
  fq = np.zeros((B, 1, Dm), np.float32)
  fq[..., 0] = 1
  fm = np.zeros((B, XY, Dm), np.float32)
  fm[..., 1] = 1
  for b, c in enumerate(tg):
    fm[b, c] = 0
    fm[b, c, 0] = 1
  rng = np.random.default_rng(seed)
  lo = 2.0 ** -20
  u = np.empty((B, per_row, 2), np.float32)
  u[..., 0] = rng.random((B, per_row))
  u[..., 1] = rng.uniform(lo, 1 - lo, (B, per_row))
  u[:, 0, 1], u[:, 1, 1], u[:, 2, 1] = lo, 1 - lo, 0.5
  assert u[..., 1].min() >= np.float32(lo) and u[..., 1].max() <= np.float32(1 - lo)
  return fq, fm.reshape(B, X, Y, Dm), u, np.array(tg)


# ----------------------------------------------------------------------------------------------
# D. pose_score
# ----------------------------------------------------------------------------------------------
PS_LDS_FLOATS = 24 * 1024
PS_DB_PLANE_BYTES = 5 * 1024 * 16 - 12 * 1024


def pose_score_body(X, Y, mask_oob):
  """The dispatch of snap_pose_score_f32, restated: (body, band rows, bands, first row of every band)."""
  if X * Y <= PS_LDS_FLOATS:
    RB, NB = X, 1
  else:
    RB = PS_LDS_FLOATS // Y
    NB = (X - 1 + (RB - 1) - 1) // (RB - 1)
  bands = NB > 1
  use_db = (not bands) and Y % 4 == 0 and X >= 2 and Y >= 2 and X * (Y + 4) * 4 <= PS_DB_PLANE_BYTES
  band_rows = PS_DB_PLANE_BYTES // ((Y + 4) * 4) - 1
  use_band_db = ((not use_db) and (not mask_oob) and Y % 4 == 0 and X >= 2 and Y >= 2 and band_rows >= 1
                 and X > band_rows)
  if use_band_db:
    nb = (X - 1 + band_rows - 1) // band_rows
    return 'band_db', band_rows, nb, [k * band_rows for k in range(1, nb)]
  if use_db:
    return ('db128' if Y == 128 else 'db'), X, 1, []
  if bands:
    return 'plain_banded', RB, NB, [k * (RB - 1) for k in range(1, NB + 1) if k * (RB - 1) <= X - 1]
  return 'plain', RB, NB, []


def window_supported(X, Y, rad):
  if X < 2 or Y < 4 or Y % 4 or rad < 0:
    return False
  WR, WC = min(2 * rad + 3, X), min((2 * rad + 9) & ~3, Y)
  return WR * ((WC >> 2) + 1) <= 3 * 1024


POSE_SCORE_SHAPES = [      # X, Y, mask_oob, body
    (9, 7, False, 'plain'), (9, 7, True, 'plain'),
    (70, 1023, False, 'plain_banded'), (70, 1023, True, 'plain_banded'), (23, 2044, True, 'plain_banded'),
    (8, 128, False, 'db128'), (8, 128, True, 'db128'),
    (8, 12, False, 'db'), (8, 12, True, 'db'),
    (23, 2044, False, 'band_db'),
]
WINDOW_SHAPE = (16, 16, 3)   # X, Y, radius in cells

PLANT_Q = np.array([[0.0, 0.0], [0.25, -0.5], [-0.125, 0.0625], [0.625, 0.3125], [-0.75, 1.0]], np.float32)


def _axis_targets(n, dense):
  """Coordinates in cells along an axis of n cells: every centre and every three-quarter point (both taps of every
  row pair, every seam), the borders and both half-cell strips, just below n, n itself (out), beyond, negative."""
  edge = [0.0, 0.25, n - 0.25, n - 2.0 ** -6, float(n), n + 0.5, -0.25, -3.5]
  if dense:
    body = [i + f for i in range(n) for f in (0.5, 0.75)]
  else:
    body = [i + f for i in (0, 1, n // 2, n - 2, n - 1) for f in (0.5, 0.75)]
  return np.array(sorted(set(edge + body)))


def planted_poses(X, Y, u_lim=None, v_lim=None):
  """theta = 0 poses whose image of PLANT_Q[0] runs over the target coordinates; [P, 3] f32, exact."""
  U, V = _axis_targets(X, True), _axis_targets(Y, Y <= 128)
  if u_lim is not None:
    U = U[(U >= u_lim[0]) & (U <= u_lim[1])]
  if v_lim is not None:
    V = V[(V >= v_lim[0]) & (V <= v_lim[1])]
  uu, vv = np.meshgrid(U, V, indexing='ij')
  t = np.stack([uu.reshape(-1) * CELL - PLANT_Q[0, 0], vv.reshape(-1) * CELL - PLANT_Q[0, 1]], -1)
  poses = np.concatenate([np.zeros((len(t), 1)), t], -1)
  assert np.array_equal(poses.astype(np.float32).astype(np.float64), poses)
  return poses.astype(np.float32)


def tap_probe(X, Y, seams):
  """A pose that puts PLANT_Q[0] at (i + 0.75, j + 0.75) with i on a seam row where there is one, and its four
  taps.  planted_poses() contains it."""
  i = min(seams[0], X - 2) if seams else min(X - 2, X // 2)
  j = min(Y - 2, 1)
  taps = [(i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)]
  return (i + 0.75, j + 0.75), taps


def planted_map_valid(X, Y, seams):
  """[4, X, Y] bool: scene k has exactly one invalid cell, under tap k of the probe."""
  _, taps = tap_probe(X, Y, seams)
  mv = np.ones((4, X, Y), bool)
  for k, (i, j) in enumerate(taps):
    mv[k, i, j] = False
  return mv


def score_terms64(sim, poses, q_xy, cell):
  """float64 terms of ONE scene: value [P, Nq] (bilinear, 'nearest' extension), in-bounds [P, Nq], the taps
  (i0, i1, j0, j1) [P, Nq] each, and u, v [P, Nq] in cells (pose_estimation.py:49-82 as oracle/pose.py states)."""
  s = np.asarray(sim, np.float64)
  p, xy = np.asarray(poses, np.float64), np.asarray(q_xy, np.float64)
  N, X, Y = s.shape
  co, si = np.cos(p[:, 0:1]), np.sin(p[:, 0:1])
  u = (co * xy[None, :, 0] - si * xy[None, :, 1] + p[:, 1:2]) / cell
  v = (si * xy[None, :, 0] + co * xy[None, :, 1] + p[:, 2:3]) / cell
  inb = (u >= 0) & (u < X) & (v >= 0) & (v < Y)
  cu, cv = u - 0.5, v - 0.5
  fu, fv = np.floor(cu), np.floor(cv)
  wu, wv = cu - fu, cv - fv
  i0 = np.clip(fu, 0, X - 1).astype(np.int64); i1 = np.clip(fu + 1, 0, X - 1).astype(np.int64)
  j0 = np.clip(fv, 0, Y - 1).astype(np.int64); j1 = np.clip(fv + 1, 0, Y - 1).astype(np.int64)
  n = np.arange(N)[None]
  val = ((1 - wu) * (1 - wv) * s[n, i0, j0] + (1 - wu) * wv * s[n, i0, j1]
         + wu * (1 - wv) * s[n, i1, j0] + wu * wv * s[n, i1, j1])
  return val, inb, (i0, i1, j0, j1), u, v


def scores64(sim, poses, q_xy, valid_q, map_valid, cell, mask_oob):
  """[P] float64 scores of one scene, and the [P, Nq] validity that entered them."""
  val, inb, (i0, i1, j0, j1), _, _ = score_terms64(sim, poses, q_xy, cell)
  ok = np.broadcast_to(np.asarray(valid_q, bool)[None], val.shape).copy()
  if mask_oob:
    mv = np.asarray(map_valid, bool)
    ok &= inb & mv[i0, j0] & mv[i0, j1] & mv[i1, j0] & mv[i1, j1]
  return (ok * val).sum(-1), ok


BORDER_TOL = 1e-4          # cells: a point this close to 0, X or Y may flip between two f32 evaluations


def explain_by_border_flips(got, sim, poses, q_xy, valid_q, map_valid, cell, atol, rtol):
  """The rule of helpers.assert_validity_mismatches_on_borders for pose scores under mask_oob: every score beyond
  tolerance must be reproduced by flipping the in-bounds test of points whose float64 u or v lies within
  BORDER_TOL of 0, X or Y.  Returns the number of such poses; raises on an unexplained one."""
  want, ok = scores64(sim, poses, q_xy, valid_q, map_valid, cell, True)
  val, inb, (i0, i1, j0, j1), u, v = score_terms64(sim, poses, q_xy, cell)
  X, Y = np.asarray(sim).shape[1:]
  mv = np.asarray(map_valid, bool)
  taps = mv[i0, j0] & mv[i0, j1] & mv[i1, j0] & mv[i1, j1]
  near = np.minimum.reduce([np.abs(u), np.abs(u - X), np.abs(v), np.abs(v - Y)]) <= BORDER_TOL
  flippable = near & taps & np.asarray(valid_q, bool)[None]
  g = np.asarray(got, np.float64)
  bad = np.nonzero(np.abs(g - want) > atol + rtol * np.abs(want))[0]
  for p in bad:
    idx = np.nonzero(flippable[p])[0]
    assert 0 < len(idx) <= 12, f'pose {p}: score {g[p]} vs {want[p]} and no point on a border'
    hit = False
    for k in range(1, len(idx) + 1):
      for sub in itertools.combinations(idx, k):
        alt = want[p] + sum((-1.0 if ok[p, n] else 1.0) * val[p, n] for n in sub)
        if abs(g[p] - alt) <= atol + rtol * abs(alt):
          hit = True
    assert hit, f'pose {p}: score {g[p]} vs {want[p]} is not explained by its {len(idx)} border point(s)'
  return len(bad), int(flippable.sum())


def rotated_case(X, Y, seed, B=2, Nq=12, P=700, cell=0.2):
  rng = np.random.default_rng(seed)
  sim = rng.random((B, Nq, X, Y), dtype=np.float32)
  poses = np.stack([rng.uniform(-np.pi, np.pi, (B, P)), rng.uniform(-0.2 * X * cell, 1.2 * X * cell, (B, P)),
                    rng.uniform(-0.2 * Y * cell, 1.2 * Y * cell, (B, P))], -1).astype(np.float32)
  q_xy = rng.uniform(-2, 2, (B, Nq, 2)).astype(np.float32)
  valid_q = rng.random((B, Nq)) > 0.2
  map_valid = rng.random((B, X, Y)) > 0.1
  return sim, poses, q_xy, valid_q, map_valid, cell


# ----------------------------------------------------------------------------------------------
# E. masked_softmax_rows
# ----------------------------------------------------------------------------------------------
SOFTMAX_N = (1, 2, 255, 256, 257, 511, 513)
SOFTMAX_ROWS = ('random mask', 'last element only', 'last segment only', 'all false', '-inf under a true mask')


def softmax_case(N, seed=31):
  """x [5, N] f32, mask [5, N] bool; the rows are SOFTMAX_ROWS.  The kernel gives thread t the segment
  [t seg, (t + 1) seg) with seg = ceil(N / 256)."""
  rng = np.random.default_rng(seed + N)
  x = (rng.standard_normal((5, N)) * 3).astype(np.float32)
  m = np.zeros((5, N), bool)
  m[0] = rng.random(N) > 0.4
  m[0, rng.integers(N)] = True
  m[1, N - 1] = True
  seg = (N + 255) // 256
  m[2, ((N - 1) // seg) * seg:] = True
  m[4] = True
  if N >= 2:
    m[4, 1::3] = False
    x[4, 0] = -np.inf                      # index 0 is valid in this row; N - 1 or 2 keeps a finite one valid
    m[4, N - 1] = True
  return x, m


def softmax_want(x, m):
  from oracle import bev as o_bev
  w = o_bev.layers_masked_softmax(np.asarray(x, np.float64), np.asarray(m, bool), -1)
  return w, np.cumsum(w, -1)

