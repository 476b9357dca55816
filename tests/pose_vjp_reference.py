"""Float64 restatement of the pose head's VJP kernels (``snap_amd/csrc/pose_bwd.hip``), their dispatch and bounds.

numpy float64 only; nothing of ``snap_amd`` is imported.  ``test_pose_vjp_reference.py`` shows on the CPU that every
input below satisfies its stated condition on the reference alone and that the tolerances reject the named mutants;
``test_gpu_pose_vjp.py`` runs the kernels against it.

``pose_score_vjp`` is the VJP of bilinear pose scoring: tap coordinates ``cu = u - 0.5`` with
``u = (cos x - sin y + tx) / cell``, taps at ``floor(cu)`` and ``floor(cu) + 1`` clamped to the plane, weights from
the UNclamped fraction (a sample that leaves the plane puts its whole weight on the border cell), and under
``mask_oob`` the test ``0 <= u < X`` (``v`` alike) and the validity of all four taps.  ``twin=<seed>`` is a NOISE
TWIN: the pose table rounded to f32 and moved one ulp up or down at random, the coordinates through the kernel's
``fmaf`` chain rounded to f32, weights and products rounded to f32, sums in float64.  ``abs(model - twin)`` is what
the freedom of a correct f32 implementation is worth on an input; tolerances are ``MARGIN`` times its maximum over
``TWIN_SEEDS`` draws plus a summation term, from the reference alone.  ``mutant=<name>`` is a wrong kernel.
"""
import functools

import numpy as np

U = 2.0 ** -24             # f32 rounding unit
MARGIN = 8.0               # over the twins' deviation (attention_reference's factor)
TWIN_SEEDS = tuple(range(8))
ATOL_G, RTOL = 2e-4, 1e-4  # test_pose_score_bwd's tolerance, in units of max|cotangent|: the validity limit
BORDER_TOL = 1e-4          # cells: mask_oob cases keep every sample this far from a decision (see `random_case`)

# ----------------------------------------------------------------------------------------------------
# the launcher snap_pose_score_bwd_ex_f32, restated from its text
# ----------------------------------------------------------------------------------------------------
PB_THREADS = 1024
PB_PPT = 10
PB_LDS_FLOATS = 24 * 1024            # X * Y above this: SNAP_ERR_UNSUPPORTED
PB_DET_BYTES = 152 * 1024            # the 8-byte plane must fit in this for the fixed-point body
LDS_DEFAULT = 64 * 1024              # above this the launcher raises the dynamic-LDS attribute
PB_CHUNK_TARGET = 512                # workgroups per launch the chunking aims at


def chunking(B, Nq):
  """(points_per_chunk, chunks): one workgroup walks `points_per_chunk` points of one scene."""
  nch = min(-(-PB_CHUNK_TARGET // B), Nq)
  ppc = -(-Nq // nch)
  return ppc, -(-Nq // ppc)


def dispatch(B, Nq, X, Y, P, mask_oob, float_atomics=False):
  """What the launcher does with a shape: body, dynamic LDS bytes, chunking, passes, highest live register slot."""
  if X * Y > PB_LDS_FLOATS:
    return dict(supported=False)
  fast = (not mask_oob) and P <= PB_THREADS * PB_PPT and X >= 2 and Y >= 2
  det = fast and X * Y * 8 <= PB_DET_BYTES and not float_atomics
  body = 'det' if det else 'fast' if fast else 'general_mask' if mask_oob else 'general'
  lds = X * Y * (8 if det else 4)
  ppc, nch = chunking(B, Nq)
  return dict(supported=True, body=body, lds=lds, lds_raised=lds > LDS_DEFAULT, points_per_chunk=ppc, chunks=nch,
              ragged=Nq % ppc != 0, passes=1 if fast else -(-P // (PB_THREADS * PB_PPT)),
              top_slot=min(P - 1, PB_THREADS * PB_PPT - 1) // PB_THREADS)


def branch_key(d):
  return (d['body'], d['lds_raised'], d['points_per_chunk'] > 1, d['ragged'], d['passes'], d['top_slot'])


# ----------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------
MUTANTS = ('drop_slot', 'swap_corners', 'no_plane_reset', 'last_chunk_dropped', 'weights_swapped',
           'second_pass_dropped', 'invalid_point_keeps_plane')


def r32(a):
  return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def f64(a):
  return np.asarray(a, np.float32).astype(np.float64)


def pose_table(poses, cell, rng=None, f32=False):
  """[..., 4]: cos / cell, sin / cell, x / cell - 0.5, y / cell - 0.5 of f32 poses and the f32 cell size."""
  p = f64(poses)
  c = float(np.float32(cell))
  t = np.stack([np.cos(p[..., 0]) / c, np.sin(p[..., 0]) / c, p[..., 1] / c - 0.5, p[..., 2] / c - 0.5], -1)
  if rng is not None:
    t32 = t.astype(np.float32)
    up = rng.random(t.shape) < 0.5
    t = np.where(up, np.nextafter(t32, np.float32(np.inf)), np.nextafter(t32, np.float32(-np.inf))).astype(np.float64)
  elif f32:
    t = r32(t)
  return t


def _scene_taps(table, q, valid_q, map_valid, X, Y, mask_oob, lo, mutant):
  """One scene.  Returns ok [Nq, P] and the four taps as (cell index [Nq, P], weight [Nq, P]).  `lo`: every
  operation rounded to f32 (the noise twin's and the f32 evaluation's arithmetic)."""
  rd = r32 if lo else (lambda a: a)
  A, S, Cx, Cy = (table[None, :, k] for k in range(4))
  qx, qy = f64(q[:, 0:1]), f64(q[:, 1:2])
  cu = rd(A * qx + rd(-S * qy + Cx))
  cv = rd(S * qx + rd(A * qy + Cy))
  fu, fv = np.floor(cu), np.floor(cv)
  wu1, wv1 = rd(cu - fu), rd(cv - fv)
  wu0, wv0 = rd(1.0 - wu1), rd(1.0 - wv1)
  if mutant == 'weights_swapped':
    wu0, wu1 = wu1, wu0
  i0 = np.clip(fu, 0, X - 1).astype(np.int64)
  i1 = np.clip(fu + 1, 0, X - 1).astype(np.int64)
  j0 = np.clip(fv, 0, Y - 1).astype(np.int64)
  j1 = np.clip(fv + 1, 0, Y - 1).astype(np.int64)
  ok = np.broadcast_to(np.asarray(valid_q, bool)[:, None], cu.shape).copy()
  if mask_oob:
    u, v = rd(cu + 0.5), rd(cv + 0.5)
    mv = np.asarray(map_valid, bool)
    ok &= (u >= 0) & (u < X) & (v >= 0) & (v < Y) & mv[i0, j0] & mv[i0, j1] & mv[i1, j0] & mv[i1, j1]
  P = table.shape[0]
  if mutant == 'drop_slot':
    ok &= (np.arange(P) // PB_THREADS != PB_PPT - 1)[None]
  if mutant == 'second_pass_dropped':
    ok &= (np.arange(P) < PB_THREADS * PB_PPT)[None]
  taps = [(i * Y + j, rd(wi * wj)) for i, wi in ((i0, wu0), (i1, wu1)) for j, wj in ((j0, wv0), (j1, wv1))]
  return ok, taps, (cu, cv)


def pose_score_vjp(dscores, poses, q_xy, valid_q, map_valid, shape, cell, mask_oob, twin=None, mutant=None,
                   stats=False, order=None):
  """dsim [B, Nq, X, Y] in float64.  stats=True: also n_c (non-zero terms per cell) and T_c = sum |g_p| w_p,c.
  order=<seed>: the f32 evaluation -- every operation AND the sums in f32, terms added in a random order."""
  B, Nq, X, Y = shape
  XY = X * Y
  assert mutant is None or mutant in MUTANTS
  rng = None if twin is None else np.random.default_rng([int(twin), 77])
  lo = twin is not None or order is not None
  table = pose_table(poses, cell, rng, f32=order is not None)
  g = f64(dscores)
  out = np.zeros((B, Nq * XY))
  n_c = np.zeros((B, Nq * XY), np.int32) if stats else None
  T_c = np.zeros((B, Nq * XY)) if stats else None
  base = (np.arange(Nq) * XY)[:, None]
  for b in range(B):
    ok, taps, _ = _scene_taps(table[b], q_xy[b], valid_q[b], None if map_valid is None else map_valid[b], X, Y,
                              mask_oob, lo, mutant)
    gg = np.where(ok, g[b][None], 0.0)
    idx = np.concatenate([(base + c).ravel() for c, _ in taps])
    term = np.concatenate([(r32(w * gg) if lo else w * gg).ravel() for _, w in taps])
    if order is not None:
      acc = np.zeros(Nq * XY, np.float32)
      perm = np.random.default_rng([int(order), 78]).permutation(len(idx))
      np.add.at(acc, idx[perm], term[perm].astype(np.float32))
      out[b] = acc
    else:
      out[b] = np.bincount(idx, weights=term, minlength=Nq * XY)
    if stats:
      n_c[b] = np.bincount(idx[term != 0], minlength=Nq * XY)
      T_c[b] = np.bincount(idx, weights=np.abs(term), minlength=Nq * XY)
  out = out.reshape(B, Nq, X, Y)
  if mutant == 'swap_corners':
    a = out[:, :, 0, Y - 1].copy()
    out[:, :, 0, Y - 1] = out[:, :, X - 1, 0]
    out[:, :, X - 1, 0] = a
  if mutant in ('no_plane_reset', 'last_chunk_dropped', 'invalid_point_keeps_plane'):
    ppc, nch = chunking(B, Nq)
    own = out.copy()
    vq = np.asarray(valid_q, bool)
    if mutant == 'last_chunk_dropped':
      out[:, (nch - 1) * ppc:] = 0.0
    else:
      for n in range(1, Nq):
        if n % ppc == 0:
          continue
        if mutant == 'no_plane_reset':
          sel = vq[:, n] & vq[:, n - 1]
          out[sel, n] += own[sel, n - 1]
        else:
          sel = ~vq[:, n]
          out[sel, n] = own[sel, n - 1]
  if stats:
    return out, n_c.reshape(B, Nq, X, Y), T_c.reshape(B, Nq, X, Y)
  return out


def pose_score_fwd(sim, poses, q_xy, valid_q, map_valid, cell, mask_oob, twin=None, stats=False):
  """scores [B, P] of the same taps (float64), for the adjoint identity.  stats=True: also sum |w sim| per pose."""
  B, Nq, X, Y = sim.shape
  rng = None if twin is None else np.random.default_rng([int(twin), 77])
  lo = twin is not None
  table = pose_table(poses, cell, rng)
  s = f64(sim).reshape(B, Nq, X * Y)
  P = table.shape[1]
  out, mass = np.zeros((B, P)), np.zeros((B, P))
  rows = np.arange(Nq)[:, None]
  for b in range(B):
    ok, taps, _ = _scene_taps(table[b], q_xy[b], valid_q[b], None if map_valid is None else map_valid[b], X, Y,
                              mask_oob, lo, None)
    for c, w in taps:
      t = np.where(ok, w * s[b][rows, c], 0.0)
      t = r32(t) if lo else t
      out[b] += t.sum(0)
      mass[b] += np.abs(t).sum(0)
  return (out, mass) if stats else out


def scale_exponent(dscores):
  """Per scene: e with 2^e the smallest power of two above the largest finite |g| (floored at 1e-37)."""
  g = np.abs(f64(dscores))
  gm = np.where(np.isfinite(g), g, 0.0).max(-1)
  return np.frexp(np.maximum(gm, float(np.float32(1e-37))))[1], gm


def corner_mask(X, Y):
  m = np.zeros((X, Y), bool)
  m[0, 0] = m[0, Y - 1] = m[X - 1, 0] = m[X - 1, Y - 1] = True
  return m


def tolerances(ref, n_c, T_c, noise, dscores):
  """(tol of a float-atomic body, tol of the fixed-point body), cell by cell.  noise [B, Nq]."""
  e, _ = scale_exponent(dscores)
  nz = noise[:, :, None, None]
  tol_float = nz + n_c * U * T_c
  tol_fixed = nz + n_c * np.ldexp(1.0, e - 39)[:, None, None, None] + U * np.abs(ref)
  # a corner cell of the fixed-point body is BOTH: the f32 sum of the samples clamped in both directions plus the
  # fixed-point sum of the samples that reach the cell through a tap -- the float term and the grid term together
  tol_fixed = np.where(corner_mask(*ref.shape[2:])[None, None], tol_fixed + n_c * U * T_c, tol_fixed)
  return tol_float, tol_fixed


def validity_limit(ref, dscores):
  _, gm = scale_exponent(dscores)
  return gm[:, None, None, None] * ATOL_G + RTOL * np.abs(ref)


# ----------------------------------------------------------------------------------------------------
# B. the random cases
# ----------------------------------------------------------------------------------------------------
CELL_RANDOM = 0.2

# name, seed, B, Nq, X, Y, P, mask_oob
VJP_CASES = [
    ('slot0-P1', 11, 2, 6, 24, 20, 1, False),
    ('slot0-P1023', 12, 2, 6, 24, 20, 1023, False),
    ('slot0-P1024', 13, 2, 6, 24, 20, 1024, False),
    ('slot1-P1025', 14, 2, 6, 24, 20, 1025, False),
    ('slot9-P10239', 15, 1, 6, 24, 20, 10239, False),
    ('slot9-P10240', 16, 1, 6, 24, 20, 10240, False),
    ('general-2pass', 17, 1, 6, 24, 20, 10241, False),
    ('masked-2pass', 18, 1, 6, 24, 20, 10241, True),
    ('chunk3-ragged', 19, 3, 400, 24, 20, 1500, False),
    ('chunk3-ragged-masked', 20, 3, 400, 24, 20, 1500, True),
    ('chunk4', 21, 8, 200, 16, 16, 700, False),
    ('64x128-at-64K', 22, 1, 5, 64, 128, 1500, False),
    ('91x91-above-64K', 23, 1, 5, 91, 91, 1500, False),
    ('128x128-training', 24, 1, 5, 128, 128, 2500, False),
    ('129x128-float-above-64K', 25, 1, 5, 129, 128, 1500, False),
    ('152x128-largest-fixed', 126, 1, 5, 152, 128, 1500, False),
    ('139x140-float-by-shape', 27, 1, 5, 139, 140, 1500, False),
    ('192x128-largest', 528, 1, 5, 192, 128, 1500, False),
    ('192x128-largest-masked', 29, 1, 5, 192, 128, 1500, True),
    ('128x128-chunk3', 430, 2, 700, 128, 128, 300, False),
]
VJP_CASE_IDS = [c[0] for c in VJP_CASES]
ADJOINT_CASES = ('slot1-P1025', 'masked-2pass')
# which case of the table rejects which mutant (test_pose_vjp_reference.py asserts each pair)
MUTANT_CASES = {
    'drop_slot': ('slot9-P10239', 'slot9-P10240'),
    'swap_corners': ('slot1-P1025', '128x128-training'),
    'no_plane_reset': ('chunk3-ragged', 'chunk4', '128x128-chunk3'),
    'last_chunk_dropped': ('chunk3-ragged', 'chunk3-ragged-masked'),
    'weights_swapped': ('slot0-P1', 'slot0-P1023', '192x128-largest-masked'),
    'second_pass_dropped': ('general-2pass', 'masked-2pass'),
    'invalid_point_keeps_plane': ('chunk3-ragged', 'chunk3-ragged-masked', 'chunk4'),
}
UNSUPPORTED_SHAPES = [(7, 3511)]


def case_by_name(name):
  return VJP_CASES[VJP_CASE_IDS.index(name)]


LIVE_COTANGENTS = 1024     # expected non-zero cotangents per scene, at most


def cotangents(rng, shape):
  """Signed, five octaves wide, and exactly zero on all but about LIVE_COTANGENTS poses of a scene, spread over
  every register slot.  A corner cell of a 24 x 20 plane collects a sixth of all samples; the summation term
  n_c 2^-24 T_c grows with the SQUARE of the live ones and passes the validity limit near 300 of them."""
  g = rng.standard_normal(shape) * 2.0 ** -rng.integers(0, 6, shape)
  live = rng.random(shape) < LIVE_COTANGENTS / max(shape[-1], LIVE_COTANGENTS)
  return np.where(live, g, 0.0).astype(np.float32)


def forced_valid(rng, B, Nq):
  """About 80 % true.  Where a workgroup walks several points: chunk 1 starts, chunk 2 continues and chunk 3 ends
  with an invalid point (their other points valid), chunk 4 is invalid throughout; else one invalid point per
  scene between valid ones."""
  vq = rng.random((B, Nq)) > 0.2
  ppc, nch = chunking(B, Nq)
  if ppc > 1:
    assert nch >= 6
    for k, hole in ((1, 0), (2, 1 if ppc > 2 else 0), (3, ppc - 1)):
      vq[:, k * ppc:(k + 1) * ppc] = True
      vq[:, k * ppc + hole] = False
    vq[:, 4 * ppc:5 * ppc] = False
    vq[:, 0:ppc] = True
    vq[:, Nq - 1] = True                 # the last chunk (the ragged one, where there is one) has work
  else:
    vq[:, :3] = [True, False, True]
  return vq


def random_case(case):
  """Inputs of a row of VJP_CASES.  Under mask_oob the in-bounds test, the tap pair and with it the taps' validity
  are DECISIONS: a pose with a sample whose float64 tap coordinate lies within BORDER_TOL cell of a multiple of
  one half is drawn again, so that no correct f32 evaluation (coordinate error below 2e-5 cell at these extents)
  decides otherwise than the model."""
  name, seed, B, Nq, X, Y, P, mask = case
  rng = np.random.default_rng(seed)
  cell = CELL_RANDOM

  def draw(n):
    return np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.2, 1.2, n) * X * cell,
                     rng.uniform(-0.2, 1.2, n) * Y * cell], -1).astype(np.float32)
  poses = draw(B * P).reshape(B, P, 3)
  q_xy = rng.uniform(-1.5, 1.5, (B, Nq, 2)).astype(np.float32)
  g = cotangents(rng, (B, P))
  g[:, [0, P - 1]] = np.where(g[:, [0, P - 1]] == 0, np.float32(0.75), g[:, [0, P - 1]])   # first and last pose live
  vq = forced_valid(rng, B, Nq)
  mv = rng.random((B, X, Y)) > 0.1
  if mask:
    for _ in range(200):
      table = pose_table(poses, cell)
      bad = np.zeros((B, P), bool)
      for b in range(B):
        _, _, (cu, cv) = _scene_taps(table[b], q_xy[b], vq[b], mv[b], X, Y, False, False, None)
        near = (np.abs(2 * cu - np.round(2 * cu)) < 2 * BORDER_TOL) | (np.abs(2 * cv - np.round(2 * cv)) < 2 * BORDER_TOL)
        bad[b] = near.any(0)
      if not bad.any():
        break
      poses[bad] = draw(int(bad.sum()))
    assert not bad.any()
  return dict(name=name, dscores=g, poses=poses, q_xy=q_xy, valid_q=vq, map_valid=mv, shape=(B, Nq, X, Y),
              cell=cell, mask_oob=mask)


def decision_margin(inp):
  """Smallest distance (cells) of a sample's float64 tap coordinate from a multiple of one half."""
  B, Nq, X, Y = inp['shape']
  table = pose_table(inp['poses'], inp['cell'])
  m = np.inf
  for b in range(B):
    _, _, (cu, cv) = _scene_taps(table[b], inp['q_xy'][b], inp['valid_q'][b], None, X, Y, False, False, None)
    m = min(m, float(np.abs(2 * cu - np.round(2 * cu)).min()) / 2, float(np.abs(2 * cv - np.round(2 * cv)).min()) / 2)
  return m


def model_of(inp, **kw):
  return pose_score_vjp(inp['dscores'], inp['poses'], inp['q_xy'], inp['valid_q'], inp['map_valid'], inp['shape'],
                        inp['cell'], inp['mask_oob'], **kw)


def reference_of(inp):
  """Model, per-cell term statistics, per-plane noise and both tolerances of an input dict."""
  ref, n_c, T_c = model_of(inp, stats=True)
  noise = np.zeros(ref.shape[:2])
  for s in TWIN_SEEDS:
    noise = np.maximum(noise, np.abs(model_of(inp, twin=s) - ref).max((2, 3)))
  noise *= MARGIN
  tol_float, tol_fixed = tolerances(ref, n_c, T_c, noise, inp['dscores'])
  return dict(inp, ref=ref, n_c=n_c, T_c=T_c, noise=noise, tol_float=tol_float, tol_fixed=tol_fixed)


@functools.lru_cache(maxsize=2)
def case_reference(name):
  return reference_of(random_case(case_by_name(name)))


def worst(got, ref, tol):
  """(largest err / tol, its index).  A cell of tolerance 0 must be met exactly."""
  err = np.abs(np.asarray(got, np.float64) - ref)
  err = np.where(np.isnan(err), np.inf, err)
  ratio = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
  i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
  return float(ratio[i]), tuple(int(k) for k in i)


# ----------------------------------------------------------------------------------------------------
# A. the exact planted grid
# ----------------------------------------------------------------------------------------------------
CELL_EXACT = 0.25
EXACT_Q = np.array([[0.0, 0.0], [0.25, -0.5], [-0.125, 0.0625], [0.625, 0.3125], [-0.75, 1.0]], np.float32)
EXACT_PLANES = [(2, 2), (2, 9), (9, 2), (24, 20)]
EXACT_LINES = [(1, 7), (7, 1)]
P_FAST, P_TWO_PASS, P_MASKED = 10240, 10241, 300
# X, Y, P, mask_oob
EXACT_CASES = ([(X, Y, P, m) for X, Y in EXACT_PLANES for P, m in ((P_FAST, False), (P_TWO_PASS, False), (P_MASKED, True))]
               + [(X, Y, P, m) for X, Y in EXACT_LINES for P, m in ((P_FAST, False), (P_MASKED, True))])


def axis_targets(n):
  """Tap coordinates (cells) along an axis of n cells: both sides of each clamp, the edges, integers."""
  return sorted({-2.0, -0.25, 0.0, 0.25, 1.0, n - 2.0, n - 1.25, n - 1.0, n - 0.75, n + 3.0})


def exact_case(X, Y, P, mask, B=2):
  """theta = 0, cell = 1/4, translations and points multiples of 1/16: every tap coordinate is a multiple of a
  quarter cell, every weight product a multiple of 1/16, every cotangent an integer / 8: all sums exact in f32.
  Pose p of scene 0 takes target p mod T for point 0, so each target sits in every register slot."""
  rng = np.random.default_rng(X * 100003 + Y * 1009 + P + int(mask))
  targets = np.array([(u, v) for u in axis_targets(X) for v in axis_targets(Y)])
  T = len(targets)
  pick = np.stack([np.arange(P) % T, (np.arange(P) * 7 + 3) % T][:B])
  poses = np.zeros((B, P, 3), np.float32)
  poses[..., 1:] = (targets[pick] + 0.5) * CELL_EXACT - EXACT_Q[0]
  g = (rng.integers(-8, 9, (B, P)) / 8.0).astype(np.float32)
  q_xy = np.broadcast_to(EXACT_Q, (B,) + EXACT_Q.shape).copy()
  vq = np.ones((B, len(EXACT_Q)), bool)
  vq[B - 1, 3] = False
  mv = np.ones((B, X, Y), bool)
  if mask:                                           # knock out taps: a corner, an edge cell, an inner cell
    mv[0, 0, 0] = False
    mv[0, X - 1, Y // 2] = False
    mv[B - 1, 0, Y - 1] = False
    mv[B - 1, X // 2, min(1, Y - 1)] = False
  return dict(name=f'exact-{X}x{Y}-P{P}-{"masked" if mask else "plain"}', dscores=g, poses=poses, q_xy=q_xy,
              valid_q=vq, map_valid=mv, shape=(B, len(EXACT_Q), X, Y), cell=CELL_EXACT, mask_oob=mask)


# ----------------------------------------------------------------------------------------------------
# D. the fixed-point scale
# ----------------------------------------------------------------------------------------------------
SCALE_SHAPE = (2, 300, 24, 20)     # two points per chunk
SCALE_P = 2500                     # slots 0..2
POISON_POSE = 2 * PB_THREADS + 17  # slot 2


def scale_case(seed=41):
  B, Nq, X, Y = SCALE_SHAPE
  inp = random_case(('scale', seed, B, Nq, X, Y, SCALE_P, False))
  assert chunking(B, Nq)[0] == 2
  return inp


def dyadic_scale_case(seed=42):
  """Coordinates on a 1/16-cell lattice and cotangents m * 2^4, 1 <= m < 256: every term is a multiple of 2^-4 of
  at most 20 bits, so the result scaled by 2^-120 (terms >= 2^-124) stays normal and exact, as by 2^100."""
  B, Nq, X, Y = SCALE_SHAPE
  rng = np.random.default_rng(seed)
  cell = CELL_EXACT
  poses = np.zeros((B, SCALE_P, 3), np.float32)
  poses[..., 1] = rng.integers(-16 * 5, 16 * (X + 5), (B, SCALE_P)) / 16.0 * cell
  poses[..., 2] = rng.integers(-16 * 5, 16 * (Y + 5), (B, SCALE_P)) / 16.0 * cell
  q_xy = (rng.integers(-64, 65, (B, Nq, 2)) / 16.0 * cell).astype(np.float32)
  g = (rng.integers(1, 256, (B, SCALE_P)) * rng.choice([-16.0, 16.0], (B, SCALE_P))).astype(np.float32)
  return dict(name='scale-dyadic', dscores=g, poses=poses, q_xy=q_xy, valid_q=forced_valid(rng, B, Nq),
              map_valid=None, shape=SCALE_SHAPE, cell=cell, mask_oob=False)


# ----------------------------------------------------------------------------------------------------
# F. the small kernels
# ----------------------------------------------------------------------------------------------------
SMALL_SHAPES = [(1, 1, 1, 1), (2, 5, 3, 7), (3, 37, 13, 21), (2, 130, 40, 24)]     # B, Nq, X, Y
SOFTMAX_BWD_N = (1, 2, 255, 256, 257, 1000, 4652)
SOFTMAX_BWD_MASKS = ('all true', 'all false', 'one true', 'ragged')
SIMILARITY_SHAPES = [(2, 37, 13, 21, 32), (1, 130, 40, 24, 128)]                   # B, Nq, X, Y, Dm


def small_case(shape, seed=51):
  """dsim, sim with planted +0.0, -0.0 and negative entries, coef [B] and row_coef [B, Nq] with a zero entry."""
  B, Nq, X, Y = shape
  rng = np.random.default_rng([seed, B, Nq, X, Y])
  dsim = rng.standard_normal(shape).astype(np.float32)
  sim = rng.standard_normal(shape).astype(np.float32)
  flat = sim.reshape(-1)
  flat[::7] = 0.0
  flat[3::11] = -0.0
  if flat.size == 1:
    flat[0] = 0.75
  coef = rng.uniform(0.5, 2.0, B).astype(np.float32)
  row_coef = rng.uniform(0.5, 2.0, (B, Nq)).astype(np.float32)
  if B > 1:
    coef[B - 1] = 0.0
  if Nq > 1:
    row_coef[0, Nq // 2] = 0.0
  return dsim, sim, coef, row_coef


def _gated(dsim, sim, clip, cf):
  """G: ONE f32 product where the gate is open, +0.0 where it is closed (sim = +-0 closes it)."""
  G = (np.asarray(dsim, np.float32) * np.asarray(cf, np.float32)).astype(np.float32)
  return np.where(sim > 0, G, np.float32(0.0)) if clip else G


def sim_bwd_prepare(dsim, sim, clip, coef):
  """-> G (f32, exact), per-scene sum dsim * sim (float64), its bound m 2^-24 sum |dsim sim|."""
  B = dsim.shape[0]
  G = _gated(dsim, sim, clip, coef.reshape((B,) + (1,) * (dsim.ndim - 1)))
  prod = (f64(dsim) * f64(sim)).reshape(B, -1)
  return G, prod.sum(-1), prod.shape[1] * U * np.abs(prod).sum(-1)


def sim_bwd_prepare_rows(dsim, sim, clip, row_coef):
  """-> G (f32, exact), rowdot [B, Nq] (float64), its bound XY 2^-24 sum |dsim sim| per row."""
  B, Nq, X, Y = dsim.shape
  G = _gated(dsim, sim, clip, row_coef[:, :, None, None])
  prod = (f64(dsim) * f64(sim)).reshape(B, Nq, X * Y)
  return G, prod.sum(-1), X * Y * U * np.abs(prod).sum(-1)


def masked_softmax_rows_bwd(w, dw):
  """dx = w (dw - sum w dw) and its bound |w_i| (N 2^-24 sum |w dw| + 2^-23 (|dw_i| + |dot|))."""
  w, dw = f64(w), f64(dw)
  N = w.shape[-1]
  dot = (w * dw).sum(-1, keepdims=True)
  bound = np.abs(w) * (N * U * np.abs(w * dw).sum(-1, keepdims=True) + 2 * U * (np.abs(dw) + np.abs(dot)))
  return w * (dw - dot), bound


def softmax_bwd_masks(N, kind, B=3, seed=61):
  rng = np.random.default_rng([seed, N])
  if kind == 'all true':
    return np.ones((B, N), bool)
  if kind == 'all false':
    return np.zeros((B, N), bool)
  if kind == 'one true':
    m = np.zeros((B, N), bool)
    m[np.arange(B), [0, N // 2, N - 1][:B]] = True
    return m
  m = rng.random((B, N)) > 0.4
  m[0, N - 1] = True                     # ragged: the last element alone in its segment, a leading gap, a hole
  m[1, :N // 3] = False
  m[1, N - 1] = True
  m[2, N // 4:N // 2] = False
  m[2, 0] = True
  return m
