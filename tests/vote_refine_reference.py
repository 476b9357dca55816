"""A float64 numpy restatement of ``snap_plane_align_score_f32`` (include/snap_hip.h) and of the refinement lattice of
``pose_exhaustive_voting.refine_lattice`` / ``refine_poses``, written from the contract, not from the kernel: whole
planes at a time, one pose after the other.

The contract, restated
----------------------
``fq [Hq, Wq, D]`` / ``vq [Hq, Wq]``: the query plane; ``fm [Hm, Wm, D]`` / ``vm [Hm, Wm]``: the map plane;
``poses [P, 4]`` f32 = (cos, sin, tx, ty), translations in cells.

* For a query cell (i, j) the sample position is u = (cos (i + 0.5) - sin (j + 0.5)) + tx, v = (sin (i + 0.5) +
  cos (j + 0.5)) + ty, each operation rounded to f32 (the contract fixes the order and forbids fma, so this is part
  of the definition, not of the error: the floor below must see the same number here and there).
* Inside iff 0 <= u < Hm and 0 <= v < Wm.  cu = fl32(u - 0.5), fu = floor(cu), wu1 = fl32(cu - fu); the tap rows are
  fu and fu + 1 clamped into [0, Hm - 1] with factors (1 - wu1, wu1); columns alike.
* The cell counts iff vq[i, j], inside, and all four taps valid in vm (zero weight or not).
* raw = sum over the counted cells of fq . (bilinear mix of the four fm taps), overlap = the number of counted cells,
  tcount = sum vq, score = raw / tcount if overlap > threshold else -inf.  A non-finite pose row: -inf, overlap 0.
* A non-finite feature among a counted cell's own features or its four taps makes the pose's score NaN here (the
  kernel may also produce +-inf from an Inf feature; the tests use NaN).

Here the factor 1 - wu1, the weights, the products and every sum are float64.

The error bound (``bound``), derived, not measured
--------------------------------------------------
With u = 2^-24, rounding to nearest, gamma_m = m u / (1 - m u) and S(p) = sum over the counted cells and channels of
|fq| * sum_taps weight * |fm tap| (the exact weights), the kernel's f32 score differs from the exact one by at most
(gamma_m + (cells + 2) 2^-53) S / tcount with m = 3 + 4 + 1 + 4 ceil(D / 32) + 3 + 1:

* a weight is the product of two factors, each wu1 (the same f32 number here and there) or 1 - wu1 (one rounding),
  and one multiplication: at most 3 roundings;
* mix = ((w00 m00 + w01 m01) + w10 m10) + w11 m11: a term passes one multiplication and at most three additions: 4;
* the product fq_d * mix_d: 1;
* the channel sum of a cell: lane l of 8 adds its 4 ceil(D / 32) products in one chain (a term passes at most that
  many additions), then a 3-level tree over the lanes: 4 ceil(D / 32) + 3;
* above the cell everything is float64: cells + 2 operations (the sums and the division) of 2^-53 each;
* the final rounding of the quotient to f32: 1.

At D = 32 that is m = 16: 9.5e-7 S / tcount.  (Overflow is outside the bound.)  The tests allow twice the bound.
"""
import math

import numpy as np

U = 2.0 ** -24
F32 = np.float32


def pose_row(quarter_or_deg, tx, ty, exact_quarter=False):
  """One pose row (cos, sin, tx, ty) f32.  ``exact_quarter``: the first argument counts quarter turns and the row
  holds exact (+-1, 0) pairs; otherwise it is an angle in degrees."""
  if exact_quarter:
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][int(quarter_or_deg) % 4]
  else:
    c, s = math.cos(math.radians(quarter_or_deg)), math.sin(math.radians(quarter_or_deg))
  return np.array([c, s, tx, ty], F32)


def _geometry(pose, Hq, Wq, Hm, Wm):
  """The f32 part of the definition for one finite pose row -> dict of [Hq, Wq] arrays."""
  c, s, tx, ty = (F32(x) for x in pose)
  gi = (np.arange(Hq, dtype=F32) + F32(0.5))[:, None]
  gj = (np.arange(Wq, dtype=F32) + F32(0.5))[None, :]
  with np.errstate(all='ignore'):
    u = ((c * gi - s * gj) + tx).astype(F32)
    v = ((s * gi + c * gj) + ty).astype(F32)
    inside = (u >= 0) & (u < Hm) & (v >= 0) & (v < Wm)
    u, v = np.where(inside, u, F32(0.5)), np.where(inside, v, F32(0.5))
    cu, cv = (u - F32(0.5)).astype(F32), (v - F32(0.5)).astype(F32)
    fu, fv = np.floor(cu), np.floor(cv)
    wu1, wv1 = (cu - fu).astype(F32), (cv - fv).astype(F32)
  clamp = lambda x, n: np.clip(x, 0, n - 1).astype(np.int64)
  return dict(inside=inside, i0=clamp(fu, Hm), i1=clamp(fu + 1, Hm), j0=clamp(fv, Wm), j1=clamp(fv + 1, Wm),
              wu1=wu1.astype(np.float64), wv1=wv1.astype(np.float64))


def _walk(fq, vq, fm, vm, poses, want):
  """want: 'score' -> (raw / tcount [P], overlap [P], nan [P]); 'bound' -> S / tcount [P]; 'taps' -> per pose the set
  of map cells (flat indices) that are taps of a counted cell."""
  fq, fm, poses = np.asarray(fq), np.asarray(fm), np.asarray(poses)
  assert fq.dtype == F32 and fm.dtype == F32 and poses.dtype == F32 and poses.ndim == 2 and poses.shape[1] == 4
  vq, vm = np.asarray(vq) != 0, np.asarray(vm) != 0
  Hq, Wq, D = fq.shape
  Hm, Wm = fm.shape[:2]
  tcount = int(vq.sum())
  fq64, fm64 = fq.astype(np.float64), fm.astype(np.float64)
  if want == 'bound':
    fq64, fm64 = np.abs(fq64), np.abs(fm64)
  bad_q = ~np.isfinite(fq).all(-1)
  bad_m = ~np.isfinite(fm).all(-1)
  total = np.zeros(len(poses))
  overlap = np.zeros(len(poses), np.int64)
  nan = np.zeros(len(poses), bool)
  taps = []
  for p, pose in enumerate(poses):
    if not np.isfinite(pose).all():
      taps.append(set())
      continue
    g = _geometry(pose, Hq, Wq, Hm, Wm)
    i0, i1, j0, j1 = g['i0'], g['i1'], g['j0'], g['j1']
    counted = vq & g['inside'] & vm[i0, j0] & vm[i0, j1] & vm[i1, j0] & vm[i1, j1]
    overlap[p] = counted.sum()
    if want == 'taps':
      flat = np.stack([i0 * Wm + j0, i0 * Wm + j1, i1 * Wm + j0, i1 * Wm + j1], -1)[counted]
      taps.append(set(flat.reshape(-1).tolist()))
      continue
    nan[p] = bool((counted & (bad_q | bad_m[i0, j0] | bad_m[i0, j1] | bad_m[i1, j0] | bad_m[i1, j1])).any())
    wu1, wv1 = g['wu1'][..., None], g['wv1'][..., None]
    wu0, wv0 = 1.0 - wu1, 1.0 - wv1
    with np.errstate(invalid='ignore'):
      mix = (wu0 * wv0) * fm64[i0, j0] + (wu0 * wv1) * fm64[i0, j1] + (wu1 * wv0) * fm64[i1, j0] + \
          (wu1 * wv1) * fm64[i1, j1]
      cell = (fq64 * mix).sum(-1)
    total[p] = np.where(counted, cell, 0.0).sum() if not nan[p] else np.nan
  if want == 'taps':
    return taps
  with np.errstate(divide='ignore', invalid='ignore'):
    return total / tcount, overlap, nan


def plane_align_score(fq, vq, fm, vm, poses, threshold):
  """-> (score float64 [P]: the exact value, -inf or NaN; overlap int64 [P])."""
  value, overlap, nan = _walk(fq, vq, fm, vm, poses, 'score')
  keep = (overlap.astype(np.float32) > np.float32(threshold)) & np.isfinite(np.asarray(poses)).all(1)
  return np.where(keep, np.where(nan, np.nan, value), -np.inf), overlap


def bound(fq, vq, fm, vm, poses, threshold):
  """The derived f32 rounding bound per pose (module docstring); 0 where the score is not finite."""
  s_abs, overlap, _ = _walk(fq, vq, fm, vm, poses, 'bound')
  score, _ = plane_align_score(fq, vq, fm, vm, poses, threshold)
  D = np.asarray(fq).shape[-1]
  m = 3 + 4 + 1 + 4 * -(-D // 32) + 3 + 1
  gamma = m * U / (1 - m * U) + (overlap + 2) * 2.0 ** -53
  return np.where(np.isfinite(score), gamma * s_abs, 0.0)


def counted_taps(fq, vq, fm, vm, poses):
  """Per pose, the set of flat map-cell indices that are taps of one of its counted cells."""
  return _walk(fq, vq, fm, vm, poses, 'taps')


# ---------------------------------------------------------------------------------------------------------------
# the lattice
# ---------------------------------------------------------------------------------------------------------------
def index_to_pose(index, extent, num_rotations):
  """Continuous index [..., 3] = (k, a, b), float64 -> pose rows [..., 4] float64 = (cos, sin, tx, ty) of
  ``exhaustive_index_to_tfm`` (corner frames, the +0.5 cell offset), translations in cells: rotation -2 pi k / R,
  t = centre + (a - H + 1.5, b - W + 1.5) - Rot centre, centre = extent / 2."""
  index = np.asarray(index, np.float64)
  H, W = extent
  th = -2 * np.pi * index[..., 0] / num_rotations
  c, s = np.cos(th), np.sin(th)
  cx, cy = H / 2, W / 2
  tx = cx + (index[..., 1] - H + 1.5) - (c * cx - s * cy)
  ty = cy + (index[..., 2] - W + 1.5) - (s * cx + c * cy)
  return np.stack([c, s, tx, ty], -1)


def refine_lattice(index, extent, num_rotations, steps_r=11, range_r=0.5, steps_xy=9, range_xy=1.0):
  """float64, unrounded: index int [K, 3] -> (continuous indices [K, L, 3], poses [K * L, 4]); rotation slowest, then
  a, then b; NaN rows for a -1 peak."""
  index = np.asarray(index)
  K = index.shape[0]
  dk = np.linspace(-range_r, range_r, steps_r)
  dxy = np.linspace(-range_xy, range_xy, steps_xy)
  off = np.stack(np.meshgrid(dk, dxy, dxy, indexing='ij'), -1).reshape(-1, 3)
  cont = index[:, None, :].astype(np.float64) + off[None]
  cont[index[:, 0] < 0] = np.nan
  return cont, index_to_pose(cont, extent, num_rotations).reshape(K * len(off), 4)


def refine_poses(fq, vq, fm, vm, index, extent, num_rotations, cell_size, min_overlap=0.05, **lattice):
  """The reference refinement: per peak the first maximum of the reference scores over the lattice (an all -inf row:
  lattice index 0) -> dict(index [K, 3], score [K], overlap [K], angle [K], t [K, 2] in metres, lattice_scores
  [K, L], best [K])."""
  cont, poses = refine_lattice(index, extent, num_rotations, **lattice)
  K, L = cont.shape[:2]
  Hq, Wq = np.asarray(fq).shape[:2]
  score, overlap = plane_align_score(fq, vq, fm, vm, poses.astype(F32), min_overlap * Hq * Wq)
  score, overlap = score.reshape(K, L), overlap.reshape(K, L)
  best = np.array([int(np.argmax(row)) for row in score])
  rows = np.arange(K)
  pick = poses.reshape(K, L, 4)[rows, best]
  return dict(index=cont[rows, best], score=score[rows, best], overlap=overlap[rows, best],
              angle=-2 * np.pi * cont[rows, best, 0] / num_rotations, t=pick[:, 2:] * cell_size,
              lattice_scores=score, best=best)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def exact_case():
  """8 x 8 planes, all 64 query cells valid (the normaliser is a power of two), integer features in [-3, 3], quarter
  turns as exact (+-1, 0) pairs, integer translations that keep some cells inside: weights 0 / 1, every product and
  sum exact."""
  rng = np.random.default_rng(7)
  fq = rng.integers(-3, 4, (8, 8, 8)).astype(F32)
  fm = rng.integers(-3, 4, (8, 8, 8)).astype(F32)
  vq = np.ones((8, 8), bool)
  vm = np.ones((8, 8), bool)
  vm[5, 2] = False
  # a quarter turn about the corner maps the plane next to itself: tx / ty bring it back
  poses = np.stack([pose_row(0, 0, 0, True), pose_row(0, 2, -3, True), pose_row(1, 8, 0, True),
                    pose_row(1, 6, 1, True), pose_row(2, 8, 8, True), pose_row(2, 9, 5, True),
                    pose_row(3, 0, 8, True), pose_row(3, -2, 7, True)])
  return fq, vq, fm, vm, poses, 0.0


def _masks_case(rng):
  Hq = Wq = Hm = Wm = 12
  D = 8
  fq = rng.standard_normal((Hq, Wq, D)).astype(F32)
  fm = rng.standard_normal((Hm, Wm, D)).astype(F32)
  vq = rng.random((Hq, Wq)) > 0.15
  vm = rng.random((Hm, Wm)) > 0.10
  # map cell (7, 6) invalid and, under the integer-aligned pose (identity, t = (2, 1)), its full-weight query cell
  # (5, 5) invalid too: for that pose it is only ever a zero-weight tap: the row tap of query (4, 5), the column tap of
  # (5, 4) and the corner tap of (4, 4), whose other taps are all valid
  vm[6:9, 5:8] = True
  vm[7, 6] = False
  vq[5, 5] = False
  vq[4, 5] = vq[5, 4] = vq[4, 4] = True
  cand = [pose_row(0, 2, 1, True)]
  for tx in np.arange(-4, 5):
    for ty in (-3.0, 0.0, 2.0):
      cand.append(pose_row(0, tx, ty, True))
      cand.append(pose_row(7.0, tx + 0.3, ty - 0.45))
  cand = np.stack(cand)
  _, ov, _ = _walk(fq, vq, fm, vm, cand, 'score')
  pairs = [(i, j) for i in range(len(cand)) for j in range(len(cand)) if ov[j] == ov[i] + 1 and ov[i] > 0]
  assert pairs, 'masks: no two candidate poses with overlaps T and T + 1'
  at, above = pairs[0]
  poses = np.stack([cand[0], cand[at], cand[above], pose_row(33.0, 1.25, 4.5), pose_row(180, 11.5, 12.25),
                    pose_row(-90, 0.5, 11.75)])
  return fq, vq, fm, vm, poses, float(ov[at])


def all_inputs():
  """-> list of (name, fq, vq, fm, vm, poses, threshold); seeded, so the same arrays in every process."""
  rng = np.random.default_rng(20261019)
  cases = []

  def planes(hq, wq, hm, wm, D):
    return (rng.standard_normal((hq, wq, D)).astype(F32), np.ones((hq, wq), bool),
            rng.standard_normal((hm, wm, D)).astype(F32), np.ones((hm, wm), bool))

  # the smallest extents: a single query cell in a 3 x 3 map, on a centre, between four, in the clamped border
  fq, vq, fm, vm = planes(1, 1, 3, 3, 4)
  cases.append(('tiny', fq, vq, fm, vm, np.stack([pose_row(0, 1, 1, True), pose_row(30, 1.2, 0.9),
                                                   pose_row(0, -0.4, 2.3, True)]), 0.0))
  # non-square, D no power of two: identity, a pure translation, an exact quarter turn, two general poses
  fq, vq, fm, vm = planes(5, 7, 9, 6, 12)
  cases.append(('ragged', fq, vq, fm, vm, np.stack([
      pose_row(0, 0, 0, True), pose_row(0, 2.5, -1.25, True), pose_row(1, 7, 0, True), pose_row(17, 3.1, 0.2),
      pose_row(-140, 6.0, 5.5)]), 1.0))
  # more than one tile per axis, ragged last tiles; 7 yaws x 10 translations (70: no multiple of 16, 32 or 64)
  fq, vq, fm, vm = planes(33, 17, 40, 40, 32)
  vq[rng.random(vq.shape) < 0.1] = False
  vm[rng.random(vm.shape) < 0.05] = False
  poses = [pose_row(yaw, 3 + 1.37 * n + (20 if yaw > 90 else 0), 11.5 - 0.81 * n + (25 if 90 < yaw < 250 else 0))
           for yaw in (0.0, 3.5, -8.0, 45.0, 91.0, 180.0, 200.5) for n in range(10)]
  cases.append(('tiles', fq, vq, fm, vm, np.stack(poses), 0.05 * 33 * 17))
  # most cells fall outside the map
  fq, vq, fm, vm = planes(20, 20, 6, 6, 8)
  cases.append(('small_map', fq, vq, fm, vm, np.stack([
      pose_row(0, -7, -7, True), pose_row(12, -9.3, -4.1), pose_row(0, -16.5, 3.0, True), pose_row(77, 10.2, -8.8),
      pose_row(0, 5.5, 5.5, True)]), 0.0))
  cases.append(('masks',) + _masks_case(rng))
  # every pose beyond the map
  fq, vq, fm, vm = planes(6, 6, 8, 8, 4)
  cases.append(('outside', fq, vq, fm, vm, np.stack([
      pose_row(0, 8, 0, True), pose_row(0, 0, -6, True), pose_row(45, 100.0, 3.0), pose_row(0, 1e30, 0, True),
      pose_row(10, -3e9, 2.5e9), np.array([3e38, 3e38, 3e38, -3e38], F32)]), 0.0))
  # a NaN row and an Inf row among finite ones (a negative threshold: only the rule for such rows masks them)
  poses = np.stack([pose_row(0, 1, 1, True), pose_row(5, 1.5, 0.5), pose_row(0, 0.25, 1.75, True),
                    pose_row(-3, 1, 1), pose_row(0, 0, 0, True)])
  poses[1, 2] = np.nan
  poses[3, 0] = np.inf
  cases.append(('nonfinite_pose', fq, vq, fm, vm, poses, -1.0))
  # the largest channel count
  fq, vq, fm, vm = planes(16, 16, 18, 15, 128)
  cases.append(('wide', fq, vq, fm, vm, np.stack([pose_row(0, 1, 0, True), pose_row(21, 4.2, -2.6),
                                                   pose_row(-77.7, 0.3, 14.1), pose_row(182, 16.5, 15.0)]), 3.0))
  return cases


def _field(x, y, D=4):
  """The analytic band-limited field of the planted-pose case at cell-unit positions (x, y) -> [..., D]: three
  sinusoids per channel, wavelengths >= 6 cells."""
  rng = np.random.default_rng(99)
  out = []
  for _ in range(D):
    acc = 0.0
    for _ in range(3):
      lam = rng.uniform(6.0, 14.0)
      ang = rng.uniform(0, 2 * np.pi)
      ph = rng.uniform(0, 2 * np.pi)
      kx, ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)
      acc = acc + rng.uniform(0.5, 1.0) * np.sin(kx * x + ky * y + ph)
    out.append(acc)
  return np.stack(out, -1)


def planted_case(H=24, D=4, R=36, cell_size=0.25):
  """Map plane = the field at the map's cell centres; query plane = the same field seen from a known pose, off the
  vote lattice by (0.3 bin, 0.4 cell, -0.3 cell) -> dict(fq, vq, fm, vm, extent, R, cell_size, index_true [3],
  pose_true [4] float64 (cells), angle_true, t_true (metres))."""
  index_true = np.array([2 + 0.3, (H - 1) + 2 + 0.4, (H - 1) - 1 - 0.3])
  pose = index_to_pose(index_true, (H, H), R)
  c, s, tx, ty = pose
  g = np.arange(H) + 0.5
  gi, gj = np.meshgrid(g, g, indexing='ij')
  fm = _field(gi, gj, D).astype(F32)
  fq = _field(c * gi - s * gj + tx, s * gi + c * gj + ty, D).astype(F32)
  ones = np.ones((H, H), bool)
  return dict(fq=fq, vq=ones, fm=fm, vm=ones.copy(), extent=(H, H), R=R, cell_size=cell_size, index_true=index_true,
              pose_true=pose, angle_true=-2 * np.pi * index_true[0] / R, t_true=pose[2:] * cell_size)
