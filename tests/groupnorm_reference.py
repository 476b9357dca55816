"""GroupNorm statistics: float64 definition, float32 restatements of the routes that produce them,
one acceptance rule and the inputs `test_groupnorm_reference.py` (CPU) and
`test_gpu_groupnorm_stats.py` (GPU) share.

Every function takes values ``v [N, HW, C]`` (or ``[N, H, W, C]``) as a float32 numpy array; a
group is ``C / groups`` neighbouring channels of one image.  The statistics of ``relu_first`` are
those of ``relu(v)``.  All return ``(mean, rstd)`` per (image, group) except ``stats64``.
"""
import numpy as np

GROUPS = 32
EPS = 1e-5
# offset of a group in units of its standard deviation; the list cycles over the groups and shifts by
# one group per image, so every launch sees every ratio
RATIOS = (0, 1, 4, 16, 64, 256, -16, -256)
CONSTANTS = (0.5, 3.1, 100.3)
# the hazard ratio of gn_finalize_tiled_kernel (encoder_ops.hip: kGnHazard)
HAZARD_K = 4.0


def _nhwc(v):
  v = np.asarray(v)
  if v.ndim == 4:
    v = v.reshape(v.shape[0], -1, v.shape[3])
  return v


def _grouped(v, groups, relu_first, dtype):
  v = _nhwc(v).astype(dtype)
  if relu_first:
    v = np.maximum(v, 0)
  N, HW, C = v.shape
  return v.reshape(N, HW, groups, C // groups)


def stats64(v, groups=GROUPS, eps=EPS, relu_first=False):
  """The definition (resnet.py:38-40) in float64, two passes -> dict of [N, groups] arrays:
  mean, var, rstd and maxabs (max abs(v) over the group, the scale of the rule's absolute term)."""
  g = _grouped(v, groups, relu_first, np.float64)
  mean = g.mean(axis=(1, 3))
  var = ((g - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
  return dict(mean=mean, var=var, rstd=1.0 / np.sqrt(var + eps), maxabs=np.abs(g).max(axis=(1, 3)), eps=eps)


def two_pass_f32(v, groups=GROUPS, eps=EPS, relu_first=False):
  """The reference's rule in float32: mean, then mean((x - mean)^2)."""
  g = _grouped(v, groups, relu_first, np.float32)
  N, HW = g.shape[:2]
  g = np.ascontiguousarray(g.transpose(0, 2, 1, 3)).reshape(N, groups, -1)     # (numpy sums a contiguous axis pairwise)
  mean = g.mean(axis=2, dtype=np.float32)
  var = ((g - mean[:, :, None]) ** 2).mean(axis=2, dtype=np.float32)
  return mean, (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)


def _finish(mean64, var64, eps):
  """The last lines of both finalize kernels: f32 mean, f32 var, clamp, 1 / sqrtf(var + eps)."""
  var = np.maximum(var64.astype(np.float32), np.float32(0))
  return mean64.astype(np.float32), (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)


def gn_plan(N, HW, C):
  """Slabs per image and pixels per slab of the stand-alone pass (encoder_ops.hip: gn_plan)."""
  chunks = (C + 1023) // 1024
  S = (1024 + N * chunks - 1) // (N * chunks)
  S = max(1, min(S, (HW + 7) // 8, 256))
  ppb = (HW + S - 1) // S
  return (HW + ppb - 1) // ppb, ppb


def pivot_first_sample_f32(v, groups=GROUPS, eps=EPS, relu_first=False):
  """gn_partial_kernel + gn_finalize_kernel: f32 sums of (v - p) and (v - p)^2 around the per-channel
  pivot p = v[pixel 0] per slab -- PW pixel lanes, each a sequential sum, then the lanes in order --
  combined over slabs and channels in float64."""
  v = _nhwc(v).astype(np.float32)
  if relu_first:
    v = np.maximum(v, np.float32(0))
  N, HW, C = v.shape
  cpg = C // groups
  S, ppb = gn_plan(N, HW, C)
  PW = 256 // (min(C, 1024) // 4)
  piv = v[:, 0, :]
  a1 = np.zeros((N, S, C), np.float32)
  a2 = np.zeros((N, S, C), np.float32)
  for s in range(S):
    blk = v[:, s * ppb:min((s + 1) * ppb, HW), :] - piv[:, None, :]
    steps = (blk.shape[1] + PW - 1) // PW
    pad = np.zeros((N, steps * PW - blk.shape[1], C), np.float32)
    blk = np.concatenate([blk, pad], axis=1).reshape(N, steps, PW, C)
    s1 = np.zeros((N, PW, C), np.float32)
    s2 = np.zeros((N, PW, C), np.float32)
    for k in range(steps):
      s1 += blk[:, k]
      s2 += blk[:, k] * blk[:, k]
    for pp in range(PW):
      a1[:, s] += s1[:, pp]
      a2[:, s] += s2[:, pp]
  a1, a2, p = a1.astype(np.float64), a2.astype(np.float64), piv.astype(np.float64)
  grp = lambda t: t.reshape(N, groups, cpg).sum(axis=2)
  t1, t2, u = grp(a1.sum(axis=1)), grp(a2.sum(axis=1)), grp((a1 * p[:, None, :]).sum(axis=1))
  p1, p2 = grp(p), grp(p * p)
  mean = (t1 + HW * p1) / (HW * cpg)
  m2 = t2 - 2 * mean * t1 + 2 * u + HW * (cpg * mean * mean - 2 * mean * p1 + p2)
  return _finish(mean, m2 / (HW * cpg), eps)


def tile_sums_f32(v, tile_rows, tree=False):
  """What a conv epilogue emits: plain f32 sums of v and v^2 (pivot 0) per channel and row tile of
  `tile_rows` rows of the flattened [N * HW] row space (a tile that straddles two images keeps one sum
  per image) -> float64 totals T1, T2 [N, C] of the f32 tile sums.  The rows of a tile are added in
  sequence, or with `tree` pairwise (neighbours first; `tile_rows` a power of two): the two extremes of
  the orders an epilogue may use."""
  N, HW, C = v.shape
  rows = v.reshape(N * HW, C)
  T = (N * HW + tile_rows - 1) // tile_rows
  pad = np.zeros((T * tile_rows - N * HW, C), np.float32)
  rows = np.concatenate([rows, pad]).reshape(T, tile_rows, C)
  img = np.minimum(np.arange(T * tile_rows) // HW, N - 1).reshape(T, tile_rows)
  second = img != img[:, :1]                     # (HW >= tile_rows: a tile touches at most two images)
  acc = np.zeros((2, 2, T, C), np.float32)       # [image slot][sum | sum of squares]
  for slot in (0, 1) if tree else ():
    m = (second == bool(slot))[:, :, None]
    a, b = np.where(m, rows, np.float32(0)), np.where(m, rows * rows, np.float32(0))     # (adding a 0 is exact)
    while a.shape[1] > 1:
      a, b = a[:, 0::2] + a[:, 1::2], b[:, 0::2] + b[:, 1::2]
    acc[slot, 0], acc[slot, 1] = a[:, 0], b[:, 0]
  for r in range(0 if tree else tile_rows):
    x = rows[:, r]
    for slot in (0, 1):
      m = (second[:, r] == bool(slot))[:, None]
      acc[slot, 0] += np.where(m, x, np.float32(0))
      acc[slot, 1] += np.where(m, x * x, np.float32(0))
  T1 = np.zeros((N, C)); T2 = np.zeros((N, C))
  first = img[:, 0]
  last = img[:, -1]
  np.add.at(T1, first, acc[0, 0].astype(np.float64)); np.add.at(T2, first, acc[0, 1].astype(np.float64))
  np.add.at(T1, last, acc[1, 0].astype(np.float64)); np.add.at(T2, last, acc[1, 1].astype(np.float64))
  return T1, T2


def plain_tile_sums_f32(v, tile_rows, groups=GROUPS, eps=EPS, relu_first=False, hazard_k=None, tree=False):
  """The conv epilogues' sums through gn_finalize_tiled_kernel's float64 combination
  var = (T2 - 2 mean T1 + n mean^2) / n.  hazard_k = None: that alone (the kernel before its repair:
  the MUTANT of the CPU file).  hazard_k = k: groups with mean^2 > k var are re-reduced around the
  float64 mean, as the kernel does."""
  v = _nhwc(v).astype(np.float32)
  if relu_first:
    v = np.maximum(v, np.float32(0))
  N, HW, C = v.shape
  assert HW >= tile_rows
  cpg = C // groups
  T1, T2 = tile_sums_f32(v, tile_rows, tree)
  t1 = T1.reshape(N, groups, cpg).sum(axis=2)
  t2 = T2.reshape(N, groups, cpg).sum(axis=2)
  n = HW * cpg
  mean = t1 / n
  m2 = t2 - 2 * mean * t1 + n * mean * mean
  hazard = np.zeros((N, groups), bool)
  if hazard_k is not None:
    with np.errstate(invalid='ignore'):
      hazard = mean * mean > hazard_k * (m2 / n)
    d = v.reshape(N, HW, groups, cpg).astype(np.float64) - mean[:, None, :, None]
    d1, d2 = d.sum(axis=(1, 3)), (d * d).sum(axis=(1, 3))
    mean = np.where(hazard, mean + d1 / n, mean)
    m2 = np.where(hazard, d2 - d1 * d1 / n, m2)
  out = _finish(mean, m2 / n, eps)
  return (*out, hazard) if hazard_k is not None else out


# ---------------------------------------------------------------------------------------------------
# the acceptance rule (from float64 alone)
# ---------------------------------------------------------------------------------------------------
def shares(mean, rstd, ref):
  """(mean, rstd) [N, groups] against ``stats64`` -> the error of each as a share of its tolerance
  (<= 1 passes):
    mean      abs(mu - mean64) <= 2e-6 + 2e-6 abs(mean64)
    variance  V = 1 / rstd^2 in float64:  abs(V - (var64 + eps)) <= 1e-5 (var64 + eps) + 64 (2^-24 max abs(v))^2"""
  mean = np.asarray(mean, np.float64)
  rstd = np.asarray(rstd, np.float64)
  with np.errstate(divide='ignore', invalid='ignore'):
    m_share = np.abs(mean - ref['mean']) / (2e-6 + 2e-6 * np.abs(ref['mean']))
    want = ref['var'] + ref['eps']
    v_share = np.abs(1.0 / (rstd * rstd) - want) / (1e-5 * want + 64.0 * (2.0 ** -24 * ref['maxabs']) ** 2)
  m_share = np.where(np.isfinite(m_share), m_share, np.inf)
  v_share = np.where(np.isfinite(v_share), v_share, np.inf)
  return m_share, v_share


def per_group(t, groups=GROUPS):
  """[N, C] -> [N, groups], asserting that the channels of a group carry one value."""
  t = np.asarray(t)
  N, C = t.shape
  g = t.reshape(N, groups, C // groups)
  assert (g == g[:, :, :1]).all(), 'channels of one group differ'
  return g[:, :, 0]


def scale_share(sc, rstd, gamma):
  """sc [N, C] against rstd [N, C] * gamma [C]: one f32 rounding, i.e. within 2^-24 of the float64
  product (share of that; <= 1 passes)."""
  want = np.asarray(rstd, np.float64) * np.asarray(gamma, np.float64)[None, :]
  with np.errstate(divide='ignore', invalid='ignore'):
    s = np.abs(np.asarray(sc, np.float64) - want) / (2.0 ** -24 * np.abs(want) + 1e-45)
  return np.where(np.isfinite(s), s, np.inf)


# ---------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------
class Planted:
  """Where `offset_field` planted its fixed cases: {name: (image, group)}."""

  def __init__(self, N, relu_first):
    self.where = {f'const {c}': (0, 5 + 8 * i) for i, c in enumerate(CONSTANTS)}
    self.where['last bits'] = (0, 29)
    if relu_first:
      self.where['all negative'] = (N - 1, 2)
      self.where['straddles 0'] = (N - 1, 10)
    # groups whose weight columns the GPU file zeroes, so that y == the residual there on every engine
    self.exact_groups = sorted({g for k, (_, g) in self.where.items() if k.startswith(('const', 'last'))})


def ratio_of(n, g):
  return RATIOS[(g + n) % len(RATIOS)]


def offset_field(N, HW, C, seed, std=1.0, relu_first=False, groups=GROUPS):
  """-> (field [N, HW, C] float32, Planted).  Unit-variance noise plus, per (image, group), the offset
  ``ratio_of(n, g) * std`` (`std`: the standard deviation the group will have once the caller has added
  what it adds -- the conv's own output), with the planted cases in their fixed groups:
  exactly constant groups (0.5, 3.1, 100.3), a group of 100 + j ulp(100), j = 0..7 (values that differ
  only in their last three mantissa bits) and, for relu_first, a group that is negative throughout and
  one around -1 that straddles 0."""
  rng = np.random.default_rng(seed)
  cpg = C // groups
  f = rng.standard_normal((N, HW, groups, cpg)).astype(np.float32)
  off = np.array([[ratio_of(n, g) * std for g in range(groups)] for n in range(N)], np.float32)
  f = f + off[:, None, :, None]
  pl = Planted(N, relu_first)
  for c in CONSTANTS:
    n, g = pl.where[f'const {c}']
    f[n, :, g, :] = np.float32(c)
  n, g = pl.where['last bits']
  f[n, :, g, :] = np.float32(100) + rng.integers(0, 8, (HW, cpg)).astype(np.float32) * np.float32(2.0 ** -17)
  if relu_first:
    n, g = pl.where['all negative']
    f[n, :, g, :] = -np.float32(40) - np.abs(f[n, :, g, :] - off[n, g])
    n, g = pl.where['straddles 0']
    f[n, :, g, :] = f[n, :, g, :] - off[n, g] - np.float32(1)
  return f.reshape(N, HW, C), pl


CONV_STD = 0.25      # standard deviation of what the conv adds to the field (both files)
GROUP_STD = float(np.sqrt(1 + CONV_STD ** 2))


def values(N, HW, C, seed, relu_first=False):
  """The CPU file's stand-in for a conv output on `offset_field`: the field plus noise of CONV_STD
  outside the exact groups."""
  f, pl = offset_field(N, HW, C, seed, GROUP_STD, relu_first)
  cpg = C // GROUPS
  add = (np.random.default_rng(seed + 1).standard_normal((N, HW, GROUPS, cpg)) * CONV_STD).astype(np.float32)
  add[:, :, pl.exact_groups, :] = 0
  return (f.reshape(N, HW, GROUPS, cpg) + add).reshape(N, HW, C), pl


# (N, HW, C) of every case of the GPU file (its conv outputs), and the slab rows its producers emit
SHAPES = [
    (2, 34 * 34, 64), (5, 256, 256), (40, 144, 256), (7, 99, 256), (3, 33 * 40, 256),
    (3, 17 * 19, 512), (5, 63, 256), (3, 20 * 23, 256), (5, 16 * 17, 512), (3, 23 * 17, 1024),
    (3, 31 * 29, 256), (2, 9 * 91, 64), (3, 11 * 85, 64), (4, 13 * 13, 128), (3, 17 * 19, 128),
    (2, 40 * 37, 32), (2, 40 * 37, 64), (3, 8 * 9, 1024), (2, 8 * 9, 2048),
]
TILE_ROWS = (32, 64, 128, 256)      # 256: the pre-split engine's largest row tile
