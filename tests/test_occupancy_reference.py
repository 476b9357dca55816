"""The exact host restatement of occupancy.hip (occupancy_reference.py: fmaf32 / gather_f32 / head_f32)
checked on its own, without a GPU: fmaf32 against exact rational arithmetic, the gather against the
oracle's interpolate_nd and a float64 trilinear interpolation, the head against a float64 MLP, and
the support rule against the library's host function."""
import fractions
import itertools

import numpy as np
import pytest

import occupancy_reference as occ_ref
from oracle import grids as o_grids

f32 = np.float32
F = fractions.Fraction


def _round_f32(a, b, c):
  """fmaf(a, b, c) from exact rational arithmetic, rounded to nearest-even binary32."""
  a, b, c = (float(v) for v in (a, b, c))
  if not all(np.isfinite((a, b, c))):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
  r = F(a) * F(b) + F(c)
  if r == 0:
    prod_zero_neg = a * b == 0 and (np.signbit(a) != np.signbit(b))
    neg = prod_zero_neg and c == 0 and np.signbit(c)
    return f32(-0.0) if neg else f32(0.0)
  sign = -1 if r < 0 else 1
  m = abs(r)
  e = m.numerator.bit_length() - m.denominator.bit_length()
  if F(2) ** e > m:
    e -= 1
  e = max(e, -126)                                             # the subnormal quantum
  q = F(2) ** (e - 23)
  n = m / q
  fl = n.numerator // n.denominator
  rem = n - fl
  if rem > F(1, 2) or (rem == F(1, 2) and fl % 2 == 1):
    fl += 1
  v = fl * q
  if v >= F(2) ** 128:
    return f32(sign * np.inf)
  return f32(sign * float(v))


def _bits(x):
  return np.asarray(x, f32).view(np.uint32)


def _check_fma(a, b, c):
  a, b, c = (np.asarray(v, f32).reshape(-1) for v in (a, b, c))
  got = occ_ref.fmaf32(a, b, c)
  want = np.array([_round_f32(x, y, z) for x, y, z in zip(a, b, c)], f32)
  bad = _bits(got) != _bits(want)
  assert not bad.any(), [(float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want[i]))
                         for i in np.flatnonzero(bad)[:5]]


def test_fmaf32_random_against_exact_arithmetic():
  rng = np.random.default_rng(0)
  n = 4000
  a = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(f32)
  b = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(f32)
  # c: unrelated, or close to -a*b (cancellation: the product's low bits decide the result)
  near = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 2.0 ** -20)).astype(f32)
  c = np.where(rng.random(n) < 0.5, (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(f32), near)
  _check_fma(a, b, c)
  # random bit patterns over the whole finite range (products far into the f64 range)
  u = rng.integers(0, 2 ** 32, (3, n), dtype=np.uint64).astype(np.uint32).view(f32)
  fin = np.isfinite(u).all(0)
  _check_fma(*u[:, fin])


def test_fmaf32_constructed_cases():
  t = f32(1 + 2.0 ** -12)                 # t * t = 1 + 2^-11 + 2^-24: an exact f32 tie (half an ulp of 1)
  tiny = f32(2.0 ** -80)
  cases = [
      (t, t, f32(0)),                      # tie, rounds to even (down)
      (t, t, tiny),                        # tie + tail: up (a float64 sum would round to the tie first)
      (t, t, -tiny),                       # tie - tail: down
      (-t, t, tiny), (-t, t, -tiny),
      (f32(1 + 2.0 ** -12), f32(1 - 2.0 ** -13), f32(2.0 ** -100)),
      (f32(3), f32(5), f32(-15)),          # exact cancellation: +0
      (f32(-3), f32(5), f32(15)),
      (f32(-0.0), f32(1), f32(-0.0)),      # -0 + -0 = -0
      (f32(0), f32(-1), f32(0)),           # -0 + +0 = +0
      (f32(-2), f32(0), f32(-0.0)),
      (f32(0), f32(0), f32(-0.0)),
      (f32(2.0 ** -70), f32(2.0 ** -70), f32(0)),                        # subnormal result
      (f32(1.5 * 2.0 ** -75), f32(1.3 * 2.0 ** -70), f32(0)),
      (f32(1.5 * 2.0 ** -75), f32(1.3 * 2.0 ** -70), f32(-2.0 ** -149)),
      (f32(2.0 ** -75), f32(2.0 ** -75), f32(2.0 ** -149)),              # 1.5 least subnormals: tie, to 2
      (f32(2.0 ** -75), f32(2.0 ** -75), f32(0)),                        # exactly half of one: tie, to 0
      (f32(2.0 ** -75), f32(2.0 ** -74), f32(2.0 ** -149)),
      (f32(1.2e-38), f32(0.9), f32(-1.1e-38)),                           # normal - normal -> subnormal
      (f32(2.0 ** 64), f32(2.0 ** 64), f32(0)),                          # overflow to +inf
      (f32(-3e38), f32(2), f32(1)),                                      # to -inf
      (np.finfo(f32).max, f32(1), np.finfo(f32).max),
      (np.finfo(f32).max, f32(1 + 2.0 ** -23), f32(0)),
      (np.finfo(f32).max, f32(1), f32(2.0 ** 103)),                      # max + exactly half an ulp: inf
      (np.finfo(f32).max, f32(1), f32(2.0 ** 103 * (1 - 2.0 ** -20))),  # just below: max
      (np.finfo(f32).max, f32(-1), f32(-2.0 ** 103)),
  ]
  a, b, c = (np.array(v, f32) for v in zip(*cases))
  _check_fma(a, b, c)
  got = occ_ref.fmaf32(a, b, c)
  assert _bits(got[1]) == _bits(f32(1 + 2.0 ** -11 + 2.0 ** -23))          # the tail decided: up
  assert _bits(got[0]) == _bits(got[2]) == _bits(f32(1 + 2.0 ** -11))
  assert np.signbit(got[8]) and not np.signbit(got[9]) and not np.signbit(got[6])
  assert got[12] == f32(2.0 ** -140) and got[15] == f32(2.0 ** -148) and got[16] == 0
  assert got[19] == np.inf and got[20] == -np.inf and got[23] == np.inf and got[24] == np.finfo(f32).max
  # non-finite operands propagate as IEEE says
  r = occ_ref.fmaf32(np.array([np.inf, 0, np.nan, np.inf], f32), np.array([1, np.inf, 1, 1], f32),
                     np.array([1, 1, 1, -np.inf], f32))
  assert r[0] == np.inf and np.isnan(r[1:]).all()


def _volume(B, X, Y, Z, D, seed, invalid=0.2):
  rng = np.random.default_rng(seed)
  vol = rng.uniform(-1, 1, (B, X, Y, Z, D)).astype(f32)
  valid = rng.random((B, X, Y, Z)) >= invalid
  return vol, valid


def _trilinear_f64(vol, pts):
  """Float64 trilinear interpolation with clamped ('nearest') extension at point / cell (corner origin)."""
  size = np.array(vol.shape[:3])
  c = pts.astype(np.float64) - 0.5
  lo = np.floor(c)
  w1 = c - lo
  lo = lo.astype(np.int64)
  out = 0
  for bits in itertools.product((0, 1), repeat=3):
    w = np.prod([w1[:, t] if b else 1 - w1[:, t] for t, b in enumerate(bits)], 0)
    i = [np.clip(lo[:, t] + b, 0, size[t] - 1) for t, b in enumerate(bits)]
    out = out + w[:, None] * vol[i[0], i[1], i[2]].astype(np.float64)
  return out


@pytest.mark.parametrize('shape', [(2, 9, 7, 5, 6), (1, 1, 4, 1, 3), (2, 5, 1, 6, 1)])
def test_gather_f32_against_oracle_and_f64(shape):
  B, X, Y, Z, D = shape
  cell = 0.2
  vol, valid = _volume(B, X, Y, Z, D, seed=sum(shape), invalid=0.05)
  rng = np.random.default_rng(1)
  pts = (rng.uniform(-0.2, 1.2, (B, 3000, 3)) * np.array([X, Y, Z]) * cell).astype(f32)
  pts[:, :27] = (np.stack(np.meshgrid(*[[0.0, 0.5, s] for s in (X, Y, Z)], indexing='ij'), -1).reshape(-1, 3)
                 * f32(cell)).astype(f32)                       # corners, centres, the far faces
  feats, v = occ_ref.gather_f32(vol, valid, pts, cell)
  feats_nv, v_nv = occ_ref.gather_f32(vol, None, pts, cell)
  np.testing.assert_array_equal(feats, feats_nv)
  rng_v = float(np.abs(vol).max())
  for b in range(B):
    idx = pts[b] / f32(cell)
    f_o, v_o = o_grids.interpolate_nd(vol[b], idx, valid[b])
    np.testing.assert_array_equal(v[b], v_o)
    _, v_o_nv = o_grids.interpolate_nd(vol[b], idx)
    np.testing.assert_array_equal(v_nv[b], v_o_nv)
    assert float(np.abs(feats[b] - f_o).max()) <= 1e-6 * rng_v
    assert float(np.abs(feats[b] - _trilinear_f64(vol[b], idx)).max()) <= 1e-6 * rng_v
  assert 0.1 < v.mean() < 0.9 and v_nv.mean() >= v.mean()


def test_gather_f32_zero_weight_invalid_tap_and_non_finite_points():
  vol, _ = _volume(1, 4, 4, 4, 2, seed=3)
  valid = np.ones((1, 4, 4, 4), bool)
  valid[0, 2, 1, 1] = False
  cell = 0.5
  # p = (1.5, 1.5, 1.5): the voxel centre (1, 1, 1), whi = 0 -- the (2, ., .) taps weigh 0 but invalidate
  pts = np.array([[[0.75, 0.75, 0.75], [0.25, 0.75, 0.75], [np.nan, 0.5, 0.5], [1e30, 0.75, 0.75],
                   [np.inf, 0.5, 0.5], [-0.1, 0.5, 0.5]]], f32)
  feats, v = occ_ref.gather_f32(vol, valid, pts, cell)
  np.testing.assert_array_equal(feats[0, 0], vol[0, 1, 1, 1])
  assert v.tolist() == [[False, True, False, False, False, False]]
  with np.errstate(invalid='ignore'):
    _, v_o = o_grids.interpolate_nd(vol[0], pts[0] / f32(cell), valid[0])
  np.testing.assert_array_equal(v[0], v_o)
  assert np.isnan(feats[0, 2]).all() and np.isnan(feats[0, 4]).all()
  np.testing.assert_array_equal(feats[0, 3], vol[0, 3, 1, 1])   # 1e30: whi = 0, the clamped upper tap


@pytest.mark.parametrize('hidden', [(32,), (64,), (32, 64), (96, 160)])
def test_head_f32_against_f64_mlp(hidden):
  rng = np.random.default_rng(len(hidden) * 100 + hidden[0])
  D, R = 32, 150
  x = rng.uniform(-1, 1, (R, D)).astype(f32)
  mlp, d_in = [], D
  for w in (*hidden, 1):
    lim = (6.0 / (d_in + w)) ** 0.5
    mlp.append((rng.uniform(-lim, lim, (d_in, w)).astype(f32), rng.uniform(-0.1, 0.1, w).astype(f32)))
    d_in = w
  got = occ_ref.head_f32(x, mlp)
  ref = x.astype(np.float64)
  for i, (k, b) in enumerate(mlp):
    ref = ref @ k.astype(np.float64) + b
    if i + 1 < len(mlp):
      ref = np.maximum(ref, 0)
  ref = ref[:, 0]
  assert got.dtype == f32 and got.shape == (R,)
  assert float(np.abs(got - ref).max()) <= 1e-5 * float(np.abs(ref).max())
  assert not np.array_equal(got.astype(np.float64), ref)        # (f32 arithmetic, not a float64 copy)


def test_head_f32_keeps_the_summation_order():
  """The restatement itself is order-sensitive: a reversed tile sum is a different function."""
  rng = np.random.default_rng(5)
  x = rng.uniform(-1, 1, (400, 32)).astype(f32)
  k0, b0 = rng.uniform(-1, 1, (32, 128)).astype(f32), rng.uniform(-0.1, 0.1, 128).astype(f32)
  k1, b1 = rng.uniform(-1, 1, (128, 128)).astype(f32), rng.uniform(-0.1, 0.1, 128).astype(f32)
  wo = rng.uniform(-1, 1, (128, 1)).astype(f32)
  bo = np.array([0.3], f32)
  got = occ_ref.head_f32(x, [(k0, b0), (k1, b1), (wo, bo)])
  h = occ_ref._snap_relu(occ_ref._fmaf_chain(occ_ref._snap_relu(occ_ref._fmaf_chain(x, k0) + b0), k1) + b1)
  parts = [occ_ref._fmaf_chain(h[:, c:c + 32], wo[c:c + 32])[:, 0] for c in range(0, 128, 32)]
  fwd = ((parts[0] + parts[1]) + parts[2]) + parts[3] + bo[0]
  rev = ((parts[3] + parts[2]) + parts[1]) + parts[0] + bo[0]
  np.testing.assert_array_equal(_bits(got), _bits(fwd))
  assert (_bits(got) != _bits(rev)).any()


def test_occupancy_head_supported_matches_the_library():
  """Every pair of (D, h1, h2) over the whole [0, 300]^2 plane, the third argument at the values that
  bound the rule (the full [0, 300]^3 cube is 27 M ctypes calls: ~20 s)."""
  from snap_amd import _lib
  lib = _lib.load()
  ws = range(0, 301)
  edges = (0, 1, 32, 33, 255, 256, 257, 288)      # around 0, the multiples of 32 and the widest
  bad, n_ok = [], 0
  for u in ws:
    for v in ws:
      for e in edges:
        for D, h1, h2 in ((u, v, e), (u, e, v), (e, u, v)):
          want = bool(lib.snap_occupancy_head_supported(D, h1, h2))
          n_ok += want
          if occ_ref.occupancy_head_supported(D, (h1,) if h2 == 0 else (h1, h2)) != want:
            bad.append((D, h1, h2, want))
  assert not bad, bad[:10]
  assert n_ok > 100
