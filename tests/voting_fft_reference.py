"""Test infrastructure: the float64 reference of the frequency-domain voting (``snap_amd/csrc/voting_fft.hip``,
``voting_fft_body.h``), its error bound, an f32 model of the transforms, and the case table that
tests/test_voting_fft_reference.py (CPU) and tests/test_gpu_voting_fft.py (GPU) share.  numpy / scipy only; nothing in
``snap_amd/`` imports it.

    scores[r, a, b] = sum_{i,j,d} q[r,i,j,d] m_pad[a+i, b+j, d] / tcount[r]         (m_pad: edge padded by Hm-1, Wm-1)
    count[r, a, b]  = sum_{i,j} q_valid[r, H-1-i, W-1-j] mv_pad[a+i, b+j]           (mv_pad: ZERO padded; the
                      reference passes q_valid un-flipped to a true convolution: the 180-degree rotated mask)
    finite where count > f32(threshold), threshold = min_overlap * H * W formed in double  (``finite_rule``)

* ``template_matching_fft64`` (tests/fft_reference.py, unchanged), ``scores64`` (the same correlation, un-masked),
  ``direct64`` / ``counts_direct`` (sliding windows: the small-size checker of both), ``counts64`` (integers).
* ``bound``: an FFT correlation's error is bounded by global norms, not per cell:
      bound[r] = 2^-24 x log2(N1 N2) x sum_p norm2(z_q[r, p]) x norm2(z_m_pad[p]) / tcount[r]
  with p over the channel pairs (2p, 2p+1) the kernel packs as one complex signal.
* ``model32``: the kernel's transforms in f32 -- the stages of tools/fft_voting_model.py (decimation in frequency
  forward, its conjugate transpose back, digit-reversed spectra), every product and sum rounded to f32 as
  ``bfly4`` / ``bfly3`` / ``cmul`` / ``cmulc`` round them, twiddles rounded from double as ``twiddle_body`` does.
* ``MARGIN``: the smallest power of two such that ``model32`` stays within 0.5 x MARGIN x bound of float64 on every
  GPU input of the case table (measured on the CPU, tests/test_voting_fft_reference.py::test_margin; never against
  the kernel).  The GPU tests allow MARGIN x bound.
"""
import functools
import math

import numpy as np
import scipy.fft

from fft_reference import template_matching_fft64   # noqa: F401  (kept as it is; re-exported)

EPS = 2.0 ** -24
MARGIN = 1.0                    # measured: the model's worst error is 0.256 x bound (10 + noise at N = 64 x 16)
K_COLS = 8                      # channel pairs per group (vfft::kCols)
SIZES = (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
GPU_SIZES = SIZES[3:]
HM_MAX = {16: 6, 24: 8, 32: 11, 48: 16, 64: 22, 96: 32, 128: 43, 192: 64, 256: 86, 384: 128, 512: 171, 768: 256,
          1024: 342}


# ------------------------------------------- the plan, restated ------------------------------------------------------
def fft_size(n):
  """Smallest N >= n of the form 2^a or 3 * 2^a (a >= 2)."""
  return min(N for N in SIZES + (1536, 2048) if N >= n)


def radices(N):
  out, n = [], N
  if n % 3 == 0:
    out.append(3); n //= 3
  k = int(round(math.log2(n)))
  assert 1 << k == n, N
  return out + [2] * (k % 2) + [4] * (k // 2)


def plan_string(N):
  """'3|2|4,4|4': the passes over LDS; two consecutive radix-4 stages run fused (``fft_lds``)."""
  rs, out, i = radices(N), [], 0
  while i < len(rs):
    if rs[i] == 4 and i + 1 < len(rs) and rs[i + 1] == 4:
      out.append('4,4'); i += 2
    else:
      out.append(str(rs[i])); i += 1
  return '|'.join(out)


def geometry(H, W, Hm, Wm):
  Hp, Wp = 3 * Hm - 2, 3 * Wm - 2
  return dict(Hp=Hp, Wp=Wp, Ho=Hp - H + 1, Wo=Wp - W + 1, N1=fft_size(Hp), N2=fft_size(Wp))


def smallest_map(N):
  """The smallest map side whose padded length 3 Hm - 2 needs N transform points."""
  Hm = 1
  while fft_size(3 * Hm - 2) < N:
    Hm += 1
  assert fft_size(3 * Hm - 2) == N
  return Hm


# ------------------------------------------- float64 references ------------------------------------------------------
def _pad_edge(m):
  Hm, Wm = m.shape[:2]
  return np.pad(np.asarray(m, np.float64), ((Hm - 1,) * 2, (Wm - 1,) * 2) + ((0, 0),) * (m.ndim - 2), mode='edge')


def _pad_zero(mv):
  Hm, Wm = mv.shape
  return np.pad(np.asarray(mv, np.float64), ((Hm - 1,) * 2, (Wm - 1,) * 2), mode='constant')


def _corr64(q, m_pad):
  """sum_{i,j,d} q[r,i,j,d] m_pad[a+i,b+j,d] by float64 FFTs -> [R, Ho, Wo]."""
  R, H, W = q.shape[:3]
  P0, P1 = m_pad.shape[:2]
  F0, F1 = scipy.fft.next_fast_len(P0, real=True), scipy.fft.next_fast_len(P1, real=True)
  Fm = scipy.fft.rfft2(m_pad, s=(F0, F1), axes=(0, 1))
  out = np.empty((R, P0 - H + 1, P1 - W + 1), np.float64)
  for r in range(R):
    Fq = scipy.fft.rfft2(np.asarray(q[r], np.float64), s=(F0, F1), axes=(0, 1))
    out[r] = scipy.fft.irfft2((np.conj(Fq) * Fm).sum(-1), s=(F0, F1), axes=(0, 1))[:P0 - H + 1, :P1 - W + 1]
  return out


def raw64(q, m, pad='edge'):
  m_pad = _pad_edge(m) if pad == 'edge' else np.stack([_pad_zero(m[..., d]) for d in range(m.shape[-1])], -1)
  return _corr64(q, m_pad)


def counts64(q_valid, m_valid, flip=True):
  """Integer overlap counts [R, Ho, Wo] (float64 FFT, error ~1e-10, rounded).  flip=False is a mutant."""
  qv = np.asarray(q_valid, np.float64)
  qv = qv[:, ::-1, ::-1] if flip else qv
  c = _corr64(qv[..., None], _pad_zero(m_valid)[..., None])
  n = np.rint(c)
  assert np.abs(c - n).max() < 1e-6
  return n.astype(np.int64)


def counts_direct(q_valid, m_valid):
  """The same integers by a sliding window (small sizes)."""
  H, W = q_valid.shape[1:]
  win = np.lib.stride_tricks.sliding_window_view(_pad_zero(m_valid).astype(np.int64), (H, W))
  return np.einsum('abij,rij->rab', win, np.asarray(q_valid, np.int64)[:, ::-1, ::-1])


def counts_all_valid(H, W, Hm, Wm):
  """Closed form with all-valid masks: the area of the overlap rectangle, [Ho, Wo]."""
  def ov(L, Lm):
    a = np.arange(3 * Lm - 1 - L)
    return np.clip(np.minimum(a + L - 1, 2 * Lm - 2) - np.maximum(a, Lm - 1) + 1, 0, None)
  return np.outer(ov(H, Hm), ov(W, Wm)).astype(np.int64)


def threshold(min_overlap, H, W):
  """The reference's threshold: the product in (Python) double, compared as f32."""
  return np.float32(min_overlap * H * W)


def threshold_f32_chain(min_overlap, H, W):
  """A mutant: min_overlap rounded to f32 first, the products formed in f32."""
  return np.float32(min_overlap) * np.float32(H) * np.float32(W)


def finite_rule(counts, thr):
  return counts > np.float32(thr)


def scores64(q, q_valid, m, m_valid=None, min_overlap=None, thr=None, tcount=None):
  """float64 scores.  thr (an explicit threshold) wins over min_overlap; neither: no overlap test."""
  R, H, W = q.shape[:3]
  s = raw64(q, m)
  if thr is None and min_overlap is not None:
    thr = threshold(min_overlap, H, W)
  if thr is not None:
    s = np.where(finite_rule(counts64(q_valid, m_valid), thr), s, -np.inf)
  tc = np.asarray(q_valid, np.float64).sum((-1, -2)) if tcount is None else np.asarray(tcount, np.float64)
  with np.errstate(divide='ignore', invalid='ignore'):
    return s / tc[:, None, None]


def direct64(q, q_valid, m, m_valid, min_overlap=0.05):
  """Sliding-window float64 form (small sizes): the checker of the FFT forms above."""
  R, H, W, D = q.shape
  win = np.lib.stride_tricks.sliding_window_view(_pad_edge(m), (H, W), axis=(0, 1))       # [Ho, Wo, D, H, W]
  s = np.einsum('abdij,rijd->rab', win, np.asarray(q, np.float64))
  if min_overlap is not None:
    s = np.where(finite_rule(counts_direct(q_valid, m_valid), threshold(min_overlap, H, W)), s, -np.inf)
  with np.errstate(divide='ignore', invalid='ignore'):
    return s / np.asarray(q_valid, np.float64).sum((-1, -2))[:, None, None]


def pair_norms(x):
  """norm2 over space of each complex channel pair z = c_2p + i c_2p+1: x [..., H, W, D] -> [..., P]."""
  x = np.asarray(x, np.float64)
  D = x.shape[-1]
  e = np.zeros(x.shape[:-3] + (2 * ((D + 1) // 2),))
  e[..., :D] = (x * x).sum((-3, -2))
  return np.sqrt(e[..., 0::2] + e[..., 1::2])


def bound(q, m, tcount, N1=None, N2=None):
  """bound[r] (see the module docstring); inf where tcount[r] == 0."""
  g = geometry(q.shape[1], q.shape[2], m.shape[0], m.shape[1])
  N1, N2 = N1 or g['N1'], N2 or g['N2']
  b = EPS * math.log2(N1 * N2) * (pair_norms(q) * pair_norms(_pad_edge(m))[None]).sum(-1)
  with np.errstate(divide='ignore'):
    return b / np.asarray(tcount, np.float64)


# ------------------------------------------- the f32 model -----------------------------------------------------------
F = np.float32


def _twiddles(N):
  ang = -2.0 * 3.14159265358979323846 * np.arange(N, dtype=np.float64) / float(N)
  return np.cos(ang).astype(F), np.sin(ang).astype(F)


def _cmul(a, b):
  return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _cmulc(a, b):      # a * conj(b)
  return a[0] * b[0] + a[1] * b[1], a[1] * b[0] - a[0] * b[1]


def _add(a, b):
  return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
  return a[0] - b[0], a[1] - b[1]


def _add_rot(a, b, inv):   # a + (-i) b forward, a + i b inverse
  return (a[0] - b[1], a[1] + b[0]) if inv else (a[0] + b[1], a[1] - b[0])


def _stage(x, y, N, L, R, inv):
  """One stage on axis 0 of the f32 planes (x, y), in place of the kernel's bfly2/3/4 with their twiddles."""
  M, ts = L // R, N // L
  sh = x.shape
  x = x.reshape((N // L, R, M) + sh[1:]); y = y.reshape(x.shape)
  twc, tws = _twiddles(N)
  k = np.arange(M)
  ex = (slice(None),) + (None,) * (len(sh) - 1)
  w = [None] + [(twc[(j * k * ts) % N][ex], tws[(j * k * ts) % N][ex]) for j in range(1, R)]
  v = [(x[:, j], y[:, j]) for j in range(R)]
  mul = _cmulc if inv else _cmul
  if inv:
    v = [v[0]] + [mul(v[j], w[j]) for j in range(1, R)]
  if R == 4:
    t0, u1, u2, d = _add(v[0], v[2]), _sub(v[0], v[2]), _add(v[1], v[3]), _sub(v[1], v[3])
    o = [_add(t0, u2), _add_rot(u1, d, inv), _sub(t0, u2), _add_rot(u1, d, not inv)]
  elif R == 3:
    sm, df = _add(v[1], v[2]), _sub(v[1], v[2])
    h = _sub(v[0], (F(0.5) * sm[0], F(0.5) * sm[1]))
    c = F(0.86602540378443864676)
    e = (c * df[0], c * df[1])
    o = [_add(v[0], sm), _add_rot(h, e, inv), _add_rot(h, e, not inv)]
  else:
    o = [_add(v[0], v[1]), _sub(v[0], v[1])]
  if not inv:
    o = [o[0]] + [mul(o[j], w[j]) for j in range(1, R)]
  xo = np.stack([a[0] for a in o], 1).reshape(sh)
  yo = np.stack([a[1] for a in o], 1).reshape(sh)
  return xo, yo


def _spans(N):
  rs, Ls, L = radices(N), [], N
  for R in rs:
    Ls.append(L); L //= R
  return list(zip(rs, Ls))


def dif32(z, axis):
  """Forward transform (natural in, digit-reversed out) of the f32 pair z = (re, im) along ``axis``."""
  x, y = (np.ascontiguousarray(np.moveaxis(a, axis, 0), F) for a in z)
  N = x.shape[0]
  for R, L in _spans(N):
    x, y = _stage(x, y, N, L, R, False)
  return np.moveaxis(x, 0, axis), np.moveaxis(y, 0, axis)


def dit32(z, axis):
  """The conjugate transpose of ``dif32``, stage by stage in reverse: N x ifft, natural order out."""
  x, y = (np.ascontiguousarray(np.moveaxis(a, axis, 0), F) for a in z)
  N = x.shape[0]
  for R, L in reversed(_spans(N)):
    x, y = _stage(x, y, N, L, R, True)
  return np.moveaxis(x, 0, axis), np.moveaxis(y, 0, axis)


def _packed(x, lead, H, W, N1, N2):
  """x [lead.., H, W, D] f32 -> channel pairs as (re, im) planes [lead.., N1, N2, P], zero padded."""
  D = x.shape[-1]
  P = (D + 1) // 2
  re = np.zeros(lead + (N1, N2, P), F); im = np.zeros(lead + (N1, N2, P), F)
  re[..., :H, :W, :] = x[..., 0::2]
  im[..., :H, :W, :D // 2] = x[..., 1::2]
  return re, im


def model32(q, q_valid, m, m_valid, thr=None, tcount=None, parts=False):
  """The kernel's arithmetic in f32 -> scores f32 [R, Ho, Wo] (parts=True: also the un-rounded counts, or None)."""
  q, m = np.asarray(q, F), np.asarray(m, F)
  R, H, W, D = q.shape
  Hm, Wm = m.shape[:2]
  g = geometry(H, W, Hm, Wm)
  N1, N2, Ho, Wo = g['N1'], g['N2'], g['Ho'], g['Wo']
  ia = np.clip(np.arange(g['Hp']) - (Hm - 1), 0, Hm - 1)
  ib = np.clip(np.arange(g['Wp']) - (Wm - 1), 0, Wm - 1)
  Zm = dif32(dif32(_packed(m[ia][:, ib], (), g['Hp'], g['Wp'], N1, N2), 0), 1)
  X = dif32(dif32(_packed(q, (R,), H, W, N1, N2), 1), 2)
  P = Zm[0].shape[-1]
  S = (np.zeros((R, N1, N2), F), np.zeros((R, N1, N2), F))
  for g0 in range(0, P, K_COLS):                         # per group: products, the 8 pairs summed, onto the running sum
    acc = S
    for p in range(g0, min(P, g0 + K_COLS)):
      acc = _add(acc, _cmulc((Zm[0][None, ..., p], Zm[1][None, ..., p]), (X[0][..., p], X[1][..., p])))
    S = acc
  Y = dit32(dit32(S, 2), 1)
  scale = F(1.0 / (float(N1) * float(N2)))
  s = (Y[0] * scale)[:, :Ho, :Wo]
  cnt = None
  if thr is not None:
    R2 = (R + 1) // 2
    cw = np.asarray(q_valid, F)[:, ::-1, ::-1]
    cre = np.zeros((R2, N1, N2), F); cim = np.zeros((R2, N1, N2), F)
    cre[:, :H, :W] = cw[:R2]
    cim[:R - R2, :H, :W] = cw[R2:]
    mv = np.zeros((N1, N2), F)
    mv[Hm - 1:2 * Hm - 1, Wm - 1:2 * Wm - 1] = np.asarray(m_valid, F)
    Zv = dif32(dif32((mv, np.zeros_like(mv)), 0), 1)
    Xc = dif32(dif32((cre, cim), 1), 2)
    C = dit32(dit32(_cmulc((Zv[0][None], Zv[1][None]), Xc), 2), 1)
    cnt = np.concatenate([C[0] * scale, (-C[1] * scale)[:R - R2]], 0)[:, :Ho, :Wo]
    s = np.where(np.rint(cnt) > F(thr), s, F(-np.inf))
  tc = np.asarray(q_valid, np.float64).sum((-1, -2)) if tcount is None else tcount
  with np.errstate(divide='ignore', invalid='ignore'):
    s = (s / np.asarray(tc, F)[:, None, None]).astype(F)
  return (s, cnt) if parts else s


# ------------------------------------------- the case table ----------------------------------------------------------
_RS = {16: 20, 24: 17, 32: 3, 48: 2, 64: 1, 96: 20, 128: 17, 192: 3, 256: 2, 384: 1, 512: 3, 768: 2, 1024: 1}
_DS = {16: 34, 24: 18, 32: 16, 48: 6, 64: 2, 96: 34, 128: 18, 192: 16, 256: 6, 384: 2, 512: 6, 768: 2, 1024: 6}
OTHER = 22                       # the other axis of a rectangular case: N = 64


def axis_geometries():
  """Every transform size on each axis, at the largest and at the smallest map that needs it.  'max': the template
  equals the map (<= N / 3 rows: the fused first stage where N = 3 x 2^a); 'min': a template LARGER than the map on
  the long axis (> N / 3 rows where it fits: the unfused first stage) and smaller on the other."""
  out = []
  for N in GPU_SIZES:
    for which in ('max', 'min'):
      big = HM_MAX[N] if which == 'max' else smallest_map(N)
      for axis in (1, 2):
        Hm, Wm = (big, OTHER) if axis == 1 else (OTHER, big)
        if which == 'max':
          H, W = Hm, Wm
        else:
          long_ = min(3 * big - 2, big + big // 2 + 1)
          H, W = (long_, 9) if axis == 1 else (9, long_)
        out.append(dict(name=f'N{N}-{which}-axis{axis}', N=N, which=which, axis=axis, H=H, W=W, Hm=Hm, Wm=Wm,
                        R=_RS[N], D=_DS[N]))
  return out


def _rng(name):
  return np.random.default_rng(int.from_bytes(name.encode(), 'little') % (2 ** 63))


def _masks(rng, g, full):
  R, H, W, Hm, Wm = g['R'], g['H'], g['W'], g['Hm'], g['Wm']
  if full:
    return np.ones((R, H, W), bool), np.ones((Hm, Wm), bool)
  tv, mv = rng.random((R, H, W)) > 0.2, rng.random((Hm, Wm)) > 0.1
  tv[:, H // 2, W // 2] = True                         # (no template without a valid cell)
  return tv, mv


def build(g, kind):
  """kind 'noise': unit noise (all-valid masks at the 'max' maps: the largest counts; partial elsewhere);
  'offset': 10 + noise on both planes, partial validity.  -> q f32, q_valid, m f32, m_valid."""
  rng = _rng(g['name'] + kind)
  R, H, W, D, Hm, Wm = g['R'], g['H'], g['W'], g['D'], g['Hm'], g['Wm']
  tv, mv = _masks(rng, g, full=(kind == 'noise' and g.get('which', 'max') == 'max') or g.get('full', False))
  off = 10.0 if kind == 'offset' else 0.0
  q = ((off + rng.standard_normal((R, H, W, D))) * tv[..., None]).astype(F)
  m = (off + rng.standard_normal((Hm, Wm, D))).astype(F)
  return q, tv, m, mv


SQUARE = dict(name='N1024-square', N=1024, H=342, W=342, Hm=342, Wm=342, R=4, D=4, full=True)

PLANT_R, PLANT_D, PLANT_TCOUNT = 7, 8, 4.0


def planted(g):
  """Planted deltas on geometry g: rotation r has ONE nonzero template cell, in channel r; the map has ONE nonzero
  cell in channel r.  Template cells: (0, 0), the last cell, the interior; map cells: (0, 0), the last cell, the
  interior and the middle of each border (the edge padding replicates those).  Dyadic values, tcount = 4: every
  float64 score is exact.  -> q [7,H,W,8], m [Hm,Wm,8], want float64 [7,Ho,Wo] (closed form, no transform), and the
  list of (r, template cell, map cell)."""
  H, W, Hm, Wm = g['H'], g['W'], g['Hm'], g['Wm']
  tpos = [(0, 0), (H - 1, W - 1), (H // 2, W // 3)]
  mpos = [(0, 0), (Hm - 1, Wm - 1), (Hm // 2, Wm // 3), (0, Wm // 2), (Hm - 1, Wm // 2), (Hm // 2, 0), (Hm // 2, Wm - 1)]
  q = np.zeros((PLANT_R, H, W, PLANT_D), F); m = np.zeros((Hm, Wm, PLANT_D), F)
  geo = geometry(H, W, Hm, Wm)
  want = np.zeros((PLANT_R, geo['Ho'], geo['Wo']))
  cells = []

  def span(u, Lm, i0, Lo):        # padded rows that replicate map row u, shifted by the template row
    lo, hi = (0 if u == 0 else u + Lm - 1), (3 * Lm - 3 if u == Lm - 1 else u + Lm - 1)
    return max(lo - i0, 0), min(hi - i0, Lo - 1)
  for r in range(PLANT_R):
    (i0, j0), (u, v) = tpos[r % 3], mpos[r]
    vq, vm = 2.0 ** (r - 3), -(2.0 ** (2 - r)) if r % 2 else 2.0 ** (2 - r)
    q[r, i0, j0, r] = vq; m[u, v, r] = vm
    (a0, a1), (b0, b1) = span(u, Hm, i0, geo['Ho']), span(v, Wm, j0, geo['Wo'])
    if a1 >= a0 and b1 >= b0:       # (a template cell beyond every replica of the map cell: no placement pairs them)
      want[r, a0:a1 + 1, b0:b1 + 1] = vq * vm / PLANT_TCOUNT
    cells.append((r, (i0, j0), (u, v)))
  return q, m, want, cells


# (template H, W, map Hm, Wm): thresholds passed straight to the explicit entry, all-valid masks
THRESHOLD_GEOMETRIES = [(5, 1, 8, 22), (1, 5, 22, 8), (5, 1, 342, 22), (1, 5, 22, 342)]


def threshold_values(H, W):
  return [0, 1, H * W - 1, H * W]


# (min_overlap, H): the rotated entry's threshold; exact products 8, 1, 63, 12 and (the default) 20
ROTATED_THRESHOLDS = [(0.02, 20), (0.01, 10), (0.07, 30), (0.03, 20), (0.05, 20)]
ROTATED_R, ROTATED_D, ROTATED_CELL = 8, 4, 0.25
ENUM_OVERLAPS = (0.01, 0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4)


def rotated_inputs(min_overlap, H):
  """Query / map planes of a rotated-entry threshold case.  A template cell needs its four bilinear taps valid
  (0.85^4 = 0.52 of the cells), the map keeps 0.6: counts run from 0 to ~0.3 H^2, across every threshold used."""
  rng = _rng(f'rot{min_overlap}-{H}')
  vq = rng.random((H, H)) < 0.85
  fq = (rng.standard_normal((H, H, ROTATED_D)) * vq[..., None]).astype(F)
  fm = rng.standard_normal((H, H, ROTATED_D)).astype(F)
  vm = rng.random((H, H)) < 0.6
  return fq, vq, fm, vm


def chain_disagreements():
  """Every (min_overlap, H) of the enumeration where the f32 chain falls below an integer double product."""
  out = []
  for mo in ENUM_OVERLAPS:
    for H in range(4, 343):
      exact, chain = mo * H * H, float(threshold_f32_chain(mo, H, H))
      if exact == int(exact) and chain < exact and float(threshold(mo, H, H)) == exact:
        out.append((mo, H, chain, exact))
  return out


@functools.lru_cache(maxsize=None)
def axis_case(name, kind):
  """Inputs and float64 expectations of one axis case, computed once."""
  g = {c['name']: c for c in axis_geometries() + [SQUARE]}[name]
  q, tv, m, mv = build(g, kind)
  thr = threshold(0.05, g['H'], g['W'])
  cnt = counts64(tv, mv)
  tc = tv.sum((-1, -2)).astype(np.float64)
  raw = raw64(q, m) / tc[:, None, None]
  for a in (q, tv, m, mv, cnt, raw):
    a.setflags(write=False)
  return dict(g=g, q=q, tv=tv, m=m, mv=mv, thr=thr, counts=cnt, raw=raw, bound=bound(q, m, tc), tcount=tc)
