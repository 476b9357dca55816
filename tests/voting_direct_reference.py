"""Test infrastructure: the float64 reference of the DIRECT-form voting (``snap_amd/csrc/voting.hip``,
``rotate_sample.h`` and the host half ``_correlate`` / ``_overlap_count`` / ``_match`` of
``snap_amd/models/pose_exhaustive_voting.py``), its error bounds, f32 / split-bf16 models of the dot product, index
restatements of the shift-stacking and of the folded overlap count, the route the host half takes, and the case table
that tests/test_voting_direct_reference.py (CPU) and tests/test_gpu_voting_direct.py (GPU) share.  numpy / scipy only;
nothing in ``snap_amd/`` imports it.  The correlation, the integer counts and the threshold rule are
``voting_fft_reference``'s (``V``): the two formulations answer to the same float64 numbers.

* ``rotate64`` / ``rotate32``: ``snap_rot_geom`` + ``snap_rot_sample`` + ``snap_rot_mix`` and the rot90 completion, in
  float64 and (a CPU model, used only to set margins) in float32 in the header's expression order.
* ``value_bound``: first-order f32 bound of one template element,
      ARITH x 2^-24 x sum_k |w_k a_k|  +  COORD x 2^-24 x H x (|du-slope| + |dv-slope|)
  ARITH = 8 roundings on the path of a value (1 - w, two weight products, the tap product, three adds: 7, taken as 8);
  the coordinate carries COORD = 12 roundings of magnitude <= H cells, counted from the expression: gx, gy, c gx, s gy,
  their difference, + tx, the divide (7); the f32 entries c, s (2) and tx (3: the rounded centre, its rotation, the sum)
  of the transform; it moves the value by its slope along each axis (the steeper side where a tap-pair seam is near).
* ``score_bound``: ``C[engine] x 2^-24 x A / tcount`` per cell, A = sum |q| |m_pad| (``abs_corr64``).
  C[engine] = ACC[engine] + OPERAND[engine]: OPERAND is derived from the split (below), ACC is the smallest power of
  two at which two numpy models of the f32 accumulation (sequential in (i, j, d) order; 16-wide k-steps onto a running
  f32 sum) stay within 0.5 x the bound on a SAMPLE of 16 placements (``sample_cells``: corners, centre, 11 drawn) of
  every GPU input (tests/test_voting_direct_reference.py measures it; never the kernel).
      bf16x3: hi = bf16(v), lo = bf16(v - hi): |v - hi - lo| <= 2^-18 |v| per operand, a_lo b_lo <= 2^-18 |a b| dropped
              -> 3 x 2^-18 = 192 x 2^-24 per product;
      bf16x6: three parts, |v - hi - mid - lo| <= 2^-27 |v|; a_mid b_lo + a_lo b_mid + a_lo b_lo <= 2^-26 dropped
              -> 2^-25, taken as 1 x 2^-24.
"""
import functools

import numpy as np

import voting_fft_reference as V
from attention_reference import round_bf16

EPS = 2.0 ** -24
F = np.float32
ARITH, COORD = 8.0, 12.0
VALUE_MARGIN = 8.0                 # the GPU test allows VALUE_MARGIN x value_bound; the f32 model stays within half
BORDER_TOL = 1e-4                  # helpers.assert_template_validity_mismatches_on_borders
FLIP_CAP = 0.01                    # at most 1 % of a case's (r, i, j) cells may flip, all within BORDER_TOL
OPERAND = {'f32': 0.0, 'bf16x3': 192.0, 'bf16x6': 1.0}
# measured on sampled placements by tests/test_voting_direct_reference.py::test_models_stay_within_half_the_bound
ACC = {'f32': 256.0, 'bf16x3': 256.0, 'bf16x6': 128.0}
C = {e: ACC[e] + OPERAND[e] for e in ACC}


# ------------------------------------------- rotation ---------------------------------------------------------------
def angles32(R):
  return np.linspace(0, np.pi * 2, R, endpoint=False).astype(F)


def transforms(R, H, cell, dtype=np.float64):
  """(cos, sin, tx, ty) [R/4, 4] of corner_t_center @ rot(theta) @ corner_t_center^-1, as ``_template_transforms``
  builds it: angles rounded to f32, the centre extent / 2 rounded to f32, then float64."""
  th = angles32(R)[: R // 4].astype(np.float64)
  cx = cy = float(F(H * cell / 2.0))
  c, s = np.cos(th), np.sin(th)
  return np.stack([c, s, cx - (c * cx - s * cy), cy - (s * cx + c * cy)], -1).astype(dtype)


def _complete(q0, direction=1, swap_index=False):
  """[R/4, H, W, ...] -> [R, H, W, ...]: quadrant k = jnp.rot90(quarter, k, axes=(2, 1)), stored at k R/4 + r0."""
  parts = [np.rot90(q0, k * direction, axes=(2, 1)) for k in range(4)]
  out = np.concatenate(parts, 0)
  if swap_index:                                           # (mutant: r0 * 4 + k)
    RQ = q0.shape[0]
    sw = np.empty_like(out)
    for k in range(4):
      for r0 in range(RQ):
        sw[r0 * 4 + k] = parts[k][r0]
    out = sw
  return out


def _rotate(feat, valid, R, H, cell, dtype, mutant=None):
  T = dtype
  feat = np.asarray(feat)
  valid = np.asarray(valid, bool)
  assert feat.shape[:2] == (H, H) and R % 4 == 0
  tfm = transforms(R, H, cell, T)
  c, s, tx, ty = (tfm[:, k][:, None, None] for k in range(4))
  cellT = T(F(cell))                                      # the kernel's ``float cell``
  half, one, zero = T(0.5), T(1.0), T(0.0)
  idx = np.arange(H).astype(T)
  gx = ((idx + half) * cellT)[None, :, None]
  gy = ((idx + half) * cellT)[None, None, :]
  xm = (c * gx - s * gy) + tx
  ym = (s * gx + c * gy) + ty
  u, v = xm / cellT, ym / cellT
  Hf = T(H)
  if mutant == 'unclamped':                                # taps outside the grid wrap instead of clamping
    clamp = lambda f: (f.astype(np.int64)) % H
  else:
    clamp = lambda f: np.clip(f, zero, T(H - 1)).astype(np.int64)

  def sample(u, v):
    inside = (u >= zero) & ((u <= Hf) if mutant == 'u<=H' else (u < Hf)) & (v >= zero) & (v < Hf)
    cu, cv = u - half, v - half
    fu, fv = np.floor(cu), np.floor(cv)
    wu1, wv1 = cu - fu, cv - fv
    wu0, wv0 = one - wu1, one - wv1
    i0, i1, j0, j1 = clamp(fu), clamp(fu + one), clamp(fv), clamp(fv + one)
    w = [wu0 * wv0, wu0 * wv1, wu1 * wv0, wu1 * wv1]
    taps = [(i0, j0), (i0, j1), (i1, j0), (i1, j1)]
    if mutant == 'weighted-taps':                          # validity from the taps that carry weight only
      ok = inside.copy()
      for wk, (i, j) in zip(w, taps):
        ok &= valid[i, j] | (wk == zero)
    else:
      ok = inside & valid[i0, j0] & valid[i0, j1] & valid[i1, j0] & valid[i1, j1]
    return ok, cu, cv, w, taps, (wu0, wu1), (wv0, wv1)
  ok, cu, cv, w, taps, wu, wv = sample(u, v)
  (wu0, wu1), (wv0, wv1) = wu, wv
  fragile = np.zeros(ok.shape, bool)
  if T is np.float64:                                      # validity at (u, v) moved by BORDER_TOL in any direction
    for du in (-BORDER_TOL, 0.0, BORDER_TOL):
      for dv in (-BORDER_TOL, 0.0, BORDER_TOL):
        fragile |= sample(u + du, v + dv)[0] != ok
  def gather(ok, taps):
    return [np.where(ok[..., None], feat[i, j].astype(T), zero) for i, j in taps]

  def slopes(a, wu, wv):
    a00, a01, a10, a11 = a
    su = np.abs(a10 - a00) * wv[0][..., None] + np.abs(a11 - a01) * wv[1][..., None]
    sv = np.abs(a01 - a00) * wu[0][..., None] + np.abs(a11 - a10) * wu[1][..., None]
    return su + sv
  a = gather(ok, taps)
  wa = [wk[..., None] * ak for wk, ak in zip(w, a)]
  val = ((wa[0] + wa[1]) + wa[2]) + wa[3]
  val = np.where(ok[..., None], val, zero).astype(T)
  slope = slopes(a, wu, wv)
  if T is np.float64:                                      # bilinear: continuous, piecewise linear -- the steeper side of a seam
    for du in (-BORDER_TOL, BORDER_TOL):
      for dv in (-BORDER_TOL, BORDER_TOL):
        o2, _, _, _, t2, wu2, wv2 = sample(u + du, v + dv)
        slope = np.maximum(slope, slopes(gather(o2 & ok, t2), wu2, wv2))
  return dict(val=val, ok=ok, u=u, v=v, cu=cu, cv=cv, w=w, a=a, wa=wa, wu=(wu0, wu1), wv=(wv0, wv1), fragile=fragile, slope=slope)


def _nearest(x):
  return np.abs(x - np.rint(x))


def rotate64(feat, valid, R, H, cell, mutant=None):
  """-> dict: templates [R,H,H,D] float64, tvalid [R,H,H], cw [H,H,R] (the 180-degree flipped mask as float), tcount
  [R], and per (r, i, j) the float64 distances ``border`` (u / v to 0 and H) and ``seam`` (cu / cv to the nearest
  integer: a change of the tap pair)."""
  g = _rotate(feat, valid, R, H, cell, np.float64, mutant)
  kw = {}
  if mutant == 'rot90-reversed':
    kw = dict(direction=-1)
  elif mutant == 'quadrant-index':
    kw = dict(swap_index=True)
  Hf = float(H)
  border = np.minimum.reduce([np.abs(g['u']), np.abs(g['u'] - Hf), np.abs(g['v']), np.abs(g['v'] - Hf)])
  seam = np.minimum(_nearest(g['cu']), _nearest(g['cv']))
  tvalid = _complete(g['ok'], **kw)
  cw = tvalid.transpose(1, 2, 0).astype(np.float64)
  if mutant != 'cw-unflipped':
    cw = cw[::-1, ::-1]
  tcount = tvalid.sum((-1, -2)).astype(np.float64)
  if mutant == 'tcount-ballot':                            # one wave's ballot (up to 64 cells) added twice
    tcount = tcount + np.minimum(64, tcount)
  return dict(templates=_complete(g['val'], **kw), tvalid=tvalid, cw=np.ascontiguousarray(cw), tcount=tcount,
              border=_complete(border, **kw), seam=_complete(seam, **kw), fragile=_complete(g['fragile'], **kw), value_bound=_complete(_value_bound(g, H), **kw))


def rotate32(feat, valid, R, H, cell):
  """The same in np.float32, in the header's expression order -> templates f32 [R,H,H,D], tvalid."""
  g = _rotate(np.asarray(feat, F), valid, R, H, cell, F)
  assert g['val'].dtype == F and g['u'].dtype == F
  return _complete(g['val']), _complete(g['ok'])


def _value_bound(g, H):
  mag = sum(np.abs(x) for x in g['wa'])
  return EPS * (ARITH * mag + COORD * H * g['slope'])


def value_bound(feat, valid, R, H, cell):
  """Per template element [R,H,H,D] (see the module docstring); 0 on invalid cells, which must be exactly 0."""
  return rotate64(feat, valid, R, H, cell)['value_bound']


def near_decision(ref):
  """Cells of ``rotate64``'s result whose validity two correct f32 evaluations may decide differently: moving the
  float64 coordinate by BORDER_TOL cell in some direction changes it (a grid border, or a change of the tap pair that
  brings an invalid tap in or out)."""
  return ref['fragile']


# ------------------------------------------- scores -----------------------------------------------------------------
def abs_corr64(q, m):
  """A[r, a, b] = sum |q| |m_pad| (edge padded)."""
  return np.maximum(V._corr64(np.abs(np.asarray(q, np.float64)), V._pad_edge(np.abs(np.asarray(m, np.float64)))), 0.0)


def score_bound(q, m, tcount, engine):
  with np.errstate(divide='ignore', invalid='ignore'):
    return C[engine] * EPS * abs_corr64(q, m) / np.asarray(tcount, np.float64)[:, None, None]


def sample_cells(name, Ho, Wo, n=96):
  """A deterministic sample of placements: the corners, the centre and ``n`` random ones."""
  rng = V._rng('cells' + name)
  cells = {(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (Ho // 2, Wo // 2)}
  while len(cells) < min(n + 5, Ho * Wo):
    cells.add((int(rng.integers(Ho)), int(rng.integers(Wo))))
  return sorted(cells)


def _split(x, parts):
  out, rest = [], np.asarray(x, np.float64)
  for _ in range(parts):
    p = round_bf16(rest)
    out.append(p)
    rest = rest - p
  return out


def model_dot(q, m, cells, engine, mode):
  """The raw sums at ``cells`` [(a, b)] -> f32 [R, len(cells)], modelled:
  mode 'seq': every product rounded to f32 and added to an f32 sum in (i, j, d) order;
  mode 'kstep': 16 products per k-step, summed exactly, each k-step's sum added to a running f32 sum.
  The split engines replace a product by the kept part products (``round_bf16`` splits, as conv_split.hip states them)."""
  R, H, W, D = q.shape
  mp = V._pad_edge(np.asarray(m, F))
  K = H * W * D
  Kp = -(-K // 16) * 16
  qk = np.zeros((R, Kp)); qk[:, :K] = np.asarray(q, np.float64).reshape(R, K)
  out = np.empty((R, len(cells)), F)
  parts = {'f32': 1, 'bf16x3': 2, 'bf16x6': 3}[engine]
  qs = _split(qk, parts) if parts > 1 else None
  keep = {2: [(0, 0), (0, 1), (1, 0)], 3: [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]}.get(parts)
  for n, (a, b) in enumerate(cells):
    wk = np.zeros(Kp); wk[:K] = mp[a:a + H, b:b + W].reshape(K)
    if parts == 1:
      prod = qk * wk[None]
    else:
      ws = _split(wk, parts)
      prod = sum(qs[i] * ws[j][None] for i, j in keep)
    if mode == 'seq':
      out[:, n] = np.cumsum(prod.astype(F), axis=1, dtype=F)[:, -1]
    else:
      out[:, n] = np.cumsum(prod.reshape(R, Kp // 16, 16).sum(-1).astype(F), axis=1, dtype=F)[:, -1]
  return out


# ------------------------------------------- stacking, fold, containment --------------------------------------------
def stack_bank(templates, S):
  """tws[i', j', d, (r S + sa) S + sb] = templates[r, i' - sa, j' - sb, d], 0 outside."""
  R, H, W, D = templates.shape
  tws = np.zeros((H + S - 1, W + S - 1, D, R * S * S), templates.dtype)
  for r in range(R):
    for sa in range(S):
      for sb in range(S):
        tws[sa:sa + H, sb:sb + W, :, (r * S + sa) * S + sb] = templates[r]
  return tws


def stacked_geometry(H, W, S, Hp, Wp):
  Ho, Wo = Hp - H + 1, Wp - W + 1
  A4, B4 = -(-Ho // S), -(-Wo // S)
  pb = max(0, S * (A4 - 1) + (H + S - 1) - Hp)
  pr = max(0, S * (B4 - 1) + (W + S - 1) - Wp)
  return dict(Ho=Ho, Wo=Wo, A4=A4, B4=B4, pb=pb, pr=pr)


def unstack(raw4, R, S, Ho, Wo, mutant=None):
  """raw4 [A4, B4, R S S] -> [Ho, Wo, R]: what ``_correlate`` does after the GEMM."""
  A4, B4 = raw4.shape[:2]
  x = raw4.reshape(A4, B4, R, S, S)
  if mutant == 'crop-first':                               # crop in the GEMM's own (block) coordinates, then un-stack
    x = x[:Ho // S, :Wo // S]
    A4, B4 = x.shape[:2]
  perm = (0, 4, 1, 3, 2) if mutant == 'swap' else (0, 3, 1, 4, 2)
  raw = x.transpose(perm).reshape(A4 * S, B4 * S, R)
  return np.ascontiguousarray(raw[:Ho, :Wo])


def stacked_corr64(templates, mp, S, mutant=None):
  """The stride-S correlation of the zero-extended ``mp`` [Hp, Wp, D] with ``stack_bank`` in float64, un-stacked."""
  R, H, W, D = templates.shape
  g = stacked_geometry(H, W, S, mp.shape[0], mp.shape[1])
  pb = 0 if mutant == 'pb=0' else g['pb']
  x = np.pad(np.asarray(mp, np.float64), ((0, pb), (0, g['pr']), (0, 0)))
  if mutant == 'pb=0' and g['pb']:                         # the last block row has no window: the GEMM has A4 - 1 rows
    A4 = (x.shape[0] - (H + S - 1)) // S + 1
  else:
    A4 = g['A4']
  win = np.lib.stride_tricks.sliding_window_view(x, (H + S - 1, W + S - 1), axis=(0, 1))[::S, ::S][:A4, :g['B4']]
  raw4 = np.einsum('abdij,ijdn->abn', win, stack_bank(np.asarray(templates, np.float64), S))
  return unstack(raw4, R, S, g['Ho'], g['Wo'], mutant if mutant in ('swap', 'crop-first') else None)


def fold_counts(mvp, cw, mutant=None):
  """The W % 32 == 0 fold of ``_overlap_count``: mvp [Hp, Wp] zero-padded mask, cw [H, W, R] flipped template masks
  -> integer counts [R, Ho, Wo] (``V.counts_direct``'s)."""
  mvp, cw = np.asarray(mvp, np.int64), np.asarray(cw, np.int64)
  H, W, R = cw.shape
  assert W % 32 == 0
  Hp, Wp = mvp.shape
  Ho, Wo = Hp - H + 1, Wp - W + 1
  nbq = -(-Wo // 32)
  ncol = nbq + W // 32 - 1 - (1 if mutant == 'ncol-short' else 0)
  need = 32 * (ncol - 1) + 31 + 31 + 1
  mv = np.pad(mvp, ((0, 0), (0, max(0, need - Wp))))
  win = np.lib.stride_tricks.sliding_window_view(mv, 32, axis=1)[:, :32 * ncol]     # win[row, s, c] = mv[row, s + c]
  X = win.reshape(Hp, ncol, 32, 32).transpose(2, 0, 1, 3)                          # [br, row, col, c]
  wq = cw.reshape(H, W // 32, 32, R)                                               # [i, t, c, r]
  xw = np.lib.stride_tricks.sliding_window_view(X, (H, W // 32), axis=(1, 2))       # [br, a, bq, c, i, t]
  out = np.einsum('xabcit,itcr->xabr', xw, wq)                                     # [32, Ho, nbq', R]
  return np.ascontiguousarray(out.transpose(1, 2, 0, 3).reshape(Ho, -1, R)[:, :Wo].transpose(2, 0, 1))


def padded_cells(Hm, Wm, cell):
  """The cells of the edge-padded map [3 Hm - 2, 3 Wm - 2] that replicate map cell (u, v)."""
  def span(x, L):
    lo = 0 if x == 0 else x + L - 1
    hi = 3 * L - 3 if x == L - 1 else x + L - 1
    return range(lo, hi + 1)
  return [(y, x) for y in span(cell[0], Hm) for x in span(cell[1], Wm)]


def plain_nonfinite_set(H, W, Hp, Wp, bad_cells):
  """Placements (a, b) whose H x W window at (a, b) covers a bad cell of the padded map -> bool [Ho, Wo]."""
  Ho, Wo = Hp - H + 1, Wp - W + 1
  a, b = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
  out = np.zeros((Ho, Wo), bool)
  for y, x in bad_cells:
    out |= (a <= y) & (y <= a + H - 1) & (b <= x) & (x <= b + W - 1)
  return out


def stacked_nonfinite_set(H, W, S, Hp, Wp, bad_cells):
  """The shift-stacked form: every output of the S x S block (floor(a / S), floor(b / S)) is a sum over the WIDENED
  window (H + S - 1) x (W + S - 1) anchored at (S floor(a / S), S floor(b / S)); the bank holds zeros outside each
  shifted copy and 0 x NaN = NaN."""
  Ho, Wo = Hp - H + 1, Wp - W + 1
  a, b = (np.arange(Ho) // S * S)[:, None], (np.arange(Wo) // S * S)[None, :]
  out = np.zeros((Ho, Wo), bool)
  for y, x in bad_cells:
    out |= (a <= y) & (y <= a + H + S - 2) & (b <= x) & (x <= b + W + S - 2)
  return out


# ------------------------------------------- the route --------------------------------------------------------------
DEFAULT_SWITCHES = dict(STACK_SHIFT=4, STACK_MIN_CELLS=64 * 64, USE_PRESPLIT_VOTING=True, FUSED_TEMPLATE_PACK=True,
                        presplit_supported=True, have_templates=True)


def restated_route(R, H, W, D, precision='f32', switches=None):
  """-> ('plain' | 'stacked' | 'presplit' | 'presplit+fused', 'scalar-count' | 'folded-count'), restated from
  ``_stacked`` / ``_correlate`` / ``_overlap_count``.  ``presplit_supported`` stands for the engine's own answer
  (``ops.conv2d_presplit_supported``), ``have_templates`` for the [R, H, W, D] tensor being at hand."""
  sw = dict(DEFAULT_SWITCHES, **(switches or {}))
  S = sw['STACK_SHIFT']
  stacked = S > 1 and H * W >= sw['STACK_MIN_CELLS'] and (R * S * S) % 4 == 0
  count = 'folded-count' if stacked and W % 32 == 0 else 'scalar-count'
  if not stacked:
    return 'plain', count
  presplit = (precision == 'bf16x3' and sw['USE_PRESPLIT_VOTING'] and D % 16 == 0 and (R * S * S) % 192 == 0
              and sw['presplit_supported'])
  if not presplit:
    return 'stacked', count
  return ('presplit+fused' if sw['have_templates'] and sw['FUSED_TEMPLATE_PACK'] else 'presplit'), count


# ------------------------------------------- the case table ---------------------------------------------------------
def _case(route, H, W, Hm, Wm, R, D, engine='f32', count='scalar-count', **switches):
  name = f'{route}-{H}x{W}-map{Hm}x{Wm}-R{R}-D{D}-{engine}'
  if 'STACK_SHIFT' in switches:
    name += f'-S{switches["STACK_SHIFT"]}'
  if switches.get('FUSED_TEMPLATE_PACK') is False:
    name += '-unfused'
  return dict(name=name, route=route, count=count, H=H, W=W, Hm=Hm, Wm=Wm, R=R, D=D, engine=engine, switches=switches)


CASES = [
    _case('plain', 5, 5, 5, 5, 4, 4),
    _case('plain', 16, 16, 16, 16, 8, 8),
    _case('plain', 10, 13, 12, 9, 12, 16),
    _case('plain', 13, 10, 9, 12, 12, 16),
    _case('plain', 7, 7, 20, 20, 7, 4),                    # odd R: explicit templates only
    _case('plain', 20, 20, 8, 8, 4, 4),                    # a template larger than the map (7 x 7 would leave Ho = 3 Hm - 1 - H = 0)
    _case('plain', 16, 16, 16, 16, 8, 8, 'bf16x3'),
    _case('plain', 16, 16, 16, 16, 8, 8, 'bf16x6'),
    _case('stacked', 64, 64, 64, 64, 4, 4, count='folded-count'),      # S = 4, Ho = 127, one folded tap
    _case('stacked', 64, 96, 64, 96, 4, 4, count='folded-count'),      # three folded taps, Wo % 32 != 0
    _case('stacked', 66, 66, 66, 66, 4, 4),                            # stacked with the scalar count
    _case('stacked', 64, 64, 40, 40, 4, 4, count='folded-count'),      # the map smaller than the template
    _case('stacked', 24, 24, 24, 24, 4, 4, STACK_SHIFT=3, STACK_MIN_CELLS=0),
    _case('stacked', 20, 20, 20, 20, 4, 4, STACK_SHIFT=3, STACK_MIN_CELLS=0),     # S = 3 divides Ho = 39
    _case('stacked', 24, 24, 24, 24, 4, 4, STACK_SHIFT=2, STACK_MIN_CELLS=0),
    _case('stacked', 20, 20, 20, 20, 4, 4, STACK_SHIFT=2, STACK_MIN_CELLS=0),
    _case('presplit+fused', 64, 64, 64, 64, 12, 16, 'bf16x3', count='folded-count'),      # R S^2 = 192
    _case('presplit', 64, 64, 64, 64, 12, 16, 'bf16x3', count='folded-count', FUSED_TEMPLATE_PACK=False),
    _case('stacked', 64, 64, 64, 64, 4, 16, 'bf16x3', count='folded-count'),              # R S^2 = 64: falls back
    _case('stacked', 64, 64, 64, 64, 12, 8, 'bf16x3', count='folded-count'),              # D % 16 != 0: falls back
]
CASE_IDS = [c['name'] for c in CASES]
BY_NAME = {c['name']: c for c in CASES}
KINDS = ('noise', 'offset', 'full')
PRODUCTION = [c for c in CASES if not {'STACK_SHIFT', 'STACK_MIN_CELLS'} & set(c['switches'])]


def build(g, kind):
  """'noise': unit noise, 85 % / 90 % validity; 'offset': 10 + noise on both planes, the same validity; 'full': unit
  noise, all-valid masks (count == the overlap area).  -> q f32 (zero under invalid cells), q_valid, m f32, m_valid."""
  rng = V._rng(g['name'] + kind)
  R, H, W, D, Hm, Wm = g['R'], g['H'], g['W'], g['D'], g['Hm'], g['Wm']
  if kind == 'full':
    tv, mv = np.ones((R, H, W), bool), np.ones((Hm, Wm), bool)
  else:
    tv, mv = rng.random((R, H, W)) < 0.85, rng.random((Hm, Wm)) < 0.9
    tv[:, H // 2, W // 2] = True
  off = 10.0 if kind == 'offset' else 0.0
  q = ((off + rng.standard_normal((R, H, W, D))) * tv[..., None]).astype(F)
  m = (off + rng.standard_normal((Hm, Wm, D))).astype(F)
  return q, tv, m, mv


@functools.lru_cache(maxsize=None)
def case(name, kind):
  """Inputs and float64 expectations of one table case, computed once and left unchanged."""
  g = BY_NAME[name]
  q, tv, m, mv = build(g, kind)
  thr = V.threshold(0.05, g['H'], g['W'])
  cnt = V.counts64(tv, mv)
  tc = tv.sum((-1, -2)).astype(np.float64)
  raw = V.raw64(q, m) / tc[:, None, None]
  b = score_bound(q, m, tc, g['engine'])
  for a in (q, tv, m, mv, cnt, raw, b):
    a.setflags(write=False)
  return dict(g=g, q=q, tv=tv, m=m, mv=mv, thr=thr, counts=cnt, raw=raw, bound=b, tcount=tc)


def planted(g):
  """``V.planted`` on geometry g with the masks ``template_matching`` needs: exactly PLANT_TCOUNT = 4 valid cells
  per rotation (the planted cell among them) -> q, tv, m, mv (all valid), want, cells."""
  q, m, want, cells = V.planted(g)
  H, W = g['H'], g['W']
  tv = np.zeros((V.PLANT_R, H, W), bool)
  for r, (i0, j0), _ in cells:
    tv[r, i0, j0] = True
    k = 0
    while tv[r].sum() < int(V.PLANT_TCOUNT):
      tv[r, (i0 + 1 + k) % H, (j0 + 2 * k) % W] = True
      k += 1
  return q, tv, m, np.ones((g['Hm'], g['Wm']), bool), want, cells


PLANTED_GEOMETRIES = [dict(name='planted-plain', H=10, W=13, Hm=12, Wm=9), dict(name='planted-stacked', H=64, W=64, Hm=64, Wm=64),
                      dict(name='planted-stacked-small-map', H=64, W=64, Hm=40, Wm=40)]

# rotation cases of the GPU file: R x H x D x cell
ROTATE_CASES = [(R, H, D, cell) for R in (4, 8, 12, 36) for H in (5, 8, 16, 33) for D in (4, 12) for cell in (0.25, 0.3)]


@functools.lru_cache(maxsize=None)
def rotate_inputs(R, H, D, cell):
  """feat f32 [H,H,D], valid [H,H] with at least one invalid cell.  The rotations by multiples of 90 degrees map every
  cell ONTO a tap-pair seam (u - 0.5 integral); so do, for odd H, the centre lines at every angle and a diagonal at 45
  degrees.  The mask is the densest of 90 / 97 / 99 % validity (then: one invalid cell) and the first seed at which
  float64 alone has at most FLIP_CAP / 4 of the case's cells within BORDER_TOL of a decision on the rotations the cap
  covers (``reference_alone_count``)."""
  def attempts():
    for density in (0.9, 0.97, 0.99):
      for salt in range(48):
        rng = V._rng(f'rotate-{R}-{H}-{D}-{cell}-{density}-{salt}')
        valid = rng.random((H, H)) < density
        if valid.all():
          valid[int(rng.integers(H)), int(rng.integers(H))] = False
        yield rng, valid
    for k in range(H * H):
      valid = np.ones((H, H), bool)
      valid[k // H, k % H] = False
      yield V._rng(f'rotate-{R}-{H}-{D}-{cell}-one-{k}'), valid
  for rng, valid in attempts():
    feat = rng.standard_normal((H, H, D)).astype(F)
    if reference_alone_count(rotate64(feat, valid, R, H, cell)) <= FLIP_CAP / 4 * R * H * H:
      feat.setflags(write=False); valid.setflags(write=False)
      return feat, valid
  raise AssertionError((R, H, D, cell))


def capped_rotations(R):
  """The rotations the flip cap covers: all but the multiples of 90 degrees, whose every cell sits on a seam (with cell
  0.25 their coordinates are exact and they are held to exact validity instead; with cell 0.3, where
  (i + 0.5) x cell / cell is inexact in f32, a flip there is accepted only inside ``near_decision``, uncapped)."""
  return np.arange(R) % (R // 4) != 0


def reference_alone_count(ref):
  """Cells the capped escape class COULD take: ``near_decision`` cells of the capped rotations."""
  return int(near_decision(ref)[capped_rotations(len(ref['tvalid']))].sum())
