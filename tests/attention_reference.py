"""Host restatement of the attention kernels of vit_ops.hip / vit_bwd.hip (TEST INFRASTRUCTURE).

numpy, float64 arithmetic with the kernels' roundings made explicit, block for block in the kernels'
order; written from the kernels' comments and include/snap_hip.h, imports nothing of the package.

Forward (``attention_kernel<HIN>``), per (batch, head), every query alike:
  c   = float32(scale * 1.4426950408889634f)
  q~  = bf16(float32(q * c))            f32 qkv; the bf16-qkv form (HIN) takes q already rounded: one
                                        more rounding, and k / v as given instead of rounded here
  keys in blocks of 64: s_j = q~ . k_j (keys >= N masked out),
      m' = max(m, max_j s_j)   alpha = 2^(m - m')   p_j = 2^(s_j - m')      (p held in f32)
      l  = l alpha + sum_j p_j             <- the UNROUNDED p
      o  = o alpha + sum_j bf16(p_j) v_j   <- the rounded p into the matrix-core product
  out = o / l    out_half = bf16(out)    lse = m + log2(l)

VJP (``attention_bwd_dq_kernel`` / ``attention_bwd_dkv_kernel``; both recompute P from the saved lse):
  delta = sum_d dout out          P = 2^(s - lse)        dP = bf16(dout) bf16(v)^T
  dS = P (dP - delta)             dq = scale bf16(dS) bf16(k)
  dk = ln2 bf16(dS)^T q~          dv = bf16(P)^T bf16(dout)

What the restatement does NOT fix is what two correct f32 implementations may differ in: the order of the
f32 sums and the last bit of exp2.  ``twin=<seed>`` is a NOISE TWIN: scores (and dP) accumulated in
float32 over a permuted order of d, every p moved one f32 ulp up or down, l held in f32 and the results
stored in f32 as the kernels store them.  |model - twin| measures what that freedom is worth on a given
input, and it is a heavy-tailed quantity: a p that lies within the f32 noise of a bf16 tie rounds to the
other neighbour in about every second twin, and one such flip moves the output by up to 2^-7 P |v|, orders of
magnitude more than everything else.  One draw is a one-sample estimate of that maximum (it misses every
second reachable flip), so the tolerances at the bottom of this file take the maximum over the
``TWIN_SEEDS`` draws -- from the reference alone, never from the kernel's output.

``mutant=<name>`` breaks one rounding point or one mask on purpose; tests/test_attention_reference.py
shows that the tolerances reject each of them.
"""
import numpy as np
import torch

f32 = np.float32
f64 = np.float64

KEY_BLOCK = 64
LOG2E_F32 = f32(1.4426950408889634)
LN2_F32 = f32(0.6931471805599453)
BF16_MAX = float((2.0 - 2.0 ** -7) * 2.0 ** 127)

FORWARD_MUTANTS = ('drop_last_key', 'tail_key_twice', 'l_from_rounded_p', 'q_rounded_twice', 'log2e_bf16',
                   'no_alpha_on_l', 'lse_natural_log')
VJP_MUTANTS = ('dv_from_unrounded_p', 'dk_without_ln2', 'delta_zero')


def round_f32(x):
  """float64 -> nearest float32 (as float64)."""
  with np.errstate(over='ignore', invalid='ignore'):
    return np.asarray(x, f64).astype(f32).astype(f64)


def round_bf16(x):
  """float64 -> nearest bfloat16, ties to even (as float64): 8 significant bits, subnormals on the 2^-133
  grid, overflow to inf; non-finite values pass."""
  x = np.asarray(x, f64)
  with np.errstate(all='ignore'):
    _, e = np.frexp(x)                                   # |x| in [2^(e-1), 2^e)
    quantum = np.ldexp(1.0, np.maximum(e, -125) - 8)
    r = np.rint(x / quantum) * quantum
    r = np.where(np.abs(r) > BF16_MAX, np.sign(x) * np.inf, r)
  return np.where(np.isfinite(x), r, x)


def _heads_first(t):
  """[B, N, H, D] -> [B, H, N, D]"""
  return np.ascontiguousarray(np.moveaxis(t, 2, 1))


def _dot(a, b, perm):
  """a [..., M, D] . b [..., K, D] -> [..., M, K].  perm None: float64 (exact products, float64 sums).
  perm given (the twin): a float32 accumulator over d in that order -- the products of two bf16 values are
  exact in float32, every partial sum is rounded."""
  if perm is None:
    return np.einsum('...md,...kd->...mk', a, b)
  a32, b32 = a.astype(f32), b.astype(f32)
  acc = np.zeros(a.shape[:-1] + (b.shape[-2],), f32)
  for d in perm:
    acc = acc + a32[..., :, None, d] * b32[..., None, :, d]
  return acc.astype(f64)


def _one_ulp(p, rng):
  """Every positive p (float32-valued) moved to a float32 neighbour, up or down at random."""
  up = rng.integers(0, 2, p.shape).astype(bool)
  p32 = p.astype(f32)
  moved = np.nextafter(p32, np.where(up, f32(np.inf), f32(0))).astype(f64)
  return np.where(p > 0, moved, p)


def _constants(D, scale, mutant):
  assert D == 64, 'the kernels take head dimension 64 only'
  sc = f32(D ** -0.5 if scale is None else scale)
  c = f32(sc * (f32(1.4453125) if mutant == 'log2e_bf16' else LOG2E_F32))   # 1.4453125 = bf16(log2 e)
  return sc, c


def attention_forward(qkv, scale=None, half_in=False, mutant=None, twin=None):
  """qkv [B, N, 3, H, 64] (float32-valued; bf16-valued with half_in) -> dict(out [B, N, H*64] float64,
  out_half (bf16-valued), lse [B, H, N] float64)."""
  assert mutant is None or mutant in FORWARD_MUTANTS, mutant
  x = np.asarray(qkv, f64)
  B, N, three, H, D = x.shape
  assert three == 3
  sc, c = _constants(D, scale, mutant)
  q, k, v = (_heads_first(x[:, :, i]) for i in range(3))
  if half_in:
    assert np.array_equal(round_bf16(x), x), 'half_in: qkv must hold bf16 values'
  else:
    k, v = round_bf16(k), round_bf16(v)
  if mutant == 'q_rounded_twice':
    q = round_bf16(q)
  qt = round_bf16(round_f32(q * float(c)))
  rng = perm = None
  if twin is not None:
    rng = np.random.default_rng(twin)
    perm = rng.permutation(D)

  m = np.full((B, H, N), -np.inf)
  l = np.zeros((B, H, N))
  o = np.zeros((B, H, N, D))
  with np.errstate(invalid='ignore', divide='ignore'):
    for k0 in range(0, N, KEY_BLOCK):
      key = np.arange(k0, k0 + KEY_BLOCK)
      idx = np.minimum(key, N - 1)                        # the loads are clamped, the scores masked
      valid = key < N
      if mutant == 'drop_last_key':
        valid = valid & (key != N - 1)
      if mutant == 'tail_key_twice':
        valid = valid | (key == N)
      s = np.where(valid, _dot(qt, k[:, :, idx], perm), -np.inf)
      m_new = np.maximum(m, s.max(-1))
      alpha = np.exp2(m - m_new)
      p = round_f32(np.exp2(s - m_new[..., None]))
      if rng is not None:
        p = _one_ulp(p, rng)
      pb = round_bf16(p)
      ps = (pb if mutant == 'l_from_rounded_p' else p).sum(-1)
      l = (l if mutant == 'no_alpha_on_l' else l * alpha) + ps
      if rng is not None:
        l = round_f32(l)
      o = o * alpha[..., None] + np.einsum('bhqk,bhkd->bhqd', pb, v[:, :, idx])
      m = m_new
    out = o / l[..., None]
    lse = m + (np.log(l) if mutant == 'lse_natural_log' else np.log2(l))
  out = np.moveaxis(out, 1, 2).reshape(B, N, H * D)
  if rng is not None:
    out, lse = round_f32(out), round_f32(lse)
  return dict(out=out, out_half=round_bf16(round_f32(out)), lse=lse)


def attention_vjp(qkv, out, dout, lse, scale=None, mutant=None, twin=None):
  """qkv [B, N, 3, H, 64], out / dout [B, N, H*64], lse [B, H, N] (float32-valued: what the forward saved)
  -> dqkv [B, N, 3, H, 64] float64."""
  assert mutant is None or mutant in VJP_MUTANTS, mutant
  x = np.asarray(qkv, f64)
  B, N, three, H, D = x.shape
  sc, c = _constants(D, scale, None)
  q, k, v = (_heads_first(x[:, :, i]) for i in range(3))
  o = _heads_first(np.asarray(out, f64).reshape(B, N, H, D))
  g = _heads_first(np.asarray(dout, f64).reshape(B, N, H, D))
  lse = np.asarray(lse, f64)
  qt = round_bf16(round_f32(q * float(c)))
  kb, vb, gb = round_bf16(k), round_bf16(v), round_bf16(g)
  rng = perm = None
  if twin is not None:
    rng = np.random.default_rng(twin)
    perm = rng.permutation(D)
  delta = np.zeros((B, H, N)) if mutant == 'delta_zero' else (g * o).sum(-1)
  if twin is not None:
    delta = round_f32(delta)
  s = _dot(qt, kb, perm)                                  # [B, H, q, k]
  dP = _dot(gb, vb, perm)
  P = round_f32(np.exp2(s - lse[..., None]))
  if rng is not None:
    P = _one_ulp(P, rng)
  dS = round_f32(P * round_f32(dP - delta[..., None]))
  dSb = round_bf16(dS)
  dq = float(sc) * np.einsum('bhqk,bhkd->bhqd', dSb, kb)
  dk = (1.0 if mutant == 'dk_without_ln2' else float(LN2_F32)) * np.einsum('bhqk,bhqd->bhkd', dSb, qt)
  dv = np.einsum('bhqk,bhqd->bhkd', P if mutant == 'dv_from_unrounded_p' else round_bf16(P), gb)
  dqkv = np.stack([np.moveaxis(t, 1, 2) for t in (dq, dk, dv)], axis=2)
  return dqkv if twin is None else round_f32(dqkv)


# ---- the inputs and the comparison both test files share ---------------------------------------------
# (B, N, H, scale, factor on Q): every N around a 32-query wave, a 64-key block and a 128-query workgroup;
# Q x 2 is the sharp softmax of test_attention, Q x 0.1 a near-uniform one
FORWARD_CASES = (
    (2, 1, 1, None, 2.0), (1, 7, 2, None, 2.0), (2, 31, 2, None, 2.0), (1, 32, 1, 0.2, 2.0), (1, 33, 3, None, 2.0),
    (1, 63, 1, None, 2.0), (2, 64, 1, None, 2.0), (2, 65, 3, None, 2.0), (1, 127, 2, 0.2, 2.0), (1, 128, 1, None, 2.0),
    (1, 129, 3, None, 2.0), (1, 191, 1, None, 2.0), (1, 200, 2, None, 2.0), (1, 200, 3, 0.09, 2.0),
    (1, 257, 2, None, 2.0), (1, 1000, 1, 0.09, 2.0), (1, 1024, 1, None, 2.0), (1, 200, 2, None, 0.1),
    (1, 1024, 1, None, 0.1),
)
# the (B, N, H) of test_gpu_kernels.py::test_attention (seed 210 + N, Q x 2, default scale)
OLD_FORWARD_CASES = ((2, 200, 3), (1, 1024, 2), (3, 64, 1), (1, 129, 12), (2, 1, 1), (1, 7, 2))
VJP_CASES = (
    (2, 1, 1, None), (1, 7, 2, None), (2, 33, 2, None), (1, 64, 1, 0.2), (2, 65, 3, None), (1, 129, 2, None),
    (2, 200, 2, None), (1, 512, 3, None), (1, 200, 1, 0.09),
)
TWIN_SEEDS = tuple(range(8))
# the bf16-qkv entry runs on bf16(the case's input); at these N that input has a heavy p within the f32 noise of a
# bf16 tie (its noise bound exceeds the 5e-4 cap: an invalid case), so the entry gets another seed's input there
HALF_INPUT_SEEDS = {31: 631, 127: 727, 191: 891, 257: 1057}


def rnd(shape, seed, scale=1.0):
  g = torch.Generator().manual_seed(seed)
  return torch.randn(shape, generator=g) * scale


def forward_inputs(B, N, H, qmul=2.0, seed=None):
  qkv = rnd((B, N, 3, H, 64), 210 + N if seed is None else seed)
  qkv[:, :, 0] *= qmul
  return qkv


def vjp_inputs(B, N, H):
  qkv = rnd((B, N, 3, H, 64), 310 + N)
  qkv[:, :, 0] *= 1.5
  return qkv, rnd((B, N, H * 64), 311 + N)


def _maxabs(a):
  return float(np.abs(np.asarray(a, f64)).max())


def _maxerr(got, want):
  """max |got - want|; a non-finite got where want is finite counts as infinite."""
  d = np.abs(np.asarray(got, f64) - np.asarray(want, f64))
  return float(np.where(np.isnan(d), np.inf, d).max())


def forward_twins(qkv, scale=None, half_in=False):
  return [attention_forward(qkv, scale, half_in=half_in, twin=s) for s in TWIN_SEEDS]


def vjp_twins(qkv, out, dout, lse, scale=None):
  return [attention_vjp(qkv, out, dout, lse, scale, twin=s) for s in TWIN_SEEDS]


def forward_tolerances(ref, twins, vmax):
  """(out tolerance, lse tolerance) of one input, from the model and its noise twins alone:
  8 x max|model - twin| + 2^-22 max|v| (the margin of 8 for exp2 results further than one ulp apart and
  for p values that flip in the kernel but in none of the twins; 2^-22 for the f32 accumulators the model keeps
  in float64).  An input on which that exceeds 5e-4 max|v| does not test anything: it fails."""
  tol = 8.0 * max(_maxerr(t['out'], ref['out']) for t in twins) + 2.0 ** -22 * vmax
  assert tol <= 5e-4 * vmax, f'invalid case: noise bound {tol:.3e} above 5e-4 x max|v| = {5e-4 * vmax:.3e}'
  lse_tol = min(8.0 * max(_maxerr(t['lse'], ref['lse']) for t in twins) + 2.0 ** -20, 1e-4)
  return tol, lse_tol


def check_forward(name, out, lse, ref, tols):
  """out [B, N, H*64] (f32 result) and lse (or None) against the model; prints the figures, then asserts."""
  tol, lse_tol = tols
  err = _maxerr(out, ref['out'])
  at = np.unravel_index(np.argmax(np.nan_to_num(np.abs(np.asarray(out, f64) - ref['out']), nan=np.inf)), ref['out'].shape)
  msg = f'[attention] {name}: max|out - model| {err:.3e} at {tuple(int(i) for i in at)} (tol {tol:.3e})'
  lerr = None
  if lse is not None:
    lerr = _maxerr(lse, ref['lse'])
    msg += f', max|lse - model| {lerr:.3e} (tol {lse_tol:.3e})'
  print(msg)
  assert err <= tol, msg
  assert lerr is None or lerr <= lse_tol, msg
  return err, lerr


def check_forward_half(name, out_half, ref, tols):
  """A bf16 result: it must be the rounding of SOME value within the tolerance of the model (rounding is
  monotonic: bf16(model - tol) <= result <= bf16(model + tol))."""
  tol = tols[0]
  got = np.asarray(out_half, f64)
  lo = round_bf16(round_f32(ref['out'] - tol))
  hi = round_bf16(round_f32(ref['out'] + tol))
  bad = ~((got >= lo) & (got <= hi))
  flips = int((got != ref['out_half']).sum())
  print(f'[attention] {name}: {flips} of {got.size} bf16 outputs are not the model\'s own rounding, '
        f'{int(bad.sum())} outside the roundings of model +- {tol:.3e}')
  assert not bad.any(), f'{name}: {int(bad.sum())} of {got.size} bf16 outputs outside bf16(model +- {tol:.3e})'


def vjp_tolerances(ref, twins):
  """Per gradient (dq, dk, dv): min(8 x max|model - twin| + 2^-22 range, 2e-3 range), range = max|model|."""
  tols = []
  for i in range(3):
    rng = _maxabs(ref[:, :, i])
    tols.append(min(8.0 * max(_maxerr(t[:, :, i], ref[:, :, i]) for t in twins) + 2.0 ** -22 * rng, 2e-3 * rng))
  return tols


def check_vjp(name, dqkv, ref, tols):
  errs, ok = [], True
  for i, g in enumerate(('dq', 'dk', 'dv')):
    err = _maxerr(np.asarray(dqkv)[:, :, i], ref[:, :, i])
    rng = _maxabs(ref[:, :, i])
    print(f'[attention vjp] {name} {g}: max|d| {err:.3e} = {err / max(rng, 1e-300):.2e} of the range (tol {tols[i]:.3e})')
    errs.append(err)
    ok = ok and err <= tols[i]
  assert ok, f'{name}: max errors {errs} vs tolerances {tols}'
  return errs
