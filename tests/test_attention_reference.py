"""The host restatement of the attention kernels (tests/attention_reference.py) against float64 maths, and the
teeth of the tolerances tests/test_gpu_attention.py computes from it: every named mutant of the model is
rejected by the very comparison the GPU test applies to the kernels.  CPU only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_reference as ar
from oracle import vit as o_vit

OLD_TOL = 4e-3           # test_gpu_kernels.py::test_attention: atol = 4e-3 * max|v| against oracle/vit.attention


def _case_id(c):
  return '-'.join(str(x) for x in c)


def _exact(qkv, scale):
  """float64 softmax attention on the operands the kernel multiplies (q~ / c, bf16 k, bf16 v):
  (P [B, H, q, k], out [B, N, H*64], base-2 lse [B, H, q], the operands [B, H, N, 64])."""
  x = np.asarray(qkv, np.float64)
  B, N, _, H, D = x.shape
  sc, c = ar._constants(D, scale, None)
  q, k, v = (ar._heads_first(x[:, :, i]) for i in range(3))
  qt = ar.round_bf16(ar.round_f32(q * float(c)))
  k, v = ar.round_bf16(k), ar.round_bf16(v)
  s = np.einsum('bhqd,bhkd->bhqk', qt, k)
  m = s.max(-1, keepdims=True)
  e = np.exp2(s - m)
  l = e.sum(-1, keepdims=True)
  P = e / l
  out = np.moveaxis(P @ v, 1, 2).reshape(B, N, H * D)
  return P, out, (m + np.log2(l))[..., 0], (qt / float(c), k, v, float(sc))


def _merge(t):
  """[B, H, N, D] -> [B, N, H*D]"""
  B, H, N, D = t.shape
  return np.moveaxis(t, 1, 2).reshape(B, N, H * D)


def test_round_bf16_is_torchs_conversion():
  g = torch.Generator().manual_seed(5)
  x = torch.randn(20000, generator=g) * torch.exp2(torch.randint(-140, 128, (20000,), generator=g).float())
  ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.3895313892515355e38, 3.4e38, 1e-40, -0.0, 0.0,
                       float('inf'), float('-inf')])
  x = torch.cat([x, ties])
  want = x.to(torch.bfloat16).double().numpy()
  got = ar.round_bf16(x.double().numpy())
  assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
  assert np.isnan(ar.round_bf16(np.array([np.nan]))).all()


@pytest.mark.parametrize('case', ar.FORWARD_CASES, ids=_case_id)
def test_model_forward_is_within_the_derivable_distance_of_float64(case):
  """|model - float64 softmax| <= 2^-8 sum_j P_j |v_j|: a half-ulp of bf16 is at most 2^-8 of the value (8
  significant bits; observed 3.9e-3 on single probabilities), the normalisation adds nothing of that size (l
  sums the unrounded p), + 2^-20 max|v| for the f32 roundings of p.  The float64 side
  is oracle/vit.attention(bf16_operands=True) and torch's scaled_dot_product_attention."""
  B, N, H, scale, qmul = case
  qkv = ar.forward_inputs(B, N, H, qmul).numpy()
  vmax = float(np.abs(qkv[:, :, 2]).max())
  ref = ar.attention_forward(qkv, scale)
  P, out64, lse64, (q, k, v, sc) = _exact(qkv, scale)
  bound = 2.0 ** -8 * _merge(P @ np.abs(v)) + 2.0 ** -20 * vmax
  oracle = o_vit.attention(qkv.astype(np.float64), scale, bf16_operands=True)
  sdpa = F.scaled_dot_product_attention(*(torch.from_numpy(t) for t in (q, k, v)), scale=sc)
  sdpa = _merge(sdpa.numpy())
  # (the float64 sides differ by the f32 rounding of c = scale * log2(e): 2^-24 of the logits)
  sides = [('sdpa', sdpa)]
  assert np.abs(sdpa - out64).max() < 1e-6
  # the oracle forms c from the float64 scale, the kernel from the f32 one: for a scale that is not a power of two
  # the two c can differ in the last bit and round a q on a bf16 tie apart -- compared where they are equal
  if np.float32((64 ** -0.5 if scale is None else scale) * 1.4426950408889634) == ar._constants(64, scale, None)[1]:
    assert np.abs(oracle - out64).max() < 1e-6
    sides.append(('oracle', oracle))
  else:
    print(f'[model] {case}: the oracle scales q by another float32 than the kernel')
  assert scale is not None or len(sides) == 2
  for name, want in sides:
    d = np.abs(ref['out'] - want)
    print(f'[model] {case} vs {name}: max|d| {d.max():.3e}, largest share of its bound {(d / bound).max():.3f}')
    assert (d <= bound).all(), (name, float((d / bound).max()))
  assert np.abs(ref['lse'] - lse64).max() <= 1e-6          # (l sums f32-rounded p: 2^-24 relative)
  assert np.array_equal(ref['out_half'], ar.round_bf16(ar.round_f32(ref['out'])))


def test_model_forward_bf16_qkv_form():
  """The HIN form on a bf16 qkv = the f32 form on the same values except that q is rounded before AND after
  its scaling; on an f32 qkv the two differ (that is the `q_rounded_twice` mutant)."""
  qkv = ar.forward_inputs(2, 65, 2).numpy()
  qh = ar.round_bf16(qkv)
  a = ar.attention_forward(qh, half_in=True)
  b = ar.attention_forward(qh)
  assert np.array_equal(a['out'], b['out'])
  assert np.array_equal(a['out'], ar.attention_forward(qkv, mutant='q_rounded_twice')['out'])
  with pytest.raises(AssertionError):
    ar.attention_forward(qkv, half_in=True)


@pytest.mark.parametrize('case', ar.VJP_CASES, ids=_case_id)
def test_model_vjp_is_within_the_derivable_distance_of_torch_autograd(case):
  """torch fp64 autograd of softmax attention on the multiplied operands, cotangent bf16(dout).  First-order
  bound from the model's rounding points: bf16(P), bf16(dS) (2^-8 each), P itself (lse and the model's l in
  f32: 2^-18 is generous), and delta = sum dout * out, which sees the UNROUNDED dout and the model's out
  (|out - exact| <= 2^-8 sum_j P_j |v_j| + its f32 rounding); 1 % on top for the second order."""
  B, N, H, scale = case
  qkv, dout = (t.numpy() for t in ar.vjp_inputs(B, N, H))
  fwd = ar.attention_forward(qkv, scale)
  out32, lse32 = fwd['out'].astype(np.float32), fwd['lse'].astype(np.float32)
  got = ar.attention_vjp(qkv, out32, dout, lse32, scale)
  P, out64, _, (q, k, v, sc) = _exact(qkv, scale)
  g = ar._heads_first(dout.astype(np.float64).reshape(B, N, H, 64))
  gb = ar.round_bf16(g)
  leaves = [torch.from_numpy(t).requires_grad_(True) for t in (q, k, v)]
  F.scaled_dot_product_attention(*leaves, scale=sc).backward(torch.from_numpy(gb))
  want = [t.grad.numpy() for t in leaves]
  o64 = ar._heads_first(out64.reshape(B, N, H, 64))
  e_out = 2.0 ** -8 * (P @ np.abs(v)) + 2.0 ** -23 * np.abs(o64)
  e_delta = (np.abs(g - gb) * np.abs(o64) + np.abs(g) * e_out).sum(-1)
  dS = P * (gb @ np.swapaxes(v, -1, -2) - (gb * o64).sum(-1)[..., None])
  e_p = 2.0 ** -18
  e_dS = np.abs(dS) * (2.0 ** -8 + e_p + 2.0 ** -22) + P * e_delta[..., None]
  bounds = [sc * (e_dS @ np.abs(k)), sc * (np.swapaxes(e_dS, -1, -2) @ np.abs(q)),
            (2.0 ** -8 + e_p) * (np.swapaxes(P, -1, -2) @ np.abs(gb))]
  for i, name in enumerate(('dq', 'dk', 'dv')):
    w = np.moveaxis(want[i], 1, 2)
    bound = 1.01 * np.moveaxis(bounds[i], 1, 2) + 2.0 ** -20 * np.abs(w).max()
    d = np.abs(got[:, :, i] - w)
    print(f'[model vjp] {case} {name}: max|d| {d.max():.3e} = {d.max() / max(np.abs(w).max(), 1e-300):.2e} of the range, '
          f'largest share of its bound {(d / bound).max():.3f}')
    assert (d <= bound).all(), (name, float((d / bound).max()))


@pytest.mark.parametrize('case', ar.FORWARD_CASES, ids=_case_id)
def test_forward_tolerances_reject_every_mutant(case):
  """On every input of the GPU test: the noise bound is valid (<= 5e-4 max|v|), the noise twin passes the
  GPU test's comparison, and each mutant that changes the result at this shape fails it."""
  B, N, H, scale, qmul = case
  qkv = ar.forward_inputs(B, N, H, qmul).numpy()
  vmax = float(np.abs(qkv[:, :, 2]).max())
  ref = ar.attention_forward(qkv, scale)
  twins = ar.forward_twins(qkv, scale)
  tols = ar.forward_tolerances(ref, twins, vmax)
  print(f'[tolerance] {case}: out {tols[0]:.3e} = {tols[0] / vmax:.2e} max|v|, lse {tols[1]:.3e}')
  for twin in twins:
    ar.check_forward('noise twin', twin['out'], twin['lse'], ref, tols)
    ar.check_forward_half('noise twin', twin['out_half'], ref, tols)
  # the bf16-qkv entry's input: its bound is valid too
  qh = ar.round_bf16(ar.forward_inputs(B, N, H, qmul, seed=ar.HALF_INPUT_SEEDS.get(N)).numpy())
  ar.forward_tolerances(ar.attention_forward(qh, scale, half_in=True), ar.forward_twins(qh, scale, half_in=True),
                        float(np.abs(qh[:, :, 2]).max()))
  changed = 0
  for mutant in ar.FORWARD_MUTANTS:
    bad = ar.attention_forward(qkv, scale, mutant=mutant)
    if all(np.array_equal(bad[n], ref[n], equal_nan=True) for n in ('out', 'lse')):
      print(f'[mutant] {mutant} changes nothing at {case}')
      continue
    changed += 1
    with pytest.raises(AssertionError):
      ar.check_forward(mutant, bad['out'], bad['lse'], ref, tols)
  assert changed >= (2 if N == 1 else 5)


@pytest.mark.parametrize('case', ar.VJP_CASES, ids=_case_id)
def test_vjp_tolerances_reject_every_mutant(case):
  B, N, H, scale = case
  qkv, dout = (t.numpy() for t in ar.vjp_inputs(B, N, H))
  fwd = ar.attention_forward(qkv, scale)
  out32, lse32 = fwd['out'].astype(np.float32), fwd['lse'].astype(np.float32)
  ref = ar.attention_vjp(qkv, out32, dout, lse32, scale)
  twins = ar.vjp_twins(qkv, out32, dout, lse32, scale)
  tols = ar.vjp_tolerances(ref, twins)
  for twin in twins:
    ar.check_vjp('noise twin', twin, ref, tols)
  changed = 0
  for mutant in ar.VJP_MUTANTS:
    bad = ar.attention_vjp(qkv, out32, dout, lse32, scale, mutant=mutant)
    if np.array_equal(bad, ref):
      print(f'[mutant] {mutant} changes nothing at {case}')
      continue
    changed += 1
    with pytest.raises(AssertionError):
      ar.check_vjp(mutant, bad, ref, tols)
  assert changed >= 2
  # a forward that saved the natural-log statistic is caught by the VJP too
  bad_lse = ar.attention_forward(qkv, scale, mutant='lse_natural_log')['lse'].astype(np.float32)
  if N > 1:
    with pytest.raises(AssertionError):
      ar.check_vjp('lse_natural_log', ar.attention_vjp(qkv, out32, dout, bad_lse, scale), ref, tols)


@pytest.mark.parametrize('B,N,H', ar.OLD_FORWARD_CASES)
def test_the_subtle_mutants_pass_the_old_bound(B, N, H):
  """Why the bound moved: on test_attention's own inputs the old comparison (4e-3 max|v| against
  oracle/vit.attention on rounded operands) accepts a sum of rounded probabilities, a truncated log2(e) and a
  twice-rounded q -- each of which the model-based comparison rejects wherever it changes the result."""
  qkv = ar.forward_inputs(B, N, H).numpy()
  vmax = float(np.abs(qkv[:, :, 2]).max())
  oracle = o_vit.attention(qkv.astype(np.float64), None, bf16_operands=True)
  ref = ar.attention_forward(qkv)
  for mutant in ('l_from_rounded_p', 'log2e_bf16', 'q_rounded_twice'):
    bad = ar.attention_forward(qkv, mutant=mutant)
    err = float(np.abs(bad['out'] - oracle).max())
    print(f'[old bound] {mutant} B{B} N{N} H{H}: {err:.3e} vs {OLD_TOL * vmax:.3e}; vs the model '
          f'{np.abs(bad["out"] - ref["out"]).max():.3e}')
    # the one exception: q rounded twice at (2, 200, 3) is 5 % OVER the old bound (1.82e-2 vs 1.73e-2), so
    # test_attention would have caught it there; recorded rather than forced (tests/README.md)
    if (mutant, B, N, H) == ('q_rounded_twice', 2, 200, 3):
      assert OLD_TOL * vmax < err <= 1.1 * OLD_TOL * vmax
    else:
      assert err <= OLD_TOL * vmax, mutant


def test_an_lse_off_by_a_hundredth_passed_the_old_bound_and_fails_the_new_one():
  """test_attention_bwd allows 2e-2 absolute on lse; the model's own lse is within 1e-6 of float64, and the new
  bound (<= 1e-4) rejects a statistic that is off by 1e-2."""
  qkv = ar.forward_inputs(1, 129, 3).numpy()
  ref = ar.attention_forward(qkv)
  tols = ar.forward_tolerances(ref, ar.forward_twins(qkv), float(np.abs(qkv[:, :, 2]).max()))
  assert tols[1] <= 1e-4 and 1e-2 <= 2e-2
  with pytest.raises(AssertionError):
    ar.check_forward('lse + 1e-2', ref['out'], ref['lse'] + 1e-2, ref, tols)
  assert math.isclose(float(ar.LN2_F32), math.log(2.0), rel_tol=1e-7)
