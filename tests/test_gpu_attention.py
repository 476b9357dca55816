"""The attention kernels (vit_ops.hip: attention_kernel<HIN>; vit_bwd.hip: attention_bwd_dq_kernel,
attention_bwd_dkv_kernel) against their host restatement, tests/attention_reference.py.

Every tolerance is computed from the reference alone (the model against its noise twin, see
attention_reference.forward_tolerances / vjp_tolerances); tests/test_attention_reference.py shows on the CPU that
the same comparison rejects each named mutant of the model.  Observed maxima: tests/README.md."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_reference as ar
import helpers
from snap_amd import _lib, ops, ops_bwd

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


def G(t):
  return t.to(DEV).contiguous()


def _np(t):
  return t.detach().float().cpu().numpy()


def _case_id(c):
  return '-'.join(str(x) for x in c)


@pytest.mark.parametrize('case', ar.FORWARD_CASES, ids=_case_id)
def test_forward_entries_match_the_model(case):
  """All four entries on one input: ops.attention f32, with lse, bf16-only output, bf16 qkv."""
  B, N, H, scale, qmul = case
  qkv = ar.forward_inputs(B, N, H, qmul)
  vmax = float(qkv[:, :, 2].abs().max())
  ref = ar.attention_forward(qkv.numpy(), scale)
  tols = ar.forward_tolerances(ref, ar.forward_twins(qkv.numpy(), scale), vmax)
  out = ops.attention(G(qkv), scale)
  out2, lse = ops.attention(G(qkv), scale, want_lse=True)
  name = f'B{B} N{N} H{H} scale {scale} Q x {qmul}'
  ar.check_forward(name, _np(out), _np(lse), ref, tols)
  assert torch.equal(out, out2)
  half = ops.attention(G(qkv), scale, out_half=True)
  assert half.dtype == torch.bfloat16 and torch.equal(half, out.to(torch.bfloat16))
  ar.check_forward_half(name + ' bf16 out', _np(half), ref, tols)
  # the bf16-qkv entry (the kernel C5 inference runs) against the model in ITS form, with its own noise bound
  qh = ar.forward_inputs(B, N, H, qmul, seed=ar.HALF_INPUT_SEEDS.get(N)).to(torch.bfloat16)
  vmax = float(qh[:, :, 2].float().abs().max())
  ref_h = ar.attention_forward(qh.float().numpy(), scale, half_in=True)
  tols_h = ar.forward_tolerances(ref_h, ar.forward_twins(qh.float().numpy(), scale, half_in=True), vmax)
  got_h = ops.attention(G(qh), scale, out_half=True)
  assert got_h.dtype == torch.bfloat16
  # (on bf16 values the two forms are the same arithmetic: q rounds to itself before its scaling)
  assert torch.equal(got_h, ops.attention(G(qh.float()), scale, out_half=True))
  ar.check_forward_half(name + ' bf16 qkv', _np(got_h), ref_h, tols_h)


def _float64_softmax(qkv, scale=None):
  """P [B, H, q, k] in float64 from the operands the kernel multiplies."""
  x = qkv.double().numpy()
  sc, c = ar._constants(64, scale, None)
  qt = ar.round_bf16(ar.round_f32(ar._heads_first(x[:, :, 0]) * float(c)))
  k = ar.round_bf16(ar._heads_first(x[:, :, 1]))
  s = np.einsum('bhqd,bhkd->bhqk', qt, k)
  return s, np.exp2(s - s.max(-1, keepdims=True)) / np.exp2(s - s.max(-1, keepdims=True)).sum(-1, keepdims=True)


@pytest.mark.parametrize('N', [65, 129, 200])
def test_probability_readout(N):
  """V[j] = one_hot(j - 64 blk) for the keys of block blk (zero elsewhere): every product of the PV matrix-core
  pass is with an exact 1, so out[q, c] IS the kernel's probability of key 64 blk + c -- one launch per key
  block reads the whole softmax matrix.  Each entry within bf16's half-ulp (2^-8 P) of the float64 softmax of
  the rounded operands, rows summing to one within 2^-8; a wrong tail mask is a 100 % error of one column."""
  B, H = 1, 2
  qkv = ar.forward_inputs(B, N, H, seed=400 + N)
  _, P = _float64_softmax(qkv)
  got = np.zeros_like(P)
  for blk in range((N + 63) // 64):
    n = min(64, N - 64 * blk)
    x = qkv.clone()
    x[:, :, 2] = 0.0
    x[:, 64 * blk:64 * blk + n, 2] = torch.eye(64)[:n][None, :, None, :]
    out = _np(ops.attention(G(x))).astype(np.float64).reshape(B, N, H, 64)
    assert (out[..., n:] == 0).all(), 'a key past N (or of another block) received weight'
    got[:, :, :, 64 * blk:64 * blk + n] = np.moveaxis(out, 2, 1)[..., :n]
  d = np.abs(got - P)
  print(f'[attention readout] N{N}: max |P_kernel - P| / P = {(d / np.maximum(P, 1e-300))[P > 2.0 ** -22].max():.3e}, '
        f'max |row sum - 1| = {np.abs(got.sum(-1) - 1).max():.3e}')
  assert (d <= 2.0 ** -8 * P + 2.0 ** -30).all()
  assert (np.abs(got.sum(-1) - 1) <= 2.0 ** -8).all()


def _hadamard64():
  h = np.ones((1, 1))
  while h.shape[0] < 64:
    h = np.block([[h, h], [h, -h]])
  return h


@pytest.mark.parametrize('N', [65, 200])
def test_one_hot_selection_is_bitwise(N):
  """Keys and queries are +-1 rows of a 64 x 64 Hadamard matrix times a power of two: q~ = +-bf16(32 c), every
  score is an exact f32 multiple of it, the target's is 64 g (~ 369 base-2 units), every other key's is 0
  (another row; the fillers all carry row 0) -- 2^-369 is exactly 0 in f32.  So p = 1 for one key, l = 1 and
  out == bf16(v[target]) bit for bit.  Targets: the first key, the last key of the ragged tail, both sides of
  every block boundary; every query block meets targets in earlier and later blocks (a later one must erase
  the earlier blocks' sums through alpha = 0)."""
  B, H = 2, 2
  had = _hadamard64()
  spots = sorted({0, 1, N - 1, N - 2} | {b for b in (63, 64, 127, 128, 191, 192) if b < N})
  assert len(spots) <= 63
  k = np.tile(had[0], (N, 1))
  for i, t in enumerate(spots):
    k[t] = had[1 + i]
  target = np.array([spots[(5 * q + q // 64) % len(spots)] for q in range(N)])
  q = 32.0 * k[target]
  blocks = {(qq // 64, int(target[qq]) // 64) for qq in range(N)}
  assert any(tb < qb for qb, tb in blocks) and any(tb > qb for qb, tb in blocks)
  v = ar.rnd((B, N, H, 64), 77)
  qkv = torch.zeros((B, N, 3, H, 64))
  qkv[:, :, 0] = torch.from_numpy(q).float()[None, :, None, :]
  qkv[:, :, 1] = torch.from_numpy(k).float()[None, :, None, :]
  qkv[:, :, 2] = v
  s, _ = _float64_softmax(qkv)
  top = s[0, 0, np.arange(N), target]
  others = np.where(np.arange(N)[None, :] == target[:, None], -np.inf, s[0, 0])
  assert (top - others.max(-1) >= 160).all()
  want = v[:, target].reshape(B, N, H * 64).to(torch.bfloat16)
  out, lse = ops.attention(G(qkv), want_lse=True)
  assert torch.equal(out.cpu(), want.float())
  assert torch.equal(lse.cpu(), torch.from_numpy(top).float()[None, None].expand(B, H, N))      # l = 1: lse = m
  assert torch.equal(ops.attention(G(qkv), out_half=True).cpu(), want)
  assert torch.equal(ops.attention(G(qkv.to(torch.bfloat16)), out_half=True).cpu(), want)


@pytest.mark.parametrize('case', ar.VJP_CASES, ids=_case_id)
def test_vjp_matches_the_model(case):
  """dqkv against the model VJP fed with the forward's own out / lse; two runs bit-equal (no atomics)."""
  B, N, H, scale = case
  qkv, dout = ar.vjp_inputs(B, N, H)
  out, lse = ops.attention(G(qkv), scale, want_lse=True)
  dqkv = ops_bwd.attention_bwd(G(qkv), out, G(dout), lse, scale)
  assert torch.equal(dqkv, ops_bwd.attention_bwd(G(qkv), out, G(dout), lse, scale))
  args = (qkv.numpy(), _np(out), dout.numpy(), _np(lse), scale)
  ref = ar.attention_vjp(*args)
  tols = ar.vjp_tolerances(ref, ar.vjp_twins(*args))
  ar.check_vjp(f'B{B} N{N} H{H} scale {scale}', _np(dqkv), ref, tols)


@pytest.mark.parametrize('N', [65, 129, 200])
def test_dv_probability_readout(N):
  """dout[q] = one_hot(q - 64 b) for the queries of block b: dv[k, c] = bf16(P[64 b + c, k]) -- the dk/dv
  kernel's probabilities entry by entry, its query-tail mask (columns of queries past N stay exactly 0) and its
  key-tail mask.  P = 2^(s - lse) from the lse the forward saved, in float64."""
  B, H = 1, 2
  qkv = ar.forward_inputs(B, N, H, qmul=1.5, seed=500 + N)
  out, lse = ops.attention(G(qkv), want_lse=True)
  s, _ = _float64_softmax(qkv)
  P = np.exp2(s - _np(lse).astype(np.float64)[..., None])          # [B, H, q, k]
  worst = 0.0
  for b in range((N + 63) // 64):
    n = min(64, N - 64 * b)
    dout = torch.zeros((B, N, H, 64))
    dout[:, 64 * b:64 * b + n] = torch.eye(64)[:n][None, :, None, :]
    dv = _np(ops_bwd.attention_bwd(G(qkv), out, G(dout.reshape(B, N, H * 64)), lse)[:, :, 2]).astype(np.float64)
    assert (dv[..., n:] == 0).all(), 'a query past N (or of another block) reached dv'
    want = np.moveaxis(P[:, :, 64 * b:64 * b + n, :], (1, 2, 3), (2, 3, 1))      # [B, k, H, c]
    d = np.abs(dv[..., :n] - want)
    worst = max(worst, float((d / np.maximum(want, 1e-300))[want > 2.0 ** -22].max()))
    # bf16's half-ulp on P, P itself through f32 exp2 of an f32 difference (2^-20 is generous)
    assert (d <= (2.0 ** -8 + 2.0 ** -20) * want + 2.0 ** -30).all()
  print(f'[attention dv readout] N{N}: max |dv - P| / P = {worst:.3e}')


def _slices(B, H):
  return [(b, h) for b in range(B) for h in range(H)]


@pytest.mark.parametrize('what', ['v', 'q'])
@pytest.mark.parametrize('poison', [float('nan'), float('inf'), float('-inf')])
def test_non_finite_values_stay_in_their_batch_and_head(what, poison):
  """A NaN / +-inf in one row of v (or q) of ONE (batch, head): every other slice of out, lse and dqkv keeps the
  bits of the clean run; the poisoned slice is NaN wherever torch float64 is."""
  B, N, H = 2, 70, 3
  pb, ph, row, ch = 1, 1, 68, 3
  qkv, dout = ar.vjp_inputs(B, N, H)

  def run(x):
    out, lse = ops.attention(G(x), want_lse=True)
    return out, lse, ops_bwd.attention_bwd(G(x), out, G(dout), lse)
  clean = run(qkv)
  bad_in = qkv.clone()
  bad_in[pb, row, 2 if what == 'v' else 0, ph, ch] = poison
  bad = run(bad_in)
  for b, h in _slices(B, H):
    if (b, h) == (pb, ph):
      continue
    assert torch.equal(bad[0][b, :, 64 * h:64 * h + 64], clean[0][b, :, 64 * h:64 * h + 64]), (b, h)
    assert torch.equal(bad[1][b, h], clean[1][b, h]), (b, h)
    assert torch.equal(bad[2][b, :, :, h], clean[2][b, :, :, h]), (b, h)
  leaves = [bad_in[pb, :, i, ph].double().requires_grad_(True) for i in range(3)]
  ref = F.scaled_dot_product_attention(*(t[None] for t in leaves))[0]
  ref.backward(dout[pb, :, 64 * ph:64 * ph + 64].double())
  got_out = bad[0][pb, :, 64 * ph:64 * ph + 64].cpu()
  assert torch.isnan(got_out)[torch.isnan(ref.detach())].all()
  for i in range(3):
    want_nan = torch.isnan(leaves[i].grad)
    assert torch.isnan(bad[2][pb, :, i, ph].cpu())[want_nan].all(), ('dq', 'dk', 'dv')[i]


def test_entries_write_inside_their_output_only():
  """Each snap_attention_* entry through the C ABI with its outputs inside canary-filled buffers at a ragged
  N: the bytes around [B, N, H*64] (and [B, H, N] of lse) are untouched."""
  lib = _lib.load()
  B, N, H, pad = 2, 70, 3, 256
  qkv = G(ar.forward_inputs(B, N, H))
  qh = qkv.to(torch.bfloat16)
  n = B * N * H * 64
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  P = lambda t: ctypes.c_void_p(t.data_ptr())

  def canary(count, dtype):
    buf = torch.full((pad + count + pad,), -7.25, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + count]

  def untouched(buf, count):
    return bool((buf[:pad] == -7.25).all()) and bool((buf[pad + count:] == -7.25).all())

  want = ops.attention(qkv)
  buf, view = canary(n, torch.float32)
  assert lib.snap_attention_bf16_f32(P(qkv), P(view), B, N, H, 64, ctypes.c_float(0.125), stream) == 0
  assert untouched(buf, n) and torch.equal(view.reshape(B, N, H * 64), want)
  buf, view = canary(n, torch.float32)
  lbuf, lview = canary(B * H * N, torch.float32)
  assert lib.snap_attention_lse_bf16_f32(P(qkv), P(view), P(lview), B, N, H, 64, ctypes.c_float(0.125), stream) == 0
  assert untouched(buf, n) and untouched(lbuf, B * H * N) and torch.equal(view.reshape(B, N, H * 64), want)
  buf, view = canary(n, torch.bfloat16)
  assert lib.snap_attention_bf16out_f32(P(qkv), P(view), B, N, H, 64, ctypes.c_float(0.125), stream) == 0
  assert untouched(buf, n) and torch.equal(view.reshape(B, N, H * 64), want.to(torch.bfloat16))
  buf, view = canary(n, torch.bfloat16)
  assert lib.snap_attention_bf16io(P(qh), P(view), B, N, H, 64, ctypes.c_float(0.125), stream) == 0
  assert untouched(buf, n) and torch.equal(view.reshape(B, N, H * 64), ops.attention(qh, out_half=True))
  # the VJP: dqkv and delta inside canaries
  dout = G(ar.rnd((B, N, H * 64), 9))
  out, lse = ops.attention(qkv, want_lse=True)
  buf, view = canary(3 * n, torch.float32)
  dbuf, dview = canary(B * H * N, torch.float32)
  assert lib.snap_attention_bwd_bf16_f32(P(qkv), P(out), P(dout), P(lse), P(dview), P(view), B, N, H, 64,
                                         ctypes.c_float(0.125), stream) == 0
  assert untouched(buf, 3 * n) and untouched(dbuf, B * H * N)
  assert torch.equal(view.reshape(B, N, 3, H, 64), ops_bwd.attention_bwd(qkv, out, dout, lse))
