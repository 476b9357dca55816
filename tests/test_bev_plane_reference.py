"""The restatement of the BEV plane family (tests/bev_plane_reference.py) alone: its float64 definitions agree with
the numpy oracle and their VJPs with torch fp64 autograd, its planted cases are what their names say, its f32 models
stay within half of their bounds, and the comparison functions of tests/test_gpu_bev_plane.py reject the named
mutants of the models.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bev_plane_reference as R
import oracle_ops
import test_gpu_bev_plane as G
from oracle import bev as o_bev

f32 = np.float32
POOL = {c['name']: c for c in R.pool_cases()}
FUSE = {c['name']: c for c in R.fuse_cases()}
CPOOL = {c['name']: c for c in R.conf_pool_cases()}


# ------------------------------- the models as a kernel would answer --------------------------
def model_pool(c, pooling, mutant=None):
  vol, valid, g = c['vol'], c['valid'], c['dplane']
  plane, pv = R.pool_32(vol, valid, pooling, mutant)
  got = dict(plane=plane, pvalid=pv, dvol=R.share_32(vol, valid, g, pooling, mutant))
  if R.pool_kernel(vol.shape[1], vol.shape[2], pooling, True) == 'vertical_pool_max_arg_kernel':
    argz, ties = R.record_64(vol, valid, mutant)
    got.update(plane_arg=plane, pvalid_arg=pv, argz=argz, ties=ties, dvol_arg=got['dvol'])
  return got


def model_fuse(c, pooling, mutant=None):
  head = (c['Wm'], c['bm'], c['normalize'], c['eps'])
  fused, fvalid, matching = R.fuse_32(c['planes'], c['valids'], pooling, *head, mutant=mutant)
  got = dict(fused=fused, fvalid=fvalid, matching=matching, vjp={})
  for dm, dfu in G.VJP_VARIANTS:
    if dm and c['Wm'] is None:
      continue
    dplanes, dy = R.fuse_vjp_32(c['planes'], c['valids'], pooling, *head, c['dmatching'] if dm else None,
                                c['dfused'] if dfu else None, mutant=mutant)
    got['vjp'][dm, dfu] = (list(dplanes), dy)
  return got


def model_conf_head(c):
  f = c['f'] if c['valid'] is None else np.where(c['valid'][:, None], c['f'], f32(0))
  df, prod, ds = R.conf_head_vjp_32(f, c['valid'], c['w'], c['b'], c['g'])
  return dict(out=R.conf_head_32(f, c['valid'], c['w'], c['b'])[0], df=df, dw=prod.astype(np.float64).sum(0).astype(f32),
              db=ds.astype(np.float64).sum(keepdims=True).astype(f32))


def model_conf_pool(c, log_sig, mutant=None):
  plane, pv, s, p = R.conf_pool_32(c['vol'], c['valid'], c['w'], c['b'], log_sig, mutant)
  p32 = G.conf_pool_expected(c['name'], bool(log_sig))['weights32']
  dvol, ds = R.conf_pool_vjp_32(c['vol'], c['w'], c['b'], p32, c['dplane'], log_sig)
  dw = (ds.astype(np.float64)[..., None] * c['vol']).sum((0, 1)).astype(f32)
  return dict(plane=plane, pvalid=pv, scores=s, weights=p, dvol=dvol, dw=dw, db=ds.astype(np.float64).sum().reshape(1).astype(f32))


# ------------------------------- the float64 definitions --------------------------------------
def _t(a):
  return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('name', [n for n in POOL if n.startswith(('scene', 'shape'))])
def test_pooling_definition_agrees_with_the_oracle(name):
  c = POOL[name]
  vol = np.where(c['valid'][..., None], c['vol'], f32(0))      # (the oracle multiplies invalid levels by zero)
  for pooling in R.POOLINGS:
    want, wv = oracle_ops.vertical_pool(_t(vol), _t(c['valid']), pooling)
    got, gv = R.reduce_64(vol, c['valid'], pooling)
    assert np.array_equal(gv, wv.numpy())
    assert np.abs(got - want.numpy()).max() <= 1e-5 * max(1.0, np.abs(got).max())


@pytest.mark.parametrize('name', [n for n in FUSE if n.startswith(('scene', 'float'))])
def test_fuse_and_head_definition_agrees_with_the_oracle(name):
  c = FUSE[name]
  M = c['planes'][0].shape[0]
  v = R.stack_valids(c['valids'], M)
  planes = [np.where(v[:, p, None], x, f32(0)) for p, x in enumerate(c['planes'])]
  for pooling in R.POOLINGS:
    fused, fvalid, matching = oracle_ops.plane_fuse_match([_t(p) for p in planes], [None if q is None else _t(q) for q in c['valids']],
                                                          pooling, _t(c['Wm']), _t(c['bm']), c['normalize'], c['eps'])
    got, any_ = R.reduce_64(np.stack(planes, -2), v, pooling)
    assert np.array_equal(any_, fvalid.numpy())
    assert np.abs(got - fused.numpy()).max() <= 1e-5 * max(1.0, np.abs(got).max())
    m = R.head_64(got, c['Wm'], c['bm'], c['normalize'], c['eps'], any_)[0]
    assert np.abs(m - matching.numpy()).max() <= 2e-4 * max(1.0, np.abs(m).max())


@pytest.mark.parametrize('name', [n for n in CPOOL if n.startswith('cscene')] + ['cpool_Z33_D124_M9'])
def test_confidence_definitions_agree_with_the_oracle(name):
  c = CPOOL[name]
  vol64 = c['vol'].astype(np.float64)
  params = {'confidence_head': {'kernel': c['w'].astype(np.float64)[:, None], 'bias': c['b'].astype(np.float64)}}
  for log_sig, mode in ((False, 'softmax'), (True, 'weighted')):
    want = o_bev.vertical_pooling({'pooling': mode}, vol64, c['valid'], params)
    plane, any_, s, p, _ = R.conf_pool_64(c['vol'], c['valid'], c['w'], c['b'], log_sig)
    assert np.array_equal(any_, want['valid'])
    for a, b in ((plane, want['features']), (s, want['scores']), (p, want['weights'])):
      assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
  conf = R.conf_head_64(c['vol'][:, 0], c['valid'][:, 0], c['w'], c['b'])[0]
  s = c['vol'][:, 0].astype(np.float64) @ c['w'].astype(np.float64) + float(c['b'][0])
  assert np.abs(conf - np.where(c['valid'][:, 0], o_bev.log_sigmoid(s), 0)).max() <= 1e-14


def _rel(a, b):
  b = b.detach().numpy() if torch.is_tensor(b) else b
  return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def _torch_reduce(x, v, pooling):
  n = v.sum(-1)
  if pooling == 'max':
    out = torch.where(v[..., None], x, torch.full_like(x, -float('inf'))).amax(-2)     # (amax shares among ties)
  else:
    out = torch.where(v[..., None], x, torch.zeros_like(x)).sum(-2)
    if pooling == 'mean':
      out = out / n.clamp(min=1)[..., None]
  return torch.where(n[..., None] > 0, out, torch.zeros_like(out))


@pytest.mark.parametrize('pooling', R.POOLINGS)
def test_vjps_equal_torch_fp64_autograd(pooling):
  rng = np.random.default_rng(5)
  # pooling: continuous data, and small integers (ties within and beyond the valid levels)
  for vol in (rng.standard_normal((7, 9, 8)), rng.integers(-1, 2, (7, 9, 8)).astype(np.float64)):
    valid = rng.random((7, 9)) < 0.6
    valid[0] = False
    g = rng.standard_normal((7, 8))
    x = _t(vol).requires_grad_()
    _torch_reduce(x, _t(valid), pooling).backward(_t(g))
    assert _rel(R.reduce_vjp_64(vol, valid, g, pooling), x.grad) <= 1e-12
  # fuse + head, with and without the normalisation, covered by 0 .. 3 planes, one plane without a mask
  for normalize in (True, False):
    planes = [rng.integers(-1, 2, (12, 8)).astype(np.float64) + (0.0 if pooling == 'max' else rng.standard_normal((12, 8)))
              for _ in range(3)]
    valids = [rng.random(12) < 0.5, rng.random(12) < 0.5, None]
    Wm, bm, dm, dfu = rng.standard_normal((8, 5)), rng.standard_normal(5), rng.standard_normal((12, 5)), rng.standard_normal((12, 8))
    xs = [_t(p).requires_grad_() for p in planes]
    v = _t(R.stack_valids(valids, 12))
    fused = _torch_reduce(torch.stack(xs, -2), v, pooling)
    y = _t(bm) + fused @ _t(Wm)
    if normalize:
      nrm = y.norm(dim=-1, keepdim=True)
      y = torch.where(nrm < 1e-5, torch.zeros_like(y), y / nrm)
    any_ = v.any(-1)[:, None]
    ((torch.where(any_, y, torch.zeros_like(y)) * _t(dm)).sum() + (torch.where(any_, fused, torch.zeros_like(fused)) * _t(dfu)).sum()).backward()
    dplanes, dy = R.fuse_vjp_64(planes, valids, pooling, Wm, bm, normalize, 1e-5, dm, dfu)
    for d, x in zip(dplanes, xs):
      assert _rel(d, x.grad) <= 1e-12
  if pooling != 'max':
    return
  # the confidence head and both modes of the confidence pooling
  f, w, b, g = rng.standard_normal((9, 12)), rng.standard_normal(12), rng.standard_normal(1), rng.standard_normal(9)
  valid = rng.random(9) < 0.6
  tf, tw, tb = (_t(a).requires_grad_() for a in (f, w, b))
  (torch.where(_t(valid), torch.nn.functional.logsigmoid(tf @ tw + tb), torch.zeros(9, dtype=torch.float64)) * _t(g)).sum().backward()
  for got, want in zip(R.conf_head_vjp_64(f, valid, w, b, g)[:3], (tf.grad, tw.grad, tb.grad)):
    assert _rel(got, want) <= 1e-12
  for log_sig in (False, True):
    vol, valid, g = rng.standard_normal((6, 7, 12)), rng.random((6, 7)) < 0.6, rng.standard_normal((6, 12))
    valid[0], valid[1] = False, True
    tv, tw, tb = (_t(a).requires_grad_() for a in (vol, w, b))
    s = tv @ tw + tb
    s = torch.nn.functional.logsigmoid(s) if log_sig else s
    any_ = _t(valid.any(-1))[:, None]
    p = torch.softmax(torch.where(_t(valid) | ~any_, s, torch.full_like(s, -float('inf'))), -1) * _t(valid)
    (torch.where(any_, (p[..., None] * tv).sum(-2), torch.zeros(6, 12, dtype=torch.float64)) * _t(g)).sum().backward()
    plane, _, _, p64, _ = R.conf_pool_64(vol, valid, w, b, log_sig)
    assert _rel(p64, p) <= 1e-12
    dvol, dw, db, _ = R.conf_pool_vjp_64(vol, w, b, p64, g, log_sig)
    assert _rel(dvol, tv.grad) <= 1e-12 and _rel(dw, tw.grad) <= 1e-12
    assert abs(db[0] - float(tb.grad)) <= 1e-12 * np.abs(dw).max()      # (zero for 'softmax': the shift invariance)


# ------------------------------- the planted cases --------------------------------------------
@pytest.mark.parametrize('Z', R.BITMASK_Z)
def test_bitmask_columns_read_back_the_levels_that_entered(Z):
  c = R.bitmask_case(Z)
  assert (Z <= 64) == (R.pool_kernel(Z, c['vol'].shape[2]) == 'vertical_pool_wave_kernel')
  pats = dict(zip(c['patterns'], c['valid']))
  for k in range(min(Z, 5) + 1):
    assert pats[f'k{k}'].sum() == k
  assert pats['first'].nonzero()[0].tolist() == [0] and pats['last'].nonzero()[0].tolist() == [Z - 1]
  assert (pats['ge32'].nonzero()[0] >= 32).all() and pats['all'].all() and not pats['odd'][0::2].any()
  want = R.bitmask_expected(Z)
  for i, v in enumerate(c['valid']):
    assert [int(b) for g in range(want.shape[1]) for b in np.nonzero([(want[i, g] >> k) & 1 for k in range(16)])[0] + 16 * g] == \
        v.nonzero()[0].tolist()
  got, _ = R.reduce_64(c['vol'], c['valid'], 'sum')
  assert np.array_equal(got[:, ::4], want) and np.array_equal(R.pool_32(c['vol'], c['valid'], 'sum')[0][:, ::4], want)
  assert not np.isfinite(c['vol'][~c['valid']]).all() or c['valid'].all()


def test_tie_columns_hold_what_their_comments_say():
  seen = np.zeros(3, bool)
  for name, c in POOL.items():
    if not name.startswith('ties'):
      continue
    vol, valid = c['vol'], c['valid']
    Z = vol.shape[1]
    argz, ties = R.record_64(vol, valid)
    assert (ties[0] == Z).all() and (argz[0] == 0).all()                          # the constant column
    assert (argz[1] == Z - 1).all() and (ties[1] == 1).all() and (vol[1, 1:Z - 1] == 9).all() and not valid[1, 1:Z - 1].any()
    assert (R.reduce_64(vol, valid, 'max')[0][2] == -np.inf).all() and (argz[2] == 0).all() and (ties[2] == Z).all()
    assert argz[3, 0] == 1 and ties[3, 0] == 2 and (ties[3, 1:4] >= 1).all()     # ranks 1 | 2: halves 1 | 0, the lower wins
    assert np.isinf(R.reduce_64(vol, valid, 'max')[0][3, 1]) and ties[3, 1] == 1 and argz[3, 1] == 0
    assert (argz[4] == 255).all() and (ties[4] == 0).all()                        # nothing valid
    # somewhere in the random columns: a maximum tied between the halves with the lower level in half 1, and a
    # value equal to the maximum in an invalid level
    best, hold, cnt = R.holders_64(vol, valid)
    rank = np.cumsum(valid, -1) - 1
    half = (rank % 2)[..., None] * np.ones(vol.shape, int)
    first_half = np.take_along_axis(half, argz.astype(int).clip(0, Z - 1)[:, None, :], 1)[:, 0]
    both = (np.where(hold, half, 0).sum(1) > 0) & (np.where(hold, 1 - half, 0).sum(1) > 0)
    with np.errstate(invalid='ignore'):
      seen |= [(both & (first_half == 1))[5:].any(), (both & (first_half == 0))[5:].any(),
               ((~valid[..., None]) & (vol == best[:, None, :]))[5:].any()]
  assert seen.all()


def test_rank_to_half_rule_of_the_sum_model():
  """Ranks 4t, 4t+2 -> half 0 and 4t+1, 4t+3 -> half 1: an input on which only that association gives these bits."""
  big, one = f32(2.0 ** 24), f32(1)
  vol = np.zeros((1, 8, 4), f32)
  valid = np.array([[1, 0, 1, 1, 0, 1, 1, 0]], bool)        # ranks 0 .. 4 at levels 0, 2, 3, 5, 6
  vol[0, [0, 2, 3, 5, 6], 0] = [big, one, -big, one, one]
  # half 0 (ranks 0, 2, 4): (2^24 - 2^24) + 1 = 1; half 1 (ranks 1, 3): 1 + 1 = 2; together 3.  In sequence the first
  # 1 is lost in 2^24 + 1: 2.
  assert R.pool_32(vol, valid, 'sum')[0][0, 0] == 3
  assert R._seq([vol[0, z] for z in (0, 2, 3, 5, 6)], 'sum')[0] == 2
  wide = np.concatenate([vol, np.zeros((1, 57, 4), f32)], 1)  # Z = 65: the plain sequence
  assert R.pool_32(wide, np.concatenate([valid, np.zeros((1, 57), bool)], 1), 'sum')[0][0, 0] == 2


def test_norm_rows_at_eps():
  c = FUSE['norm_at_eps_Dm4']
  eps = f32(c['eps'])
  m = R.fuse_32(c['planes'], c['valids'], 'sum', c['Wm'], c['bm'], True, c['eps'])[2]
  y = c['planes'][0]
  nrm32 = R.normalize_32(y, c['eps'])[1][:, 0]
  nrm64 = np.sqrt((y.astype(np.float64) ** 2).sum(-1))
  assert nrm32[0] == eps and nrm64[0] == eps and (m[0] == 0.5).all()             # exactly eps: not invalid
  assert nrm32[1] == eps and nrm64[1] < eps and m[1].all()                       # the ulp rounds away in f32 (see the case)
  assert nrm32[2] < eps and nrm64[2] < eps and not m[2].any()                    # two ulps: zero
  assert nrm32[3] >= eps and m[3].all() and not m[4].any() and m[5, 0] == 1
  c = FUSE['norm_at_eps_Dm1']
  assert R.fuse_32(c['planes'], c['valids'], 'sum', c['Wm'], c['bm'], True, c['eps'])[2].ravel().tolist() == [1.0, 0.0, 1.0]
  c = FUSE['zero_vector_default_eps']
  assert not R.fuse_32(c['planes'], c['valids'], 'sum', c['Wm'], c['bm'], True, c['eps'])[2].any()


def test_no_random_cell_has_a_norm_near_eps():
  """The cap is 0: only the planted rows of the eps cases take the model-only comparison of check_fuse."""
  for name, c in FUSE.items():
    if c['Wm'] is None or not c['normalize']:
      continue
    for pooling in c['poolings']:
      near = G.fuse_expected(name, pooling)['near']
      assert near.sum() == (0 if 'norm_case' not in c else near.sum()), name
      if 'norm_case' in c:
        assert near.sum() <= 4


def test_confidence_pooling_columns_are_what_their_kinds_say():
  for name, c in CPOOL.items():
    if c['kinds'] is None:
      continue
    kinds, valid = c['kinds'], c['valid']
    Z = valid.shape[1]
    for log_sig in (False, True):
      plane, any_, s, p, raw = R.conf_pool_64(c['vol'], valid, c['w'], c['b'], log_sig)
      assert np.abs(raw).max() <= 81 and np.isfinite(plane).all()
      assert (np.where(valid, s, -np.inf).max(-1)[any_] > -104).all()            # no 0 / 0 column
      if Z > 2:
        assert (np.diff(raw[kinds == 1], axis=-1) > 0).all() and (np.diff(raw[kinds == 2], axis=-1) < 0).all()
      assert (raw[kinds == 3] < 0).all()
      for m in np.nonzero(kinds == 4)[0]:
        assert np.allclose(p[m][valid[m]], 1.0 / valid[m].sum(), rtol=1e-12)
        s32 = R.conf_pool_32(c['vol'], valid, c['w'], c['b'], log_sig)[2][m]
        assert (s32 == s32[0]).all()
      assert (p[kinds == 5].max(-1) == 1).all() and (valid[kinds == 5].sum(-1) == 1).all()
      assert not any_[kinds == 6].any() and not plane[kinds == 6].any() and not p[kinds == 6].any()
      if Z >= 2 and not log_sig and (kinds == 7).any():
        dead = valid & (p.astype(f32) == 0)
        assert dead[kinds == 7].any()


def test_every_kernel_is_reached_and_every_dispatch_edge_is_in_the_table():
  hit = R.kernels_reached()
  assert all(hit[k] for k in R.KERNELS), {k: len(v) for k, v in hit.items()}
  zs = {c['vol'].shape[1] for c in R.pool_cases()}
  assert {1, 2, 3, 4, 5, 63, 64, 65, 255} <= zs
  assert {c['vol'].shape[2] for c in R.pool_cases()} >= {4, 8, 124, 128, 132, 252, 256}
  assert {c['planes'][0].shape[1] for c in R.fuse_cases()} >= {4, 8, 124, 128, 132, 252, 256}
  assert {c['Wm'].shape[1] for c in R.fuse_cases() if c['Wm'] is not None} >= {1, 5, 31, 32}
  assert {len(c['planes']) for c in R.fuse_cases()} == {1, 2, 3, 4}
  assert [R.fuse_kernel(M, 128, True).endswith('d128_kernel') for M in R.PERSISTENT_SIZES] == [False, True, True, True, True]
  assert R.fuse_kernel(16385, 128, False) == 'plane_fuse_match_kernel' and R.fuse_kernel(16385, 124, True) == 'plane_fuse_match_kernel'
  assert R.pool_kernel(64, 128, 'max', True) == 'vertical_pool_max_arg_kernel'
  assert R.pool_kernel(65, 128, 'max', True) == 'vertical_pool_kernel' and R.pool_kernel(64, 132, 'max', True) == 'vertical_pool_wave_kernel'
  assert R.pool_kernel(64, 128, 'sum', True) == 'vertical_pool_wave_kernel'


def test_entry_points_refuse_with_status_codes_before_any_launch():
  """No device here: a refusal that returns its status code cannot have launched anything."""
  from snap_amd import _lib
  lib = _lib.load()
  one = ctypes.c_void_p(16)
  ptrs = (ctypes.c_void_p * 5)(16, 16, 16, 16, 16)
  pp = ctypes.cast(ptrs, ctypes.c_void_p)
  BAD_SHAPE, UNSUPPORTED = -1, -2
  for D in (6, 260):
    assert R.pool_refused(3, D)
    assert lib.snap_vertical_pool_f32(one, one, one, one, 4, 3, D, 0, None) == BAD_SHAPE
    assert lib.snap_plane_fuse_match_f32(pp, pp, 2, 4, D, 0, one, one, None, None, 0, 1, 1e-5, None, None) == BAD_SHAPE
    assert lib.snap_plane_fuse_match_bwd_f32(pp, pp, pp, 2, 4, D, 0, None, None, 0, 1, 1e-5, None, one, None, None) == BAD_SHAPE
  for n in (0, 5):
    assert R.fuse_refused(n, 8)
    assert lib.snap_plane_fuse_match_f32(pp, pp, n, 4, 8, 0, one, one, None, None, 0, 1, 1e-5, None, None) == UNSUPPORTED
    assert lib.snap_plane_fuse_match_bwd_f32(pp, pp, pp, n, 4, 8, 0, None, None, 0, 1, 1e-5, None, one, None, None) == UNSUPPORTED
  assert R.fuse_refused(2, 8, Dm=33)
  assert lib.snap_plane_fuse_match_f32(pp, pp, 2, 4, 8, 0, one, one, one, one, 33, 1, 1e-5, one, None) == UNSUPPORTED
  assert lib.snap_plane_fuse_match_bwd_f32(pp, pp, pp, 2, 4, 8, 0, one, one, 33, 1, 1e-5, one, None, one, None) == UNSUPPORTED
  for Z, D in ((65, 8), (4, 132)):
    assert R.conf_pool_refused(Z, D)
    assert lib.snap_vertical_pool_conf_f32(one, one, one, one, 4, Z, D, 0, one, one, one, one, None) == BAD_SHAPE
    assert lib.snap_vertical_pool_conf_bwd_f32(one, one, one, one, one, one, 4, Z, D, 0, one, one, None) == BAD_SHAPE
  assert lib.snap_vertical_pool_max_arg_f32(one, one, one, one, one, one, 4, 65, 8, None) == UNSUPPORTED
  assert lib.snap_vertical_pool_max_arg_f32(one, one, one, one, one, one, 4, 64, 132, None) == UNSUPPORTED


# ------------------------------- the models against their bounds ------------------------------
def _all_checks(mutant=None, families=('pool', 'fuse', 'persistent', 'conf_head', 'conf_pool'), stop_at_first=False):
  """Run the model (or a mutant of it) through the GPU file's comparison functions: the cases that reject it."""
  rejected = []

  def run(label, fn):
    try:
      fn()
    except AssertionError as e:
      rejected.append((label, str(e).split('\n')[0][:160]))
    return bool(rejected) and stop_at_first

  for c in R.pool_cases() if 'pool' in families else ():
    for pooling in R.POOLINGS:
      if run(f'{c["name"]} {pooling}', lambda: G.check_pool(c, pooling, model_pool(c, pooling, mutant))):
        return rejected
  cases = list(R.fuse_cases()) if 'fuse' in families else []
  cases += [R.persistent_case(M) for M in ((8193,) if mutant else (8191, 8193))] if 'persistent' in families else []
  for c in cases:
    for pooling in c['poolings']:
      if run(f'{c["name"]} {pooling}', lambda: G.check_fuse(c, pooling, model_fuse(c, pooling, mutant))):
        return rejected
  for c in R.conf_head_cases() if 'conf_head' in families else ():
    run(c['name'], lambda: G.check_conf_head(c, model_conf_head(c)))
  for c in R.conf_pool_cases() if 'conf_pool' in families else ():
    for log_sig in (False, True):
      if run(f'{c["name"]} log_sig={log_sig}', lambda: G.check_conf_pool(c, log_sig, model_conf_pool(c, log_sig, mutant))):
        return rejected
  return rejected


def test_f32_models_stay_within_half_of_their_bounds():
  """Every case of the table: the models pass the GPU file's checks, and their worst error is at most 0.5 of the bound
  (SHARES is in units of MARGIN x bound).  ULP_EXP is the smallest power of two at which this holds."""
  G.SHARES.clear()
  assert _all_checks() == []
  worst = {k: v * R.MARGIN for k, v in G.SHARES.items()}
  G.SHARES.clear()
  for k in sorted(worst):
    print(f'[bev-planes] f32 model, {k}: worst share of the bound {worst[k]:.3f}')
  over = {k: v for k, v in worst.items() if v > 0.5}
  assert not over, over


FAMILY = dict(last_level_dropped=('pool',), level63_masked=('pool',), mean_by_Z=('pool',), invalid_in_sum=('pool',),
              argz_highest=('pool',), ties_over_invalid=('pool',), full_grad_holders=('pool',), no_bias=('fuse',),
              head_128_only=('fuse',), norm_le_eps=('fuse',), uncovered_bias=('fuse',), noncover_ties=('fuse',),
              softmax_over_invalid=('conf_pool',), weight_on_invalid=('conf_pool',), persistent_first_trip_only=('persistent',))


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_mutants_are_rejected(mutant):
  rejected = _all_checks(mutant, FAMILY[mutant], stop_at_first=True)
  assert rejected, f'{mutant}: no case of the table rejects it'
  print(f'[bev-planes] mutant {mutant}: rejected by {rejected[0][0]} ({rejected[0][1]})')


def test_the_softmax_shift_without_its_floor_cannot_be_rejected():
  """max(0, max score) against max score alone: the softmax is invariant under the shift, so the two differ by
  roundings only -- and only on columns whose scores are all negative, which the table holds.  Recorded, not forced."""
  assert any((c['kinds'] == 3).any() for c in R.conf_pool_cases() if c['kinds'] is not None)
  assert _all_checks('softmax_no_floor', ('conf_pool',)) == []
