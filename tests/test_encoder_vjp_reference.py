"""CPU: `encoder_vjp_reference.py` on the reference alone.  The float64 formulas ARE the VJPs (torch autograd), every case
takes the path it declares through the restated launchers, no random GroupNorm case has an element within the gate
margin, the f32 restatements in the kernels' summation order stay at or below 0.5 of the bounds with ``MULT`` the
smallest power of two that achieves it, and every named mutant of a restatement exceeds 1.0."""
import functools
import math

import numpy as np
import pytest

import encoder_vjp_reference as R
import groupnorm_reference as gr


# ----------------------------------------------------------------------------------------------------
# the reference is the VJP
# ----------------------------------------------------------------------------------------------------
def rel(a, b):
  return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('groups', [32, 2, 1])
@pytest.mark.parametrize('mode', R.GN_MODES)
def test_groupnorm_formula_equals_autograd(mode, groups):
  rng = np.random.default_rng(3 + groups)
  N, HW, C = 2, 6, 64
  x, dz = rng.standard_normal((N, HW, C)) * 1.5 + 0.4, rng.standard_normal((N, HW, C))
  gam, beta = rng.standard_normal(C) * 0.3 + 1, rng.standard_normal(C) * 0.2
  dx, dgamma, dbeta, mu, rstd = R.gn_autograd(x, dz, gam, beta, mode, groups)
  ref = R.gn_vjp_ref(x, dz, None, gam, beta, mode, groups, mu, rstd)
  assert rel(ref['dx'][0], dx) <= 1e-12 and rel(ref['dgamma'][0], dgamma) <= 1e-12 and rel(ref['dbeta'][0], dbeta) <= 1e-12
  add = rng.standard_normal((N, HW, C))
  assert rel(R.gn_vjp_ref(x, dz, add, gam, beta, mode, groups, mu, rstd)['dx'][0], dx + add) <= 1e-12


@pytest.mark.parametrize('shape', R.WS_SHAPES[1:])
def test_weight_standardisation_formula_equals_autograd(shape):
  c = R.ws_case(shape)
  ws, dw = R.ws_autograd(c['w'], c['dws'])
  ref = R.ws_ref(c['w'], c['dws'])
  assert rel(ref['fwd'][0], ws) <= 1e-12 and rel(ref['bwd'][0], dw) <= 1e-12


def test_weight_standardisation_k1_is_zero():
  c = R.ws_case(R.WS_SHAPES[0])
  ref = R.ws_ref(c['w'], c['dws'])
  assert (ref['fwd'][0] == 0).all() and (ref['bwd'][0] == 0).all()
  assert (R.ws_fwd_f32(c['w']) == 0).all() and (R.ws_bwd_f32(c['w'], c['dws']) == 0).all()


@pytest.mark.parametrize('shape', R.UP_SHAPES)
def test_upsample_formula_equals_autograd(shape):
  dy = R.up_case(shape)
  assert rel(R.up_ref(dy)[0], R.up_autograd(dy)) <= 1e-12
  ones = np.ones_like(dy)
  assert (R.up_ref(ones)[0] == 4).all() and (R.up_f32(ones) == 4).all()
  ex = R.up_case(shape, exact=True)                    # weights are multiples of 1 / 16: integer dy is exact
  assert R.same_values(R.up_f32(ex).astype(np.float64), R.up_ref(ex)[0])


@pytest.mark.parametrize('shape,path', R.POOL_SHAPES)
def test_max_pool_formula_equals_autograd(shape, path):
  x, dy = R.pool_case(shape, ties=False)
  assert rel(R.pool_ref(x, dy), R.pool_autograd(x, dy)) <= 1e-12
  x, dy = R.pool_case(shape, ties=True)                # first-maximum routing is torch's rule for this window
  assert R.same_values(R.pool_ref(x, dy), R.pool_autograd(x, dy))
  assert R.same_values(R.pool_ref(x, dy, np.float32).astype(np.float64), R.pool_ref(x, dy))
  xs, dys = R.pool_special_planes(shape)
  assert R.pool_ref(xs, dys).sum() == dys.astype(np.float64).sum()       # -inf windows keep their gradient


# ----------------------------------------------------------------------------------------------------
# case validity
# ----------------------------------------------------------------------------------------------------
def test_groupnorm_cases_take_their_declared_paths():
  seen = set()
  for name, N, H, W, C, groups, path, plan, _ in R.GN_CASES:
    assert R.gn_reduce_path(N, C, groups) == path, name
    assert R.gn_plan_b(N, H * W, C) == plan, name
    seen.add(path)
  assert seen == {'group16', 'group64', 'two_kernel'}
  assert R.gn_reduce_path(2, 48, 32) == 'rejected' and R.gn_reduce_path(2, 3072 + 512, 32) == 'rejected'
  by = {c[0]: c for c in R.GN_CASES}
  # both sides of the LDS switch, exactly at 64 KiB
  assert R.gn_lds_bytes(512, 32, 32) == 65536 and R.gn_lds_bytes(513, 32, 32) == 0
  assert R.gn_lds_bytes(128, 1024, 32) == 65536 and R.gn_lds_bytes(129, 1024, 32) == 0
  # thread layouts
  assert R.quad_layout(4) == (1, 256) and R.quad_layout(1024) == (256, 1) and R.quad_layout(2048) == (256, 1)
  assert R.quad_layout(32) == (8, 32)
  # slab plans: one slab, 5 + 4, the 256 cap recomputed with a ragged last slab, one slab because of N
  assert by['cpg16-one-slab'][7] == (1, 7) and by['cpg1-slabs5+4'][7] == (2, 5)
  S, ppb = by['hw2049-capped-ragged'][7]
  assert (S, ppb) == (228, 9) and 2049 - (S - 1) * ppb == 6 and math.ceil(2049 / 256) == ppb
  assert by['n1025-one-slab'][7][0] == 1 and R.gn_plan_b(1024, 16, 32)[0] == 1 and R.gn_plan_b(512, 16, 32)[0] == 2
  # the plan the older test reached
  assert R.gn_plan_b(3, 63, 64) == (8, 8) and R.gn_plan_b(3, 6, 2048) == (1, 6)
  for C, groups in R.GN_EXACT:
    assert R.gn_reduce_path(3, C, groups) in ('group16', 'two_kernel')
  assert {R.gn_reduce_path(3, C, g) for C, g in R.GN_EXACT} == {'group16', 'two_kernel'}


@pytest.mark.parametrize('mode', R.GN_MODES)
def test_no_random_groupnorm_element_sits_on_its_gate(mode):
  for name in R.GN_CASE_IDS:
    c = R.gn_case(name, mode)
    bad = R.gn_gate_offenders(c['x'], c['gamma'], c['beta'], mode, c['groups'], c['mu'], c['rstd'])
    assert int(bad.sum()) == 0, name
    assert c['moved'] <= 0.01 * c['x'].size, name
  c = offset_case(mode)
  assert int(R.gn_gate_offenders(c['x'], c['gamma'], c['beta'], mode, 32, c['mu'], c['rstd']).sum()) == 0


def offset_case(mode):
  c = R.gn_offset_inputs(mode, gr.offset_field)
  rf = mode == R.RELU_GN
  x, mu, rstd, _ = R.gn_settle_gate(c['x'], c['gamma'], c['beta'], mode, 32, lambda v: R.gn_stats_f32(v, 32, rf))
  c.update(x=x, mu=mu, rstd=rstd)
  return c


@pytest.mark.parametrize('mode', R.GN_MODES)
def test_offset_field_is_what_it_says(mode):
  c = offset_case(mode)
  N, H, W, C = c['shape']
  g = c['x'].astype(np.float64).reshape(N, H * W, 32, C // 32)
  ratios = np.abs(g.mean(axis=(1, 3))) / np.maximum(g.std(axis=(1, 3)), 1e-30)
  for want in (16, 64, 256):
    assert ((ratios > 0.7 * want) & (ratios < 1.4 * want)).any(), want
  n, grp = c['planted'].where['const 3.1']
  assert g[n, :, grp].std() == 0 and abs(float(c['rstd'][n, grp * (C // 32)]) - 1 / math.sqrt(1e-5)) < 1e-3
  if mode == R.RELU_GN:
    n, grp = c['planted'].where['all negative']
    assert (g[n, :, grp] < 0).all()


def test_exact_groupnorm_case_is_exact_in_f32():
  for mode in R.GN_MODES:
    for C, groups in R.GN_EXACT:
      c = R.gn_exact_case(mode, C, groups)
      assert (c['x'] == 0).any() and np.signbit(c['x'][c['x'] == 0]).any() and (c['gamma'] == 0).any()
      ref = R.gn_vjp_ref(*R.gn_args(c))
      got = R.gn_vjp_f32(*R.gn_args(c))
      for k in ref:
        assert R.same_values(got[k].astype(np.float64), ref[k][0]), (mode, C, k)
      dx = ref['dx'][0]
      if mode == R.RELU_GN:
        assert (dx[c['x'] <= 0] == 0).all()


def test_column_sum_cases_take_their_declared_paths():
  assert [R.colsum_slabs(M) for M in (1, 511, 512, 513, 1024, 1025)] == [1, 1, 1, 2, 2, 3]
  assert [R.colsum_slabs(M) for M in R.COLSUM_M] == [1, 1, 2, 3]
  M, C = R.COLSUM_RAGGED
  S = R.colsum_slabs(M)
  rpb = R.cdiv(M, S)
  assert S == 5 and 0 < M - (S - 1) * rpb < rpb and R.quad_layout(C) == (1, 256)
  assert all(R.epilogue_colsum_path(C) == 'fused' for C in R.COLSUM_C_FUSED)
  assert all(R.epilogue_colsum_path(C) == 'fallback' for C in R.COLSUM_C_FALLBACK)
  assert R.colsum_kernel_of(12) == 'v4' and R.colsum_kernel_of(1028) == 'scalar' and R.colsum_kernel_of(2048) == 'fused'
  c = R.colsum_case(513, 256)
  y = c['y']
  assert np.isnan(y).any() and ((y == 0) & np.signbit(y)).any() and ((y == 0) & ~np.signbit(y)).any()
  ref = R.gate_ref(c['dy'], y, None, True, None)
  with np.errstate(invalid='ignore'):
    assert (ref['out'][~(y > 0)] == 0).all()
  assert [R.gate_ref(c['dy'], y, None, False, rc)['Msum'] for rc in R.row_counts(513)] == [513, 0, 1, 513, 513]


def test_weight_tables_and_pool_paths():
  shapes = [R.WS_SHAPES[i] for i in R.WS_MULTI['seven']]
  begin, total = R.wstd_table(shapes)
  assert begin == [0, 1, 8, 10, 12, 14, 15] and total == 16
  owners = [R.wstd_lookup(begin, b) for b in range(total)]
  assert owners == [0] + [1] * 7 + [2] * 2 + [3] * 2 + [4] * 2 + [5] + [6]
  assert {len(v) for v in R.WS_MULTI.values()} == {1, 2, 7}
  blocks = [R.cdiv(R.WS_SHAPES[i][3], 32) for i in R.WS_MULTI['seven']]
  assert blocks[0] == 1 and blocks[1] > 1 and blocks[-1] == 1 and blocks[-2] == 1 and max(blocks) == 7
  two = [R.cdiv(R.WS_SHAPES[i][3], 32) for i in R.WS_MULTI['two']]
  assert two[0] > 1 and two[1] == 1                               # many blocks first, one block last
  for shape, path in R.POOL_SHAPES:
    assert R.maxpool_path(shape[0], shape[3]) == path
  assert R.maxpool_path(1, 8, aligned=False) == 'scalar' and R.maxpool_path(70000, 8) == 'vec4'
  assert R.cdiv(68, 64) == 2 and (68 // 4) - 16 == 1            # the second channel workgroup has one live quad


# ----------------------------------------------------------------------------------------------------
# the f32 restatements against the bounds
# ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured():
  """{op: (worst error / (MULT bound) of the f32 restatement over all cases, case)}."""
  worst = {k: (0.0, '') for k in R.MULT}

  def upd(op, r, tag):
    if r > worst[op][0]:
      worst[op] = (r, tag)

  for mode in R.GN_MODES:
    for c in [R.gn_case(n, mode) for n in R.GN_CASE_IDS] + [offset_case(mode)]:
      ref, got = R.gn_vjp_ref(*R.gn_args(c)), R.gn_vjp_f32(*R.gn_args(c))
      for k in ref:
        upd('gn_' + k, R.ratio(got[k], *ref[k], 'gn_' + k), f'{c["name"]} {mode}')
  for c in [R.ws_case(s) for s in R.WS_SHAPES] + [R.ws_case(R.WS_OFFSET_SHAPE, o) for o in R.WS_OFFSETS]:
    ref = R.ws_ref(c['w'], c['dws'])
    tag = f'{c["shape"]} offset {c["offset"]:g}'
    upd('ws_fwd', R.ratio(R.ws_fwd_f32(c['w']), *ref['fwd'], 'ws_fwd'), tag)
    upd('ws_bwd', R.ratio(R.ws_bwd_f32(c['w'], c['dws']), *ref['bwd'], 'ws_bwd'), tag)
  for name in R.WS_MULTI:
    for c in R.ws_multi_cases(name):
      ref = R.ws_ref(c['w'], c['dws'])
      upd('ws_fwd', R.ratio(R.ws_fwd_f32(c['w']), *ref['fwd'], 'ws_fwd'), f'multi {name} {c["shape"]}')
      upd('ws_bwd', R.ratio(R.ws_bwd_f32(c['w'], c['dws']), *ref['bwd'], 'ws_bwd'), f'multi {name} {c["shape"]}')
  for C in R.COLSUM_C_FUSED + R.COLSUM_C_FALLBACK:
    kern = R.colsum_kernel_of(C)
    for M, c, use_mask, rc, relu in R.gate_variants_f32(C):
      ref = R.gate_ref(c['dy'], c['y'], c['mask'] if use_mask else None, relu, rc, kern)
      got = R.colsum_f32(ref['out'].astype(np.float32), ref['Msum'], kern)
      upd('colsum', R.ratio(got, *ref['sums'], 'colsum'), f'{M}x{C} {kern} mask={use_mask} rows={rc} relu={relu}')
  for kind in ('bf16', 'fp16'):
    for C in R.HALF_C:
      for M, exact, h, rc, relu in R.gate_variants_half(C, kind):
        for wrelu in (False, True):
          w = R.half_weight(h, kind, wrelu)
          ref = R.gate_ref(h['dy'], h['y'], None, relu, rc, weight=w)
          n = ref['Msum']
          o = ref['out'].astype(np.float32)
          tag = f'{kind} {M}x{C} rows={rc} relu={relu} wrelu={wrelu}'
          upd('colsum', R.ratio(R.colsum_f32(o, n), *ref['sums'], 'colsum'), tag)
          wo = np.zeros_like(o)
          wo[:n] = o[:n] * w[:n, None]
          upd('wsum', R.ratio(R.colsum_f32(wo, n), *ref['wsum'], 'wsum'), tag)
          if C == 256:
            wt = R.round_half(h['wtail'], kind)
            upd('dtail', R.ratio(R.dtail_f32(o[:n], wt), *R.dtail_ref(o[:n], wt), 'dtail'), tag)
  for shape in R.UP_SHAPES:
    dy = R.up_case(shape)
    upd('upsample', R.ratio(R.up_f32(dy), *R.up_ref(dy), 'upsample'), str(shape))
  for shape, _ in R.POOL_SHAPES:
    x, dy = R.pool_case(shape, ties=False)
    upd('maxpool', R.ratio(R.pool_ref(x, dy, np.float32), R.pool_ref(x, dy), R.pool_bound(x, dy), 'maxpool'), str(shape))
  return worst


@pytest.mark.parametrize('op', sorted(R.MULT))
def test_restatement_stays_below_half_and_the_multiplier_is_the_smallest(op):
  r, where = measured()[op]
  print(f'[encoder vjp cpu] {op}: f32 restatement max err / bound = {r:.4f} at {where}; multiplier 2^{int(math.log2(R.MULT[op]))}')
  assert 0 < r <= 0.5, (op, r, where)
  assert r > 0.25, f'{op}: half the multiplier would still hold the restatement at {2 * r:.3f}'


# ----------------------------------------------------------------------------------------------------
# the bounds bite
# ----------------------------------------------------------------------------------------------------
def gn_mutant_ratio(c, mutant):
  ref, got = R.gn_vjp_ref(*R.gn_args(c)), R.gn_vjp_f32(*R.gn_args(c), mutant=mutant)
  return {k: R.ratio(got[k], *ref[k], 'gn_' + k) for k in ref}


@pytest.mark.parametrize('mode', R.GN_MODES)
def test_groupnorm_mutants_exceed_the_bound(mode):
  out = {}
  out['1 drop_phase'] = gn_mutant_ratio(R.gn_case('cpg1-slabs5+4', mode), 'drop_phase')
  out['1 drop_phase c4'] = gn_mutant_ratio(R.gn_case('c4-256-phases', mode), 'drop_phase')
  out['2 drop_last_slab'] = gn_mutant_ratio(R.gn_case('hw2049-capped-ragged', mode), 'drop_last_slab')
  out['2 drop_last_slab 5+4'] = gn_mutant_ratio(R.gn_case('cpg1-slabs5+4', mode), 'drop_last_slab')
  for k, v in out.items():
    print(f'[encoder vjp cpu] mutant {k} {mode}: {v}')
    assert min(v.values()) > 1.0, (k, v)
  r = gn_mutant_ratio(R.gn_case('groups1-c128', mode), 'wrong_inv_cnt')
  print(f'[encoder vjp cpu] mutant 3 wrong_inv_cnt {mode}: {r}')
  assert r['dx'] > 1.0 and max(r['dgamma'], r['dbeta']) <= 0.5          # (the parameter gradients do not read inv_cnt)
  for C, groups in R.GN_EXACT:
    r = gn_mutant_ratio(R.gn_exact_case(mode, C, groups), 'gate_ge')
    print(f'[encoder vjp cpu] mutant 4 gate_ge {mode} C={C}: {r}')
    assert r['dx'] > 1.0
    if mode == R.GN_RELU:
      assert min(r.values()) > 1.0


def test_weight_standardisation_mutants_exceed_the_bound():
  for shape in [(1, 1, 31, 33), (1, 1, 33, 31), (3, 3, 20, 36)]:
    c = R.ws_case(shape)
    ref = R.ws_ref(c['w'], c['dws'])
    f = R.ratio(R.ws_fwd_f32(c['w'], mutant='k_rounded_up'), *ref['fwd'], 'ws_fwd')
    b = R.ratio(R.ws_bwd_f32(c['w'], c['dws'], mutant='k_rounded_up'), *ref['bwd'], 'ws_bwd')
    print(f'[encoder vjp cpu] mutant 5 k_rounded_up {shape}: fwd {f:.3g} bwd {b:.3g}')
    assert f > 1.0 and b > 1.0
  for name, idx in R.WS_MULTI.items():
    cs = [R.ws_case(R.WS_SHAPES[i], seed=j) for j, i in enumerate(idx)]
    ws, gs = [c['w'] for c in cs], [c['dws'] for c in cs]
    for dws in (None, gs):
      good = R.ws_multi_f32(ws, dws)
      bad = R.ws_multi_f32(ws, dws, mutant='table_off_by_one')
      worst = 0.0
      for j, c in enumerate(cs):
        ref = R.ws_ref(c['w'], c['dws'])
        single = R.ws_fwd_f32(c['w']) if dws is None else R.ws_bwd_f32(c['w'], c['dws'])
        assert R.bits_equal(good[j], single), (name, j)
        key, op = ('fwd', 'ws_fwd') if dws is None else ('bwd', 'ws_bwd')
        assert R.ratio(good[j], *ref[key], op) <= 0.5
        worst = max(worst, R.ratio(bad[j], *ref[key], op))
      print(f'[encoder vjp cpu] mutant 6 table_off_by_one {name} {"fwd" if dws is None else "bwd"}: {worst}')
      assert worst > 1.0 or len(idx) == 1          # (a table of one item has no neighbour to be sent to)


def test_column_sum_mutants_exceed_the_bound():
  M, C = R.COLSUM_RAGGED
  c = R.colsum_case(M, C)
  ref = R.gate_ref(c['dy'], c['y'], c['mask'], True, None)
  o = ref['out'].astype(np.float32)
  for mutant in ('drop_phase', 'drop_last_slab'):
    r = R.ratio(R.colsum_f32(o, M, mutant=mutant), *ref['sums'], 'colsum')
    print(f'[encoder vjp cpu] mutant colsum {mutant} {M}x{C}: {r:.3g}')
    assert r > 1.0
  c = R.colsum_case(1025, 256)
  ref = R.gate_ref(c['dy'], c['y'], None, True, None)
  o = ref['out'].astype(np.float32)
  for mutant in ('drop_phase', 'drop_last_slab'):
    r = R.ratio(R.colsum_f32(o, 1025, mutant=mutant), *ref['sums'], 'colsum')
    print(f'[encoder vjp cpu] mutant colsum {mutant} 1025x256: {r:.3g}')
    assert r > 1.0
  # the gate with >=: y = +0.0 / -0.0 would pass
  with np.errstate(invalid='ignore'):
    ge = np.where(c['y'].astype(np.float64) >= 0, c['dy'].astype(np.float64), 0.0)
  assert R.ratio(ge, ref['out'], np.zeros_like(ge), 'colsum') > 1.0


def test_pool_and_upsample_mutants_exceed_the_bound():
  for shape, _ in R.POOL_SHAPES[2:]:
    x, dy = R.pool_case(shape, ties=True)
    r = R.ratio(R.pool_ref(x, dy, np.float32, last=True), R.pool_ref(x, dy), R.pool_bound(x, dy), 'maxpool')
    print(f'[encoder vjp cpu] mutant 7 last_maximum {shape}: {r}')
    assert r > 1.0
  for shape in R.UP_SHAPES:
    dy = R.up_case(shape)
    r = R.ratio(R.up_f32(dy, mutant='border_once'), *R.up_ref(dy), 'upsample')
    print(f'[encoder vjp cpu] mutant 8 border_once {shape}: {r:.3g}')
    assert r > 1.0
