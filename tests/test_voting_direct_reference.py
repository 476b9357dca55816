"""The direct-form voting's reference, checked on itself (no GPU): tests/voting_direct_reference.py against
``oracle/voting.py`` and ``voting_fft_reference``; the f32 rotation model deciding as float64 does; the stacking and
fold restatements against the sliding-window forms; the restated route on both sides of every condition; the score
multipliers measured from the accumulation models; the escape cap's reference-alone count; and mutants of the reference
that the comparison functions of tests/test_gpu_voting_direct.py must reject.
"""
import numpy as np
import pytest

import voting_direct_reference as Dr
import voting_fft_reference as V
import test_gpu_voting_direct as G
from oracle import grids as o_grids
from oracle import voting as o_voting


def test_rotate64_matches_the_oracle():
  """Values at the oracle's f32 level (it samples in f32: twice the margin the kernel gets), validity exact outside
  the decision distance."""
  for R, H, D, cell in [(8, 16, 4, 0.25), (12, 8, 12, 0.25), (36, 16, 4, 0.3), (4, 33, 4, 0.25), (8, 5, 4, 0.3)]:
    feat, valid = Dr.rotate_inputs(R, H, D, cell)
    ref = Dr.rotate64(feat, valid, R, H, cell)
    t, tv = o_voting.sample_query_templates(feat, valid, R, o_grids.Grid2D((H, H), cell))
    tv = np.asarray(tv, bool)
    assert not ((tv != ref['tvalid']) & ~Dr.near_decision(ref)).any()
    both = tv & ref['tvalid']
    assert both.sum() > 0.3 * both.size
    err = np.abs(np.asarray(t, np.float64) - ref['templates'])[both]
    assert (err <= 2 * Dr.VALUE_MARGIN * ref['value_bound'][both] + 1e-12).all(), err.max()
    assert (ref['tcount'] == ref['tvalid'].sum((-1, -2))).all()
    assert (ref['cw'] == ref['tvalid'][:, ::-1, ::-1].transpose(1, 2, 0)).all()


def test_rotate32_decides_as_rotate64_and_the_escape_cap_holds_on_the_reference_alone():
  """Every rotation case of the GPU file carries invalid input cells; the f32 model stays within HALF the GPU's value
  margin, its validity flips only at cells float64 puts within BORDER_TOL of a decision, and on the capped rotations
  float64 alone has at most a quarter of the cap there."""
  worst, alone, axis_flips = 0.0, 0, 0
  for R, H, D, cell in Dr.ROTATE_CASES:
    feat, valid = Dr.rotate_inputs(R, H, D, cell)
    assert not valid.all()
    ref = Dr.rotate64(feat, valid, R, H, cell)
    n = Dr.reference_alone_count(ref)
    assert n <= Dr.FLIP_CAP / 4 * R * H * H, (R, H, D, cell, n)
    alone += n
    t32, v32 = Dr.rotate32(feat, valid, R, H, cell)
    flips = v32 != ref['tvalid']
    capped = Dr.capped_rotations(R)
    assert not (flips & ~Dr.near_decision(ref)).any() and flips[capped].sum() <= n
    axis_flips += int(flips[~capped].sum())
    if cell == 0.25:                                         # exact coordinates: the rotations by 90 degrees are copies
      RQ = R // 4
      assert not flips[~capped].any()
      for k in range(4):
        assert (t32[k * RQ][v32[k * RQ]] == np.rot90(feat, k, axes=(1, 0))[v32[k * RQ]]).all()
    both = v32 & ref['tvalid']
    err, tol = np.abs(t32.astype(np.float64) - ref['templates'])[both], ref['value_bound'][both]
    assert (err[tol == 0] == 0).all()
    worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
  print(f'rotate32: worst error / value_bound = {worst:.3f}; reference-alone cells near a decision: {alone}; '
        f'flips of the model on the uncapped rotations at cell 0.3: {axis_flips}')
  assert worst <= 0.5 * Dr.VALUE_MARGIN
  # (i + 0.5) x 0.3f / 0.3f is NOT i + 0.5 for every i: at cell 0.3 the rotations by 90 degrees are no bit copies,
  # and their validity may take the other tap pair
  feat, valid = Dr.rotate_inputs(4, 33, 4, 0.3)
  t32, v32 = Dr.rotate32(feat, valid, 4, 33, 0.3)
  assert (t32[0][v32[0]] != feat[v32[0]]).any() and axis_flips > 0


def test_stack_bank_and_unstack_are_the_direct_form():
  rng = np.random.default_rng(3)
  divides = set()
  for S in (2, 3, 4):
    for H, W, Hm, Wm in [(5, 7, 5, 7), (6, 6, 7, 5), (5, 4, 6, 6), (7, 5, 5, 7), (4, 4, 5, 5)]:
      R, D = 3, 2
      divides |= {(S, (3 * Hm - 1 - H) % S == 0), (S, (3 * Wm - 1 - W) % S == 0)}
      q = rng.standard_normal((R, H, W, D))
      m = rng.standard_normal((Hm, Wm, D))
      tv = np.ones((R, H, W), bool)
      want = V.direct64(q, tv, m, None, None) * (H * W)
      got = Dr.stacked_corr64(q, V._pad_edge(m), S).transpose(2, 0, 1)
      assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (S, H, W)
  assert divides == {(S, d) for S in (2, 3, 4) for d in (True, False)}, divides
  assert (3 * 20 - 1 - 20) % 3 == 0                                    # the table's S = 3 case: S divides Ho = 39


def test_fold_counts_are_the_sliding_window_integers():
  rng = np.random.default_rng(5)
  for W, Wm, H, Hm in [(32, 32, 3, 4), (64, 64, 2, 3), (96, 96, 2, 2), (64, 40, 3, 3)]:
    tv = rng.random((3, H, W)) < 0.8
    mv = rng.random((Hm, Wm)) < 0.9
    want = V.counts_direct(tv, mv)
    got = Dr.fold_counts(V._pad_zero(mv), tv[:, ::-1, ::-1].transpose(1, 2, 0))
    assert got.shape == want.shape and (got == want).all(), (W, Wm)
    assert (want.shape[2] % 32 != 0)


def test_restated_route():
  for g in Dr.CASES:
    assert Dr.restated_route(g['R'], g['H'], g['W'], g['D'], g['engine'], g['switches']) == (g['route'], g['count']), g['name']
    assert g['name'].startswith(g['route'])
  assert len({g['name'] for g in Dr.CASES}) == len(Dr.CASES) == 20
  rr = Dr.restated_route
  # STACK_MIN_CELLS
  assert rr(4, 64, 64, 4)[0] == 'stacked' and rr(4, 63, 65, 4)[0] == 'plain' and rr(4, 64, 63, 4)[0] == 'plain'
  # R S^2 % 4 (S = 3, odd R) and S <= 1
  assert rr(7, 24, 24, 4, 'f32', dict(STACK_SHIFT=3, STACK_MIN_CELLS=0))[0] == 'plain'
  assert rr(8, 24, 24, 4, 'f32', dict(STACK_SHIFT=3, STACK_MIN_CELLS=0))[0] == 'stacked'
  assert rr(4, 64, 64, 4, 'f32', dict(STACK_SHIFT=1))[0] == 'plain'
  # W % 32 -- and only on the stacked route
  assert rr(4, 64, 96, 4)[1] == 'folded-count' and rr(4, 66, 66, 4)[1] == 'scalar-count' and rr(4, 96, 64 + 8, 4)[1] == 'scalar-count'
  assert rr(4, 32, 32, 4)[1] == 'scalar-count'
  # every pre-split condition
  ok = (12, 64, 64, 16, 'bf16x3')
  assert rr(*ok)[0] == 'presplit+fused'
  assert rr(*ok, dict(FUSED_TEMPLATE_PACK=False))[0] == 'presplit' and rr(*ok, dict(have_templates=False))[0] == 'presplit'
  assert rr(12, 64, 64, 16, 'f32')[0] == 'stacked' and rr(12, 64, 64, 16, 'bf16x6')[0] == 'stacked'
  assert rr(*ok, dict(USE_PRESPLIT_VOTING=False))[0] == 'stacked'
  assert rr(12, 64, 64, 8, 'bf16x3')[0] == 'stacked' and rr(4, 64, 64, 16, 'bf16x3')[0] == 'stacked'
  assert rr(*ok, dict(presplit_supported=False))[0] == 'stacked'
  # every production route is reached without patching a switch
  reached = {(g['route'], g['count']) for g in Dr.PRODUCTION if g['switches'].get('FUSED_TEMPLATE_PACK', True)}
  assert {r for r, _ in reached} == {'plain', 'stacked', 'presplit+fused'} and len({k for _, k in reached}) == 2


# worst |model - float64| in units of 2^-24 x A, per engine (both models, every case and kind of the table)
MODEL_WORST = {}


def test_models_stay_within_half_the_bound():
  """The sequential and the k-step model of the f32 accumulation (on the split engines: of the kept part products) on
  a SAMPLE of 16 placements (the corners, the centre, 11 drawn) of every GPU input: within 0.5 x score_bound, and
  ACC[engine] is the smallest power of two that achieves it on that sample.  Every case and kind has rotations whose float64 argmax is decided."""
  worst = {}
  for name in Dr.CASE_IDS:
    g = Dr.BY_NAME[name]
    for kind in Dr.KINDS:
      c = Dr.case(name, kind)
      geo = V.geometry(g['H'], g['W'], g['Hm'], g['Wm'])
      cells = Dr.sample_cells(name, geo['Ho'], geo['Wo'], n=11)
      ia, ib = (np.array(cells).T)
      unit = c['bound'][:, ia, ib] * c['tcount'][:, None] / Dr.C[g['engine']]                  # 2^-24 x A
      want = c['raw'][:, ia, ib] * c['tcount'][:, None]
      for mode in ('seq', 'kstep'):
        err = np.abs(Dr.model_dot(c['q'], c['m'], cells, g['engine'], mode) - want) / unit
        worst[g['engine']] = max(worst.get(g['engine'], 0.0), float(err.max()))
      fin = V.finite_rule(c['counts'], c['thr'])
      assert G.check_argmax(name, np.where(fin, c['raw'], -np.inf).astype(np.float32), c['raw'], fin, c['bound']) > 0, (name, kind)
  print('worst model error in units of 2^-24 x A:', {k: round(v, 2) for k, v in worst.items()})
  MODEL_WORST.update(worst)
  for e, w in worst.items():
    assert w <= 0.5 * Dr.C[e], (e, w)
    assert Dr.ACC[e] == 1.0 or w > 0.5 * (Dr.ACC[e] / 2 + Dr.OPERAND[e]), (e, w)


def test_containment_sets():
  """The two placement sets on a small geometry, against the definition (a NaN pushed through float64 sums)."""
  H, W, Hm, Wm, S = 5, 6, 5, 6, 3
  rng = np.random.default_rng(9)
  q = rng.standard_normal((2, H, W, 2))
  m = rng.standard_normal((Hm, Wm, 2))
  for cell in [(2, 2), (0, 0), (Hm - 1, 3)]:
    bad = m.copy(); bad[cell[0], cell[1], 0] = np.nan
    mp = V._pad_edge(bad)
    cells = Dr.padded_cells(Hm, Wm, cell)
    assert sorted(map(tuple, np.argwhere(np.isnan(mp[..., 0])))) == sorted(cells)
    plain = np.isnan(V.direct64(q, np.ones((2, H, W), bool), bad, None, None))
    assert (plain == Dr.plain_nonfinite_set(H, W, *mp.shape[:2], cells)[None]).all()
    stacked = np.isnan(Dr.stacked_corr64(q, mp, S).transpose(2, 0, 1))
    want = Dr.stacked_nonfinite_set(H, W, S, *mp.shape[:2], cells)
    assert (stacked == want[None]).all()
    assert (want & ~plain[0]).any() and not (plain[0] & ~want).any()          # wider, by up to S - 1 cells
  assert (Dr.stacked_nonfinite_set(H, W, 1, 13, 16, [(6, 7)]) == Dr.plain_nonfinite_set(H, W, 13, 16, [(6, 7)])).all()


# ------------------------------- mutants ---------------------------------
def _rejects(fn, *a, **k):
  with pytest.raises(AssertionError):
    fn(*a, **k)


def _as_kernel(ref):
  return dict(templates=ref['templates'].astype(np.float32), tvalid=ref['tvalid'],
              tw=ref['templates'].astype(np.float32).transpose(1, 2, 3, 0), cw=ref['cw'].astype(np.float32),
              tcount=ref['tcount'].astype(np.float32))


def test_comparison_functions_reject_the_mutants():
  rejected, unrejectable = [], []
  # --- the rotate kernel's contracts: R = 8, H = 16, cell 0.25 (exact axis rotations, 90 % validity)
  R, H, D, cell = 8, 16, 4, 0.25
  feat, valid = Dr.rotate_inputs(R, H, D, cell)
  ref = Dr.rotate64(feat, valid, R, H, cell)
  assert G.check_rotation('good', _as_kernel(ref), ref, exact_first=True, source=feat) == 0
  for mutant in ('rot90-reversed', 'quadrant-index', 'weighted-taps', 'unclamped', 'cw-unflipped', 'tcount-ballot'):
    _rejects(G.check_rotation, mutant, _as_kernel(Dr.rotate64(feat, valid, R, H, cell, mutant)), ref, exact_first=True, source=feat)
    rejected.append(mutant)
  # u <= H: needs a cell whose coordinate IS H -- no cell centre of a rotation about the grid centre reaches it
  # (|u - H/2| <= (H - 1) / sqrt(2) ... only beyond the grid at 45 degrees, where u > H): the mutant decides as the
  # kernel does on every input of the table
  m = Dr.rotate64(feat, valid, R, H, cell, 'u<=H')
  same = all((Dr.rotate64(*Dr.rotate_inputs(*c), *c[:2], c[3], 'u<=H')['tvalid'] == Dr.rotate64(*Dr.rotate_inputs(*c), *c[:2], c[3])['tvalid']).all()
             for c in Dr.ROTATE_CASES[::7])
  if same and (m['tvalid'] == ref['tvalid']).all():
    unrejectable.append('u <= H: no cell centre maps onto u == H exactly')
  else:
    rejected.append('u<=H')
  # --- scores, mask, padding: the rectangular case with a map of another size, offset data
  c = Dr.case('plain-10x13-map12x9-R12-D16-f32', 'offset')
  fin = V.finite_rule(c['counts'], c['thr'])
  ok = np.where(fin, c['raw'], -np.inf).astype(np.float32)
  assert G.check_case('good', ok, c, 'mutants') > 0
  tc = c['tcount'][:, None, None]
  zero = V.raw64(c['q'], c['m'], pad='zero') / tc
  _rejects(G.check_case, 'zero', np.where(fin, zero, -np.inf).astype(np.float32), c, 'mutants')
  rejected.append('zero instead of edge padding')
  Hm, Wm = c['mv'].shape
  edge = np.pad(c['mv'], ((Hm - 1,) * 2, (Wm - 1,) * 2), mode='edge').astype(np.float64)
  cnt_edge = np.rint(V._corr64(c['tv'][:, ::-1, ::-1].astype(np.float64)[..., None], edge[..., None])).astype(np.int64)
  _rejects(G.check_case, 'edge mask', np.where(V.finite_rule(cnt_edge, c['thr']), c['raw'], -np.inf).astype(np.float32), c, 'mutants')
  _rejects(G.check_pad, 'edge mask', np.pad(c['m'], ((Hm - 1,) * 2, (Wm - 1,) * 2, (0, 0)), mode='edge'), edge.astype(np.float32), c['m'], c['mv'])
  rejected.append('mvalid_pad edge padded')
  _rejects(G.check_case, 'tcount', np.where(fin, c['raw'] * tc, -np.inf).astype(np.float32), c, 'mutants')
  rejected.append('a missing / tcount')
  # >= in finalize: a case with counts on the threshold (0.02, 20): threshold 8
  fq, vq, fm, vm = V.rotated_inputs(0.02, 20)
  t, tv = o_voting.sample_query_templates(fq, vq, V.ROTATED_R, o_grids.Grid2D((20, 20), V.ROTATED_CELL))
  counts, thr = V.counts64(tv, vm), V.threshold(0.02, 20, 20)
  raw = V.raw64(t, fm)
  G.check_mask('good', np.where(V.finite_rule(counts, thr), raw, -np.inf).astype(np.float32), counts, thr)
  _rejects(G.check_mask, '>=', np.where(counts >= thr, raw, -np.inf).astype(np.float32), counts, thr)
  rejected.append('>= in finalize')
  unflipped = V.counts64(tv, vm, flip=False)
  _rejects(G.check_mask, 'cw', np.where(V.finite_rule(unflipped, thr), raw, -np.inf).astype(np.float32), counts, thr)
  # --- the un-stack and the zero rows: S = 4 on 24 x 24 (Ho = 47: S does not divide it)
  c = Dr.case('stacked-24x24-map24x24-R4-D4-f32-S2', 'noise')
  fin = V.finite_rule(c['counts'], c['thr'])
  mp = V._pad_edge(c['m'])
  for S in (2, 4):
    good = Dr.stacked_corr64(c['q'], mp, S).transpose(2, 0, 1) / c['tcount'][:, None, None]
    assert G.check_case('good', np.where(fin, good, -np.inf).astype(np.float32), c, 'mutants') > 0
  for mutant, label in (('swap', 'un-stack with sa / sb swapped'), ('crop-first', 'crop before the un-stack'), ('pb=0', 'pb = 0')):
    bad = Dr.stacked_corr64(c['q'], mp, 4, mutant).transpose(2, 0, 1)
    assert Dr.stacked_geometry(24, 24, 4, 70, 70)['pb'] > 0
    if bad.shape != fin.shape:
      _rejects(G.check_case, mutant, bad.astype(np.float32), c, 'mutants')
    else:
      _rejects(G.check_case, mutant, np.where(fin, bad / c['tcount'][:, None, None], -np.inf).astype(np.float32), c, 'mutants')
    rejected.append(label)
  # --- the fold
  c = Dr.case('stacked-64x96-map64x96-R4-D4-f32', 'noise')
  cw = c['tv'][:, ::-1, ::-1].transpose(1, 2, 0)
  G.check_counts('good', Dr.fold_counts(V._pad_zero(c['mv']), cw).transpose(1, 2, 0).astype(np.float32), c['counts'])
  _rejects(G.check_counts, 'ncol', Dr.fold_counts(V._pad_zero(c['mv']), cw, 'ncol-short').transpose(1, 2, 0).astype(np.float32), c['counts'])
  rejected.append('fold with ncol one short')
  # --- containment: the plain set handed to the stacked route
  clean = np.zeros((1, 9, 9), np.float32)
  want = Dr.stacked_nonfinite_set(5, 5, 3, 13, 13, [(6, 6)])
  got = np.where(Dr.plain_nonfinite_set(5, 5, 13, 13, [(6, 6)]), np.nan, 0).astype(np.float32)[None]
  _rejects(G.check_nonfinite_set, 'plain set', got, clean, want[None])
  print('rejected:', rejected, 'unrejectable:', unrejectable)
  assert len(rejected) + len(unrejectable) == 15
  G.SHARES.pop('mutants', None); G.SHARES.pop('rotate', None)
