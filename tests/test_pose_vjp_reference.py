"""`-m "not gpu"`: ``pose_vjp_reference.py`` on the reference alone.

The float64 model is torch's float64 autograd of the bilinear scoring expression; every case of the tables meets its
validity condition before any kernel is run; every named mutant is rejected by the tolerances on the cases
``MUTANT_CASES`` names; the restated launcher sends the tables through every branch; the exact cases are exact.
"""
import numpy as np
import pytest
import torch

import pose_vjp_reference as pvr


# ----------------------------------------------------------------------------------------------------
# the model is the autograd of the scoring expression (test_pose_score_bwd's, copied as the independent statement)
# ----------------------------------------------------------------------------------------------------
def autograd_vjp(inp):
  B, Nq, X, Y = inp['shape']
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
  poses, q_xy, valid_q, mv = t(inp['poses']), t(inp['q_xy']), t(inp['valid_q']), t(inp['map_valid'])
  cell = float(np.float32(inp['cell']))
  P = poses.shape[1]
  sd = torch.zeros((B, Nq, X, Y), dtype=torch.float64, requires_grad=True)
  c, s = torch.cos(poses[..., 0].double()), torch.sin(poses[..., 0].double())
  qx, qy = q_xy[..., 0].double(), q_xy[..., 1].double()
  u = (c[:, :, None] * qx[:, None] - s[:, :, None] * qy[:, None] + poses[..., 1].double()[:, :, None]) / cell
  v = (s[:, :, None] * qx[:, None] + c[:, :, None] * qy[:, None] + poses[..., 2].double()[:, :, None]) / cell
  cu, cv = u - 0.5, v - 0.5
  fu, fv = torch.floor(cu), torch.floor(cv)
  wu1, wv1 = cu - fu, cv - fv
  i0 = fu.long().clamp(0, X - 1); i1 = (fu.long() + 1).clamp(0, X - 1)
  j0 = fv.long().clamp(0, Y - 1); j1 = (fv.long() + 1).clamp(0, Y - 1)
  bi = torch.arange(B)[:, None, None]
  ni = torch.arange(Nq)[None, None, :]
  val = ((1 - wu1) * (1 - wv1) * sd[bi, ni, i0, j0] + (1 - wu1) * wv1 * sd[bi, ni, i0, j1]
         + wu1 * (1 - wv1) * sd[bi, ni, i1, j0] + wu1 * wv1 * sd[bi, ni, i1, j1])
  ok = valid_q[:, None, :].expand(B, P, Nq)
  if inp['mask_oob']:
    inb = (u >= 0) & (u < X) & (v >= 0) & (v < Y)
    tv = mv[bi, i0, j0] & mv[bi, i0, j1] & mv[bi, i1, j0] & mv[bi, i1, j1]
    ok = ok & inb & tv
  (val * ok).sum(-1).backward(t(inp['dscores']).double())
  return sd.grad.numpy()


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('B,Nq,X,Y,P', [(2, 7, 5, 3, 90), (1, 4, 1, 6, 60), (2, 9, 12, 17, 300)])
def test_model_is_float64_autograd_of_the_scoring_expression(B, Nq, X, Y, P, mask):
  inp = pvr.random_case(('autograd', 900 + X, B, Nq, X, Y, P, mask))
  got, want = pvr.model_of(inp), autograd_vjp(inp)
  assert np.abs(want).max() > 0.01
  assert np.abs(got - want).max() <= 1e-12
  assert (got[~inp['valid_q']] == 0).all()


def test_forward_model_is_the_adjoint_of_the_vjp():
  inp = pvr.random_case(('adjoint', 77, 2, 6, 9, 7, 200, True))
  sim = np.random.default_rng(5).standard_normal(inp['shape']).astype(np.float32)
  fwd = pvr.pose_score_fwd(sim, inp['poses'], inp['q_xy'], inp['valid_q'], inp['map_valid'], inp['cell'], True)
  lhs = (pvr.f64(inp['dscores']) * fwd).sum()
  rhs = (pvr.model_of(inp) * sim).sum()
  assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs))


# ----------------------------------------------------------------------------------------------------
# every case is valid from the reference alone
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', pvr.VJP_CASE_IDS)
def test_every_case_meets_the_validity_condition(name):
  r = pvr.case_reference(name)
  _, _, B, Nq, X, Y, P, mask = pvr.case_by_name(name)
  lim = pvr.validity_limit(r['ref'], r['dscores'])
  worst_float, worst_fixed = float((r['tol_float'] / lim).max()), float((r['tol_fixed'] / lim).max())
  print(f'[pose vjp] {name}: tol / limit float {worst_float:.3f} fixed {worst_fixed:.3f}; max n_c {int(r["n_c"].max())}')
  assert worst_float <= 1.0 and worst_fixed <= 1.0
  # the twins pass their own tolerance, the model is not trivial, invalid points are zero planes
  assert pvr.worst(pvr.model_of(r, twin=3), r['ref'], r['tol_fixed'])[0] <= 1.0 / pvr.MARGIN + 1e-9
  vq = r['valid_q']
  assert (r['ref'][~vq] == 0).all() and np.abs(r['ref'][vq]).max() > 0.05
  assert 0.6 <= vq.mean() <= 0.95 or Nq < 10
  # corner and edge traffic on every valid plane family
  cm = pvr.corner_mask(X, Y)
  if not mask and P > 100:
    assert (r['n_c'][vq][:, cm] > 0).all()
  ppc, nch = pvr.chunking(B, Nq)
  if ppc > 1:          # the forced entries: an invalid first, middle and last point of a chunk; an invalid chunk
    assert not vq[:, ppc].any() and vq[:, ppc + 1:2 * ppc].all()
    assert not vq[:, 3 * ppc + ppc - 1].any() and vq[:, 3 * ppc:4 * ppc - 1].all()
    assert not vq[:, 4 * ppc:5 * ppc].any() and vq[:, Nq - 1].all()
    if ppc > 2:
      assert not vq[:, 2 * ppc + 1].any() and vq[:, 2 * ppc].all() and vq[:, 2 * ppc + 2].all()
  if mask:
    assert pvr.decision_margin(r) >= pvr.BORDER_TOL


# ----------------------------------------------------------------------------------------------------
# every mutant is rejected
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mutant,name', [(m, n) for m in pvr.MUTANTS for n in pvr.MUTANT_CASES[m]])
def test_the_tolerances_reject_every_mutant(mutant, name):
  r = pvr.case_reference(name)
  wrong = pvr.model_of(r, mutant=mutant)
  for kind in ('tol_float', 'tol_fixed'):
    ratio, where = pvr.worst(wrong, r['ref'], r[kind])
    print(f'[pose vjp] {mutant} on {name}: {ratio:.3g} x {kind} at {where}')
    assert ratio > 4.0, (mutant, name, kind, ratio)


def test_every_mutant_has_a_case():
  assert set(pvr.MUTANT_CASES) == set(pvr.MUTANTS) and all(pvr.MUTANT_CASES[m] for m in pvr.MUTANTS)


# ----------------------------------------------------------------------------------------------------
# the restated launcher sends the tables through every branch
# ----------------------------------------------------------------------------------------------------
def all_dispatches():
  out = []
  for _, _, B, Nq, X, Y, P, mask in pvr.VJP_CASES:
    out += [pvr.dispatch(B, Nq, X, Y, P, mask, fa) for fa in (False, True)]
  for X, Y, P, mask in pvr.EXACT_CASES:
    out += [pvr.dispatch(2, len(pvr.EXACT_Q), X, Y, P, mask, fa) for fa in (False, True)]
  out.append(pvr.dispatch(*pvr.SCALE_SHAPE, pvr.SCALE_P, False))
  return out


def test_the_tables_take_every_branch_of_the_launcher():
  seen = {pvr.branch_key(d) for d in all_dispatches()}
  has = lambda **kw: any(all(dict(zip(('body', 'raised', 'multi', 'ragged', 'passes', 'slot'), k))[a] == b
                             for a, b in kw.items()) for k in seen)
  for body in ('det', 'fast', 'general', 'general_mask'):
    assert has(body=body), body
  for body in ('det', 'fast'):
    assert has(body=body, raised=False) and has(body=body, raised=True), body
    assert has(body=body, multi=True) and has(body=body, multi=False) and has(body=body, ragged=True), body
    assert has(body=body, slot=0) and has(body=body, slot=1) and has(body=body, slot=9)
  for body in ('general', 'general_mask'):
    assert has(body=body, passes=1) and has(body=body, passes=2), body
  assert has(body='general_mask', multi=True, ragged=True) and has(body='general_mask', raised=True)
  assert all(not pvr.dispatch(1, 5, X, Y, 100, False)['supported'] for X, Y in pvr.UNSUPPORTED_SHAPES)
  assert all(X * Y == pvr.PB_LDS_FLOATS + 1 for X, Y in pvr.UNSUPPORTED_SHAPES)


def test_the_restated_rules_at_their_edges():
  d = lambda name, fa=False: pvr.dispatch(*pvr.case_by_name(name)[2:], fa)
  assert (d('64x128-at-64K')['body'], d('64x128-at-64K')['lds'], d('64x128-at-64K')['lds_raised']) == ('det', 65536, False)
  assert (d('91x91-above-64K')['body'], d('91x91-above-64K')['lds_raised']) == ('det', True)
  assert (d('128x128-training')['body'], d('128x128-training')['lds']) == ('det', 131072)
  assert (d('128x128-training', True)['body'], d('128x128-training', True)['lds_raised']) == ('fast', False)
  assert (d('129x128-float-above-64K', True)['body'], d('129x128-float-above-64K', True)['lds_raised']) == ('fast', True)
  assert (d('152x128-largest-fixed')['body'], d('152x128-largest-fixed')['lds']) == ('det', pvr.PB_DET_BYTES)
  assert d('139x140-float-by-shape')['body'] == 'fast' and d('192x128-largest')['body'] == 'fast'
  assert d('192x128-largest')['lds'] == 4 * pvr.PB_LDS_FLOATS and d('192x128-largest-masked')['body'] == 'general_mask'
  assert [d(n)['top_slot'] for n in ('slot0-P1', 'slot0-P1023', 'slot0-P1024', 'slot1-P1025', 'slot9-P10239',
                                     'slot9-P10240')] == [0, 0, 0, 1, 9, 9]
  assert d('slot9-P10240')['body'] == 'det' and d('general-2pass')['body'] == 'general' and d('general-2pass')['passes'] == 2
  assert (d('chunk3-ragged')['points_per_chunk'], d('chunk3-ragged')['chunks'], d('chunk3-ragged')['ragged']) == (3, 134, True)
  assert (d('chunk4')['points_per_chunk'], d('chunk4')['chunks'], d('chunk4')['ragged']) == (4, 50, False)
  assert (d('128x128-chunk3')['points_per_chunk'], d('128x128-chunk3')['chunks'], d('128x128-chunk3')['ragged']) == (3, 234, True)
  # the suite's two older shapes: one point per chunk, slot 0, under 8 KiB
  for B, Nq, X, Y, P in ((2, 30, 24, 20, 300), (2, 45, 25, 37, 700)):
    o = pvr.dispatch(B, Nq, X, Y, P, False)
    assert (o['points_per_chunk'], o['top_slot'], o['lds_raised']) == (1, 0, False)
  for X, Y in pvr.EXACT_LINES:
    assert pvr.dispatch(2, 5, X, Y, pvr.P_FAST, False)['body'] == 'general'
  assert pvr.chunking(*pvr.SCALE_SHAPE[:2])[0] == 2 and (pvr.SCALE_P - 1) // pvr.PB_THREADS == 2
  assert pvr.POISON_POSE // pvr.PB_THREADS == 2 and pvr.POISON_POSE < pvr.SCALE_P


# ----------------------------------------------------------------------------------------------------
# the exact cases are exact
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X,Y,P,mask', pvr.EXACT_CASES)
def test_exact_cases_have_f32_exact_sums_in_any_order(X, Y, P, mask):
  inp = pvr.exact_case(X, Y, P, mask)
  ref = pvr.model_of(inp)
  assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
  for order in (1, 2):
    assert np.array_equal(pvr.model_of(inp, order=order), ref), order
  # point 0 of scene 0 sits on the targets: every corner from every side, both sides of each clamp, integers
  table = pvr.pose_table(inp['poses'], inp['cell'])
  targets = np.array([(u, v) for u in pvr.axis_targets(X) for v in pvr.axis_targets(Y)])
  n = min(P, len(targets))
  assert np.array_equal(table[0, :n, 2:], targets[:n])
  assert np.array_equal(table[..., 0], np.full(table.shape[:2], 4.0)) and not table[..., 1].any()
  if P >= pvr.P_FAST:
    slots = np.arange(P) // pvr.PB_THREADS
    for t in range(len(targets)):          # every target in slots 0, 5 and 9 with a non-zero cotangent
      live = (np.arange(P) % len(targets) == t) & (inp['dscores'][0] != 0)
      assert {0, 5, 9} <= set(slots[live].tolist()), t
  assert (ref != 0).any() and (inp['dscores'] == 0).any()
  if mask:
    assert not inp['map_valid'].all() and not np.array_equal(ref, pvr.model_of(dict(inp, mask_oob=False)))


def test_the_dyadic_scale_case_stays_normal_under_2_to_minus_120():
  inp = pvr.dyadic_scale_case()
  ref = pvr.model_of(inp)
  assert np.array_equal(pvr.model_of(inp, order=1), ref)
  nz = np.abs(ref[ref != 0])
  assert nz.min() >= 2.0 ** -4 and nz.min() * 2.0 ** -120 >= 2.0 ** -126 and nz.max() * 2.0 ** 100 < 2.0 ** 127
  g = np.abs(inp['dscores'])
  assert g.min() >= 16 and g.max() < 4096


# ----------------------------------------------------------------------------------------------------
# the small kernels' references
# ----------------------------------------------------------------------------------------------------
def test_masked_softmax_rows_bwd_reference_is_autograd():
  rng = np.random.default_rng(3)
  x = torch.tensor(rng.standard_normal((3, 17)), requires_grad=True)
  m = torch.tensor(pvr.softmax_bwd_masks(17, 'ragged'))
  w = torch.softmax(torch.where(m, x, torch.full_like(x, -np.inf)), -1)
  dw = rng.standard_normal((3, 17)).astype(np.float32)
  w32 = w.detach().numpy().astype(np.float32)
  (w * torch.tensor(dw.astype(np.float64))).sum().backward()
  dx, bound = pvr.masked_softmax_rows_bwd(w32, dw)
  assert np.abs(dx - x.grad.numpy()).max() <= 1e-6 and (bound >= 0).all()
  assert (dx[~m.numpy()] == 0).all()


@pytest.mark.parametrize('shape', pvr.SMALL_SHAPES)
def test_sim_bwd_prepare_reference_gates_signed_zeros(shape):
  dsim, sim, coef, row_coef = pvr.small_case(shape)
  B = shape[0]
  G, dot, bound = pvr.sim_bwd_prepare(dsim, sim, True, coef)
  assert G.dtype == np.float32 and not np.signbit(G[sim <= 0]).any() and (G[sim <= 0] == 0).all()
  if sim.size > 1:
    assert (sim == 0).any() and np.signbit(sim[sim == 0]).any() and (sim < 0).any()
  G0, _, _ = pvr.sim_bwd_prepare(dsim, sim, False, coef)
  assert np.array_equal(G0, dsim * coef.reshape(B, 1, 1, 1))
  Gr, rowdot, rb = pvr.sim_bwd_prepare_rows(dsim, sim, True, row_coef)
  assert np.allclose(rowdot.sum(-1), dot, rtol=1e-12, atol=1e-12) and rowdot.shape == shape[:2]
  assert np.array_equal(Gr != 0, (sim > 0) & (dsim * row_coef[:, :, None, None] != 0))
  assert (bound >= 0).all() and (rb >= 0).all()
