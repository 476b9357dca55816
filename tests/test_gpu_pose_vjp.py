"""`-m gpu`: the VJP kernels of ``pose_bwd.hip`` against float64 at their dispatch edges.

**A** an exact planted grid through all four bodies of ``snap_pose_score_bwd_ex_f32`` (bit for bit), **B** random data
cell by cell within tolerances that come from the reference alone, **C** the adjoint identity with ``ops.pose_score``,
**D** the fixed-point scale, **E** the unsupported edge, **F** the small kernels.  Inputs, model, bounds and the
restated launcher live in ``pose_vjp_reference.py``; ``test_pose_vjp_reference.py`` shows on the CPU that every case
is valid and that the tolerances reject the named mutants.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import pose_vjp_reference as pvr
from snap_amd import ops, ops_bwd

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


def dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def vjp(inp, monkeypatch, float_atomics=False, dscores=None):
  monkeypatch.setattr(ops_bwd, 'DETERMINISTIC_POSE_BWD', not float_atomics)
  g = inp['dscores'] if dscores is None else dscores
  out = ops_bwd.pose_score_bwd(dev(g), dev(inp['poses']), dev(inp['q_xy']), dev(inp['valid_q']), dev(inp['map_valid']),
                               tuple(inp['shape']), inp['cell'], mask_oob=inp['mask_oob'])
  return out.cpu().numpy()


def body_of(inp, float_atomics=False):
  B, Nq, X, Y = inp['shape']
  return pvr.dispatch(B, Nq, X, Y, inp['dscores'].shape[1], inp['mask_oob'], float_atomics)['body']


def check(label, got, r, kind):
  ratio, where = pvr.worst(got, r['ref'], r[kind])
  print(f'[pose vjp] {label}: max err / {kind} = {ratio:.4f} at {where} (ref {r["ref"][where]:.6e}, got {got[where]:.6e})')
  return ratio


# ----------------------------------------------------------------------------------------------------
# A. the exact planted grid
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X,Y,P,mask', pvr.EXACT_CASES)
def test_exact_planted_grid_bit_for_bit(X, Y, P, mask, monkeypatch):
  inp = pvr.exact_case(X, Y, P, mask)
  want = pvr.model_of(inp).astype(np.float32)
  line = min(X, Y) == 1
  expect = 'general_mask' if mask else 'general' if (P > pvr.P_FAST or line) else 'det'
  assert body_of(inp) == expect
  runs = [False] + ([True] if expect == 'det' else [])
  for fa in runs:
    got = vjp(inp, monkeypatch, float_atomics=fa)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f'{inp["name"]} {body_of(inp, fa)}: {len(bad)} cells differ; first (b, n, i, j) = '
                           f'{bad[0].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}')


# ----------------------------------------------------------------------------------------------------
# B. random data, cell by cell
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', pvr.VJP_CASE_IDS)
def test_random_case_within_the_reference_tolerance(name, monkeypatch):
  r = pvr.case_reference(name)
  body = body_of(r)
  got = vjp(r, monkeypatch)
  ratios = [check(f'{name} {body}', got, r, 'tol_fixed' if body == 'det' else 'tol_float')]
  zero = bool((got[~r['valid_q']] == 0).all())
  same = True
  if body == 'det':
    same = np.array_equal(vjp(r, monkeypatch).view(np.uint32), got.view(np.uint32))
    flt = vjp(r, monkeypatch, float_atomics=True)
    assert body_of(r, True) == 'fast'
    ratios.append(check(f'{name} fast (float atomics)', flt, r, 'tol_float'))
    zero = zero and bool((flt[~r['valid_q']] == 0).all())
  assert max(ratios) <= 1.0, ratios
  assert zero, 'an invalid point has a non-zero plane'
  assert same, 'two runs of the fixed-point body differ'


# ----------------------------------------------------------------------------------------------------
# C. the adjoint identity with the forward kernel
# ----------------------------------------------------------------------------------------------------
def adjoint_inputs():
  out = [pvr.exact_case(24, 20, pvr.P_FAST, False), pvr.exact_case(24, 20, pvr.P_MASKED, True)]
  return out + [pvr.random_case(pvr.case_by_name(n)) for n in pvr.ADJOINT_CASES]


@pytest.mark.parametrize('k', range(4), ids=['exact-plain', 'exact-masked'] + list(pvr.ADJOINT_CASES))
def test_adjoint_identity_with_pose_score(k, monkeypatch):
  inp = adjoint_inputs()[k]
  r = pvr.reference_of(inp)
  B, Nq, X, Y = inp['shape']
  sim = np.random.default_rng(70 + k).standard_normal(inp['shape']).astype(np.float32)
  args = (sim, inp['poses'], inp['q_xy'], inp['valid_q'], inp['map_valid'], inp['cell'], inp['mask_oob'])
  fwd, mass = pvr.pose_score_fwd(*args, stats=True)
  noise = np.zeros_like(fwd)
  for s in pvr.TWIN_SEEDS:
    noise = np.maximum(noise, np.abs(pvr.pose_score_fwd(*args, twin=s) - fwd))
  tol_fwd = pvr.MARGIN * noise + 4 * Nq * pvr.U * mass
  scores = ops.pose_score(dev(sim), dev(inp['poses']), dev(inp['q_xy']), dev(inp['valid_q']), dev(inp['map_valid']),
                          inp['cell'], mask_oob=inp['mask_oob']).cpu().numpy().astype(np.float64)
  g = pvr.f64(inp['dscores'])
  for fa in ([False, True] if body_of(inp) == 'det' else [False]):
    dsim = vjp(inp, monkeypatch, float_atomics=fa).astype(np.float64)
    kind = 'tol_fixed' if body_of(inp, fa) == 'det' else 'tol_float'
    lhs, rhs = float((g * scores).sum()), float((dsim * sim).sum())
    bound = float((np.abs(g) * tol_fwd).sum() + (np.abs(sim) * r[kind]).sum())
    print(f'[pose vjp] adjoint {inp["name"]} {body_of(inp, fa)}: <g, fwd> {lhs:.9e} <vjp, sim> {rhs:.9e} '
          f'diff {abs(lhs - rhs):.3e} bound {bound:.3e}; float64 value {float((g * fwd).sum()):.9e}')
    assert abs(lhs - rhs) <= bound


# ----------------------------------------------------------------------------------------------------
# D. the fixed-point scale
# ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scale_reference():
  return pvr.reference_of(pvr.scale_case())


def test_scale_zero_cotangents_give_positive_zero(monkeypatch):
  r = scale_reference()
  assert body_of(r) == 'det'
  got = vjp(r, monkeypatch, dscores=np.zeros_like(r['dscores']))
  assert not got.view(np.uint32).any()


@pytest.mark.parametrize('exp', [-120, 100])
def test_scale_power_of_two_is_exact_on_dyadic_data(exp, monkeypatch):
  inp = pvr.dyadic_scale_case()
  assert body_of(inp) == 'det'
  base = vjp(inp, monkeypatch)
  assert np.array_equal(base, pvr.model_of(inp).astype(np.float32))
  k = np.float32(2.0 ** exp)
  got = vjp(inp, monkeypatch, dscores=inp['dscores'] * k)
  nz = np.abs(base[base != 0]).astype(np.float64) * 2.0 ** exp
  assert nz.min() >= 2.0 ** -126 and nz.max() < 2.0 ** 127             # normal before and after
  assert np.array_equal(got, base * k)


def test_scale_2_to_100_is_exact_on_random_data(monkeypatch):
  r = scale_reference()
  base = vjp(r, monkeypatch)
  assert check('scale case det', base, r, 'tol_fixed') <= 1.0
  k = np.float32(2.0 ** 100)
  got = vjp(r, monkeypatch, dscores=r['dscores'] * k)
  assert np.array_equal(got, base * k)


def test_scale_one_large_cotangent_among_tiny_ones(monkeypatch):
  inp = pvr.scale_case()
  rng = np.random.default_rng(43)
  g = (rng.choice([-1.0, 1.0], inp['dscores'].shape) * 2.0 ** -30).astype(np.float32)
  g[:, pvr.PB_THREADS + 5] = 1.0
  r = pvr.reference_of(dict(inp, dscores=g))
  assert (pvr.scale_exponent(g)[0] == 1).all()
  got = vjp(r, monkeypatch)
  assert check('1.0 among 2^-30', got, r, 'tol_fixed') <= 1.0
  assert check('1.0 among 2^-30, float atomics', vjp(r, monkeypatch, float_atomics=True), r, 'tol_float') <= 1.0


@pytest.mark.parametrize('poison', [float('nan'), float('inf'), -float('inf')])
def test_scale_non_finite_cotangent_poisons_its_scene_only(poison, monkeypatch):
  r = scale_reference()
  vq = r['valid_q']
  clean = vjp(r, monkeypatch)
  g = r['dscores'].copy()
  g[0, pvr.POISON_POSE] = poison
  bad = vjp(r, monkeypatch, dscores=g)
  assert not np.isfinite(bad[0][vq[0]]).any(), 'a cell of a valid plane of the poisoned scene is finite'
  assert not bad[0][~vq[0]].view(np.uint32).any()
  assert np.array_equal(bad[1].view(np.uint32), clean[1].view(np.uint32))
  flt = vjp(r, monkeypatch, float_atomics=True, dscores=g)
  assert not np.isfinite(flt[0]).all() and (flt[0][~vq[0]] == 0).all()
  one = {k: (v[1:] if isinstance(v, np.ndarray) and v.shape[:1] == (2,) else v) for k, v in r.items()}
  assert check(f'float atomics next to {poison}', flt[1:], one, 'tol_float') <= 1.0


# ----------------------------------------------------------------------------------------------------
# E. unsupported shapes
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('X,Y', pvr.UNSUPPORTED_SHAPES)
def test_a_plane_above_24576_cells_is_refused(X, Y, monkeypatch):
  inp = pvr.random_case(('refused', 1, 1, 5, X, Y, 100, False))
  assert not pvr.dispatch(1, 5, X, Y, 100, False)['supported']
  for fa in (False, True):
    with pytest.raises(RuntimeError, match='snap_pose_score_bwd_ex_f32'):
      vjp(inp, monkeypatch, float_atomics=fa)
  assert pvr.dispatch(1, 5, 192, 128, 100, False)['supported']       # (192 x 128 runs: the table's last rows)


# ----------------------------------------------------------------------------------------------------
# F. the small kernels
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('shape', pvr.SMALL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sim_bwd_prepare_exact_products_and_bounded_sums(shape, clip):
  dsim, sim, coef, row_coef = pvr.small_case(shape)
  G, dot, bound = pvr.sim_bwd_prepare(dsim, sim, clip, coef)
  d = dev(dsim).clone()
  got_dot = ops_bwd.sim_bwd_prepare_(d, dev(sim), clip, dev(coef)).cpu().numpy().astype(np.float64)
  got = d.cpu().numpy()
  assert np.array_equal(got, G)
  if clip:
    assert not got[sim <= 0].view(np.uint32).any()                   # a closed gate writes +0.0
  err = np.abs(got_dot - dot)
  print(f'[pose vjp] sim_bwd_prepare {shape} clip={clip}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.4f}')
  assert (err <= bound).all()
  Gr, rowdot, rbound = pvr.sim_bwd_prepare_rows(dsim, sim, clip, row_coef)
  d = dev(dsim).clone()
  got_rd = ops_bwd.sim_bwd_prepare_rows_(d, dev(sim), clip, dev(row_coef)).cpu().numpy().astype(np.float64)
  got = d.cpu().numpy()
  assert np.array_equal(got, Gr)
  if clip:
    assert not got[sim <= 0].view(np.uint32).any()
  err = np.abs(got_rd - rowdot)
  print(f'[pose vjp] sim_bwd_prepare_rows {shape} clip={clip}: max err / bound {np.max(err / np.maximum(rbound, 1e-300)):.4f}')
  assert (err <= rbound).all()


@pytest.mark.parametrize('kind', pvr.SOFTMAX_BWD_MASKS)
@pytest.mark.parametrize('N', pvr.SOFTMAX_BWD_N)
def test_masked_softmax_rows_bwd(N, kind):
  rng = np.random.default_rng([71, N])
  x = rng.standard_normal((3, N)).astype(np.float32) * 2
  dw = rng.standard_normal((3, N)).astype(np.float32)
  m = pvr.softmax_bwd_masks(N, kind)
  w, _ = ops.masked_softmax_rows(dev(x), dev(m))
  got = ops_bwd.masked_softmax_rows_bwd(w, dev(dw)).cpu().numpy().astype(np.float64)
  w = w.cpu().numpy()
  support = m if kind != 'all false' else np.ones_like(m)
  assert (w[~support] == 0).all() and (w[support] > 0).all()
  want, bound = pvr.masked_softmax_rows_bwd(w, dw)
  err = np.abs(got - want)
  print(f'[pose vjp] masked_softmax_rows_bwd N={N} {kind}: max err / bound '
        f'{np.max(np.where(err == 0, 0, err / np.maximum(bound, 1e-300))):.4f}')
  assert (err <= bound).all()
  assert (got[~support] == 0).all()


def rnd(shape, seed, scale=1.0):
  return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dtemp_check(name, got, dsim, sim_gpu, terms_per_sum, extra_terms):
  prod = dsim.double().cpu() * sim_gpu.double().cpu()
  want = float(prod.sum())
  bound = (terms_per_sum + extra_terms) * pvr.U * float(prod.abs().sum()) + pvr.U * abs(want)
  print(f'[pose vjp] {name} d temperature: got {float(got):.9e} want {want:.9e} err {abs(float(got) - want):.3e} '
        f'bound {bound:.3e}')
  assert abs(float(got) - want) <= bound


@pytest.mark.parametrize('B,Nq,X,Y,Dm', pvr.SIMILARITY_SHAPES)
def test_similarity_bwd_num_valid_form(B, Nq, X, Y, Dm):
  from snap_amd import autograd as ag
  fq = F.normalize(rnd((B, Nq, Dm), 410), dim=-1)
  fm = F.normalize(rnd((B, X, Y, Dm), 411), dim=-1)
  nv = torch.tensor([float(Nq - 2), float(Nq)][:B])
  temp = torch.tensor(2.0)
  dsim = rnd((B, Nq, X, Y), 412)
  fqd, fmd, td = (t.double().requires_grad_(True) for t in (fq, fm, temp))
  sim = torch.relu(torch.einsum('bnd,bijd->bnij', fqd, fmd)) * torch.exp(td) / nv.double()[:, None, None, None]
  sim.backward(dsim.double())
  scale = float(torch.exp(temp))
  if Dm <= 64:
    simg, _, _, _ = ops.sim_softmax(fq.to(DEV), fm.to(DEV), scale, True, nv.to(DEV))
  else:            # the forward similarity kernel takes Dm <= 64; the VJP takes any: hand it the float64 forward
    simg = sim.detach().float().to(DEV)
  dfq, dfm, dtemp = ag.similarity_bwd(dsim.to(DEV).clone(), simg, fq.to(DEV), fm.to(DEV), scale, True, nv.to(DEV))
  helpers.report('dfq', dfq, fqd.grad.float(), atol=3e-4 * float(fqd.grad.abs().max()))
  helpers.report('dfm', dfm, fmd.grad.float(), atol=3e-4 * float(fmd.grad.abs().max()))
  dtemp_check(f'similarity {B, Nq, X, Y, Dm}', dtemp, dsim, simg, Nq * X * Y, B)


@pytest.mark.parametrize('B,Nq,X,Y,Dm', pvr.SIMILARITY_SHAPES)
def test_similarity_bwd_row_weight_form(B, Nq, X, Y, Dm):
  from snap_amd import autograd as ag
  fq = F.normalize(rnd((B, Nq, Dm), 420), dim=-1)
  fm = F.normalize(rnd((B, X, Y, Dm), 421), dim=-1)
  conf = rnd((B, Nq), 422)
  valid = torch.rand((B, Nq), generator=torch.Generator().manual_seed(423)) > 0.2
  nv = valid.sum(-1).float()
  temp = torch.tensor(2.0)
  dsim = rnd((B, Nq, X, Y), 424)
  fqd, fmd, td, cd = (t.double().requires_grad_(True) for t in (fq, fm, temp, conf))
  wref = torch.softmax(torch.where(valid, cd, torch.full_like(cd, -math.inf)), -1)
  simr = torch.relu(torch.einsum('bnd,bxyd->bnxy', fqd, fmd)) * torch.exp(td) * wref[..., None, None]
  simr.backward(dsim.double())
  if Dm > 64:      # the forward similarity kernel takes Dm <= 64; the VJP takes any: hand it the float64 forward
    w, _ = ops.masked_softmax_rows(conf.to(DEV), valid.to(DEV))
    sim_out = simr.detach().float().to(DEV)
    dfq, dfm, dtemp, dweight = ag.similarity_bwd(dsim.to(DEV).clone(), sim_out, fq.to(DEV), fm.to(DEV),
                                                 float(torch.exp(temp)), True, nv.to(DEV), row_weight=w)
    dconf = ops_bwd.masked_softmax_rows_bwd(w, dweight.contiguous())
    for name, got, want in (('fq', dfq, fqd), ('fm', dfm, fmd), ('confidence', dconf, cd)):
      helpers.report(f'weighted sim d {name}', got, want.grad.float(), atol=3e-4 * float(want.grad.abs().max()))
    assert bool((dconf[~valid.to(DEV)] == 0).all())
    dtemp_check(f'weighted similarity {B, Nq, X, Y, Dm}', dtemp, dsim, sim_out, X * Y, B * Nq)
    return
  fqg, fmg, tg, cg = (t.to(DEV).requires_grad_(True) for t in (fq, fm, temp, conf))
  wg, _ = ag.masked_softmax_rows(cg, valid.to(DEV))
  sim, _, _, _ = ag.sim_softmax_weighted(fqg, fmg, tg, wg, True, nv.to(DEV))
  sim_out = sim.detach().clone()
  sim.backward(dsim.to(DEV))
  for name, got, want in (('fq', fqg, fqd), ('fm', fmg, fmd), ('confidence', cg, cd)):
    helpers.report(f'weighted sim d {name}', got.grad, want.grad.float(), atol=3e-4 * float(want.grad.abs().max()))
  assert bool((cg.grad[~valid.to(DEV)] == 0).all())
  dtemp_check(f'weighted similarity {B, Nq, X, Y, Dm}', tg.grad, dsim, sim_out, X * Y, B * Nq)
