"""`-m gpu`: the RANSAC pose chain of ``pose.hip`` against float64 references at its edges.

``argmax_rows`` (NaN, +-inf, both kernel widths), ``poses_from_corr`` (every pose accounted for, planted
selections and degenerate pairs), ``ransac_sample`` (the multi-chunk walk of all three bodies against the inverse
CDF), ``pose_score`` (planted geometry and one rotated case on every body, the window body bit for bit) and
``masked_softmax_rows`` (small and ragged N).  Inputs, references, bounds and the restated dispatch rules live in
``pose_chain_reference.py``; ``test_pose_chain_reference.py`` shows on the CPU that every input satisfies its
stated condition on the reference alone.  Every escape below is a named class with a cap, and is printed.
"""
import functools

import numpy as np
import pytest
import torch

import helpers
import oracle_ops
import pose_chain_reference as pcr
from snap_amd import ops

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------
# A. argmax_rows: NaN is the maximum, the first NaN wins (np.argmax)
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('start', [0, 7])
@pytest.mark.parametrize('width', pcr.ARGMAX_WIDTHS)
def test_argmax_rows_is_np_argmax_on_nan_and_inf_rows(width, start):
  s, names = pcr.argmax_case_rows(width, start)
  assert s.shape[1] - start == width and pcr.argmax_threads(width) == (256 if width == 4096 else 1024)
  got = ops.argmax_rows(dev(s), start).cpu().numpy()
  want = pcr.argmax_want(s, start)
  bad = [f'{names[r]}: got {got[r]} want {want[r]}' for r in range(len(names)) if got[r] != want[r]]
  assert not bad, bad


def test_argmax_rows_of_one_element():
  nan, inf = np.float32(np.nan), np.float32(np.inf)
  s = np.random.default_rng(1).standard_normal((5, 300)).astype(np.float32)
  s[:, 299] = [nan, -inf, inf, 1.0, -1.0]
  s[0, 10] = inf
  s[1, 20] = nan
  got = ops.argmax_rows(dev(s), 299).cpu().numpy()
  assert np.array_equal(got, pcr.argmax_want(s, 299)) and not got.any()


@pytest.mark.parametrize('width,extent', [(4096, (64, 64)), (4097, (17, 241))])
def test_argmax_nd_on_nan_rows(width, extent):
  from snap_amd.utils import grids as g
  s, names = pcr.argmax_case_rows(width, 0)
  want = np.stack(np.unravel_index(np.argmax(s, -1), extent), -1)
  got = g.argmax_nd(dev(s.reshape(len(s), *extent)), g.GridND(tuple(extent), 0.5)).cpu().numpy()
  bad = [f'{names[r]}: got {got[r]} want {want[r]}' for r in range(len(names)) if not np.array_equal(got[r], want[r])]
  assert not bad, bad


# ----------------------------------------------------------------------------------------------------
# B. poses_from_corr
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pcr.POSE_RANDOM_CASES, ids=lambda c: f'retries{c[4]}')
def test_poses_from_corr_accounts_for_every_pose(case):
  seed, B, Nq, P, retries, X, Y, cell = case
  corr, q_xy = pcr.corr_random(seed, B, Nq, P, retries, X, Y)
  got = ops.poses_from_corr(dev(corr), dev(q_xy), P, retries, cell).cpu().numpy()
  pcr.check_poses_rule_b(f'random, retries {retries}', got, corr, q_xy, P, retries, cell)


def test_poses_from_corr_planted_selection_and_degenerate_pairs():
  pi32 = np.float32(np.pi)
  for name, corr, q_xy, retries, winner, kind in pcr.planted_pose_cases():
    got = ops.poses_from_corr(dev(corr), dev(q_xy), 1, retries, pcr.CELL).cpu().numpy()
    ref = pcr.poses_ref64(corr, q_xy, 1, retries, pcr.CELL)
    m, _ = pcr.match_poses(got, ref)
    assert m[0, 0] == winner, f'{name}: got {got[0, 0]}, retry {winner} gives {ref["pose"][0, 0, winner]}'
    w = ref['pose'][0, 0, winner]
    if kind == 'degenerate':
      assert got[0, 0, 0] == 0.0 and np.array_equal(got[0, 0, 1:], w[1:].astype(np.float32)), (name, got[0, 0])
    if kind == 'antipodal':
      assert abs(got[0, 0, 0]) == pi32 and np.array_equal(got[0, 0, 1:], w[1:].astype(np.float32)), (name, got[0, 0])


# ----------------------------------------------------------------------------------------------------
# C. ransac_sample: table-free, table, and the four-per-wave kernel (table + sim + row_unscale)
# ----------------------------------------------------------------------------------------------------
BODIES = ('table-free', 'table', 'fast')


def draw(body, fq, fm, stats, scale, clip, u, sim, unscale, row_cdf=None):
  S = u.shape[1]
  if body == 'table-free':
    return ops.ransac_sample(fq, fm, stats, scale, clip, S, uniforms=u, row_table=False, row_cdf=row_cdf)
  if body == 'table':
    return ops.ransac_sample(fq, fm, stats, scale, clip, S, uniforms=u, row_cdf=row_cdf)
  return ops.ransac_sample(fq, fm, stats, scale, clip, S, uniforms=u, row_cdf=row_cdf, sim=sim, row_unscale=unscale)


@functools.lru_cache(maxsize=None)
def sampler_reference(X, Y, clip):
  fq, fm, u = pcr.sampler_random_inputs(X, Y, pcr.SAMPLER_SEEDS[(X, Y)])
  return (fq, fm, u) + pcr.sampler_ref(fq, fm, pcr.SAMPLER_SCALE, clip, u)


def check_cells(name, got, rows, cells, cdf, u, Y):
  """The acceptance rule of test_ransac_sample_given_uniforms: the row exactly; the oracle's cell, or a cell whose
  float64 CDF brackets the uniform within 1e-5 of the row mass.  Returns how many samples needed the bracket."""
  got = got.cpu().numpy().astype(np.int64)
  assert np.array_equal(got[..., 0], rows), f'{name}: query row selection differs'
  gc = got[..., 1] * Y + got[..., 2]
  assert (got[..., 1] >= 0).all() and (got[..., 2] >= 0).all() and (got[..., 2] < Y).all() and (gc < cdf.shape[-1]).all()
  differ = gc != cells
  ok = pcr.bracketed(cdf, rows, gc, u[..., 1])
  assert (ok | ~differ).all(), f'{name}: {int((differ & ~ok).sum())} samples outside their CDF bracket'
  return int(differ.sum())


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('X,Y', pcr.SAMPLER_SHAPES)
def test_ransac_sample_multi_chunk_walk_against_the_inverse_cdf(X, Y, clip):
  assert pcr.fast_sampler_dispatch(X, Y)
  fq, fm, u, rows, cells, cdf = sampler_reference(X, Y, clip)
  B, Nq = fq.shape[:2]
  nv = torch.full((B,), float(Nq), device=DEV)
  fq_d, fm_d, u_d = dev(fq), dev(fm), dev(u)
  sim, stats, _, _ = ops.sim_softmax(fq_d, fm_d, pcr.SAMPLER_SCALE, clip, nv, math='f32')
  unscale = nv[:, None].expand(B, Nq).contiguous()
  for body in BODIES:
    got = draw(body, fq_d, fm_d, stats, pcr.SAMPLER_SCALE, clip, u_d, sim, unscale)
    n = check_cells(f'{X}x{Y} {body}', got, rows, cells, cdf, u, Y)
    print(f'[sampler] {X}x{Y} clip={clip} {body}: {n} of {rows.size} samples needed the bracket')
    assert n <= 0.02 * rows.size


@pytest.mark.parametrize('X,Y', pcr.SAMPLER_SHAPES)
def test_ransac_sample_one_hot_rows_return_their_target(X, Y):
  fq, fm, u, tg = pcr.one_hot_inputs(X, Y)
  B = len(tg)
  nv = torch.ones(B, device=DEV)                    # sim = x exactly: the fast kernel reads the same scores
  fq_d, fm_d, u_d = dev(fq), dev(fm), dev(u)
  sim, stats, _, _ = ops.sim_softmax(fq_d, fm_d, pcr.ONE_HOT_SCALE, True, nv, math='f32')
  unscale = torch.ones(B, 1, device=DEV)
  for body in BODIES:
    got = draw(body, fq_d, fm_d, stats, pcr.ONE_HOT_SCALE, True, u_d, sim, unscale).cpu().numpy().astype(np.int64)
    gc = got[..., 1] * Y + got[..., 2]
    bad = np.argwhere((gc != tg[:, None]) | (got[..., 0] != 0))
    assert len(bad) == 0, (f'{X}x{Y} {body}: {len(bad)} samples off their target; first: target {tg[bad[0][0]]} '
                           f'u2 {u[tuple(bad[0])][1]} got {got[tuple(bad[0])]}')


def test_ransac_sample_rows_through_the_confidence_cdf():
  X, Y, clip = 65, 64, True
  fq, fm, u, _, _, _ = sampler_reference(X, Y, clip)
  B, Nq = fq.shape[:2]
  u = u.copy()
  u[:, 0, 0] = 1 - 2.0 ** -24                       # the largest uniform: the last row that has any weight
  u[:, 1, 0] = 0.0
  rng = np.random.default_rng(5)
  conf = rng.standard_normal((B, Nq)).astype(np.float32) * 2
  mask = np.ones((B, Nq), bool)
  mask[:, ::3] = False                              # weight exactly 0, row 0 among them
  mask[1, Nq - 1] = False                           # scene 1: the last row has no weight either
  w, row_cdf = ops.masked_softmax_rows(dev(conf), dev(mask))
  w, c = w.cpu().numpy(), row_cdf.cpu().numpy()
  assert (w[~mask] == 0).all() and (w[mask] > 0).all()
  rows, cells, cdf = pcr.sampler_ref(fq, fm, pcr.SAMPLER_SCALE, clip, u, row_cdf=c)
  assert rows[0, 0] == Nq - 1 and rows[1, 0] == np.nonzero(mask[1])[0][-1] and (rows[:, 1] == 1).all()
  nv = torch.full((B,), float(Nq), device=DEV)
  fq_d, fm_d, u_d = dev(fq), dev(fm), dev(u)
  sim, stats, _, _ = ops.sim_softmax(fq_d, fm_d, pcr.SAMPLER_SCALE, clip, nv, math='f32')
  unscale = nv[:, None].expand(B, Nq).contiguous()
  for body in BODIES:
    got = draw(body, fq_d, fm_d, stats, pcr.SAMPLER_SCALE, clip, u_d, sim, unscale, row_cdf=row_cdf)
    n = check_cells(f'row_cdf {body}', got, rows, cells, cdf, u, Y)
    g = got.cpu().numpy()
    assert mask[np.arange(B)[:, None], g[..., 0]].all(), f'{body}: a row of weight 0 was drawn'
    assert n <= 0.02 * rows.size


# ----------------------------------------------------------------------------------------------------
# D. pose_score
# ----------------------------------------------------------------------------------------------------
ATOL, RTOL = 2e-4, 1e-5


@pytest.mark.parametrize('X,Y,mask,body', pcr.POSE_SCORE_SHAPES)
def test_pose_score_planted_geometry_on_every_body(X, Y, mask, body, monkeypatch):
  got_body, RB, NB, seams = pcr.pose_score_body(X, Y, mask)
  assert got_body == body                                  # the dispatch rule of snap_pose_score_f32, restated
  monkeypatch.setattr(oracle_ops, 'DTYPE', np.float64)
  poses1 = pcr.planted_poses(X, Y)
  B, Nq, P = 4, len(pcr.PLANT_Q), len(poses1)
  rng = np.random.default_rng(X * 1000 + Y)
  sim = rng.random((B, Nq, X, Y), dtype=np.float32)
  poses = np.broadcast_to(poses1, (B, P, 3)).copy()
  q_xy = np.broadcast_to(pcr.PLANT_Q, (B, Nq, 2)).copy()
  vq = np.ones((B, Nq), bool)
  vq[3, 4] = False
  mv = pcr.planted_map_valid(X, Y, seams) if mask else None      # scene k: one invalid cell under tap k of the probe
  t = torch.from_numpy
  got = ops.pose_score(dev(sim), dev(poses), dev(q_xy), dev(vq), None if mv is None else dev(mv), pcr.CELL,
                       mask_oob=mask)
  want = oracle_ops.pose_score(t(sim), t(poses), t(q_xy), t(vq), None if mv is None else t(mv), pcr.CELL,
                               mask_oob=mask)
  helpers.report(f'planted pose scores {X}x{Y} {body}', got, want, atol=ATOL, rtol=RTOL)
  # the valid set, exactly: plane n is the constant 2^n, every bilinear value is 2^n, a score is the bit mask
  # of the points that entered it
  sim2 = np.broadcast_to((2.0 ** np.arange(Nq, dtype=np.float32))[None, :, None, None], sim.shape).copy()
  got2 = ops.pose_score(dev(sim2), dev(poses), dev(q_xy), dev(vq), None if mv is None else dev(mv), pcr.CELL,
                        mask_oob=mask).cpu().numpy()
  for b in range(B):
    want2, ok = pcr.scores64(sim2[b], poses[b], q_xy[b], vq[b], None if mv is None else mv[b], pcr.CELL, mask)
    bad = np.nonzero(got2[b] != want2)[0]
    assert len(bad) == 0, (f'{X}x{Y} {body} scene {b}: {len(bad)} poses with another valid set; first: pose '
                           f'{poses[b, bad[0]]} mask {got2[b, bad[0]]} want {want2[bad[0]]}')


@pytest.mark.parametrize('X,Y,mask,body', pcr.POSE_SCORE_SHAPES)
def test_pose_score_rotated_poses_on_every_body(X, Y, mask, body):
  assert pcr.pose_score_body(X, Y, mask)[0] == body
  sim, poses, q_xy, vq, mv, cell = pcr.rotated_case(X, Y, 110 + X)
  got = ops.pose_score(dev(sim), dev(poses), dev(q_xy), dev(vq), dev(mv), cell, mask_oob=mask).cpu().numpy()
  flips = near = 0
  for b in range(sim.shape[0]):
    if mask:
      f, n = pcr.explain_by_border_flips(got[b], sim[b], poses[b], q_xy[b], vq[b], mv[b], np.float64(np.float32(cell)),
                                         ATOL, RTOL)
      flips, near = flips + f, near + n
    else:
      want, _ = pcr.scores64(sim[b], poses[b], q_xy[b], vq[b], mv[b], np.float64(np.float32(cell)), False)
      helpers.report(f'rotated pose scores {X}x{Y} {body}', got[b], want.astype(np.float32), atol=ATOL, rtol=RTOL)
  if mask:
    print(f'[pose_score] {X}x{Y} {body}: {flips} pose(s) explained by a border flip; {near} point samples lie '
          f'within {pcr.BORDER_TOL} cell of a border')
    assert flips <= near


def test_pose_score_window_is_the_general_body_on_the_planted_edges():
  X, Y, rad = pcr.WINDOW_SHAPE
  assert ops.pose_score_window_supported(X, Y, rad) and pcr.window_supported(X, Y, rad)
  assert pcr.pose_score_body(X, Y, False)[0] == 'db'
  centres_uv = [(1.0, 1.0), (X - 1.0, Y - 1.0), (X / 2, Y / 2 + 0.25), (0.25, Y - 0.5)]
  B, Nq = len(centres_uv), len(pcr.PLANT_Q)
  sets = [pcr.planted_poses(X, Y, (cu - rad + 0.25, cu + rad - 0.25), (cv - rad + 0.25, cv + rad - 0.25))
          for cu, cv in centres_uv]
  P = max(len(s) for s in sets)
  poses = np.stack([np.concatenate([s, np.repeat(s[:1], P - len(s), 0)]) for s in sets])
  centers = np.array([[0.0, cu * pcr.CELL - pcr.PLANT_Q[0, 0], cv * pcr.CELL - pcr.PLANT_Q[0, 1]]
                      for cu, cv in centres_uv], np.float32)
  # the promise, in cells: theta = 0, so every point moves by the translation difference
  assert np.abs((poses[..., 1:] - centers[:, None, 1:]) / pcr.CELL).max() <= rad - 0.25
  u0 = (poses[..., 1] + pcr.PLANT_Q[0, 0]) / pcr.CELL
  assert (u0 == 0).any() and (u0 == X).any() and (u0 < 0).any() and (u0 == X - 2.0 ** -6).any()
  rng = np.random.default_rng(9)
  sim = rng.standard_normal((B, Nq, X, Y)).astype(np.float32)
  q_xy = np.broadcast_to(pcr.PLANT_Q, (B, Nq, 2)).copy()
  vq = np.ones((B, Nq), bool)
  vq[2, 1] = False
  gen = ops.pose_score(dev(sim), dev(poses), dev(q_xy), dev(vq), None, pcr.CELL)
  win = ops.pose_score_window(dev(sim), dev(poses), dev(centers), rad, dev(q_xy), dev(vq), pcr.CELL)
  assert torch.equal(win, gen), float((win - gen).abs().max())
  for b in range(B):
    want, _ = pcr.scores64(sim[b], poses[b], q_xy[b], vq[b], None, pcr.CELL, False)
    helpers.report('window, planted edges', win[b], want.astype(np.float32), atol=ATOL, rtol=RTOL)


# ----------------------------------------------------------------------------------------------------
# E. masked_softmax_rows
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', pcr.SOFTMAX_N)
def test_masked_softmax_rows_small_and_ragged(N):
  x, m = pcr.softmax_case(N)
  w, cdf = ops.masked_softmax_rows(dev(x), dev(m))
  w, cdf = w.cpu().numpy(), cdf.cpu().numpy()
  want_w, want_c = pcr.softmax_want(x, m)
  helpers.report(f'masked softmax rows N={N}', w, want_w.astype(np.float32), atol=1e-8, rtol=2e-5)
  helpers.report(f'masked softmax cdf N={N}', cdf, want_c.astype(np.float32), atol=2e-6, rtol=2e-5)
  for r, name in enumerate(pcr.SOFTMAX_ROWS):
    if m[r].any():
      assert (w[r][~m[r]] == 0).all(), name
    assert abs(float(cdf[r, -1]) - 1.0) <= 2e-6, (name, cdf[r, -1])
    assert (np.diff(cdf[r]) >= 0).all(), name
    # an entry of weight 0 adds nothing, bit for bit: the sampler's search can never return its row
    step = np.diff(np.concatenate([[np.float32(0)], cdf[r]]))
    assert (step[w[r] == 0] == 0).all(), name
