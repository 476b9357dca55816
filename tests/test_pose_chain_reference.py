"""CPU side of the pose chain tests: every input of ``test_gpu_pose_chain.py`` satisfies its stated condition
on the float64 reference alone, and the restatements of ``pose_chain_reference.py`` agree with ``oracle/``.
No kernel runs here; the GPU file then has no escape hatch of its own."""
import numpy as np
import pytest
import torch

import oracle_ops
import pose_chain_reference as pcr
from oracle import pose as o_pose


# -- A. argmax -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('start', [0, 7])
@pytest.mark.parametrize('width', pcr.ARGMAX_WIDTHS)
def test_argmax_rows_reference_is_first_nan_else_first_maximum(width, start):
  s, names = pcr.argmax_case_rows(width, start)
  want = pcr.argmax_want(s, start)
  assert np.array_equal(want, oracle_ops.argmax_rows(torch.from_numpy(s), start).numpy())
  for r, name in enumerate(names):
    row = s[r, start:]
    nan = np.nonzero(np.isnan(row))[0]
    first = nan[0] if len(nan) else np.nonzero(row == row.max())[0][0]
    assert want[r] == first, name
  NT = pcr.argmax_threads(width)
  assert {names[r]: want[r] for r in range(len(names))}['nan@NT behind a larger value of the same thread'] == NT
  assert width > 2 * NT + 3 and (NT == 1024) == (width > 4096)


# -- B. poses_from_corr --------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pcr.POSE_RANDOM_CASES, ids=lambda c: f'retries{c[4]}')
def test_random_poses_have_few_near_ties_and_the_closed_form_is_the_svd(case):
  seed, B, Nq, P, retries, X, Y, cell = case
  corr, q_xy = pcr.corr_random(seed, B, Nq, P, retries, X, Y)
  ref = pcr.poses_ref64(corr, q_xy, P, retries, cell)
  ties = int((pcr.near_tie_candidates(ref['ratio']).sum(-1) > 1).sum())
  print(f'[poses] retries {retries}: {ties} of {B * P} poses have a second retry within 2^-20 of the minimum')
  if retries > 1:
    assert ties <= 0.005 * B * P              # half the GPU test's cap of 1 %
  # the selected pair through the SVD (oracle.pose.kabsch_algorithm_2d) in float64
  worst = 0.0
  for b in range(B):
    for p in range(P):
      r = ref['sel'][b, p]
      tf, _, _ = o_pose.kabsch_algorithm_2d(ref['j_xy'][b, p, r], ref['i_xy'][b, p, r])
      w = ref['pose'][b, p, r]
      worst = max(worst, pcr.wrap(float(tf.angle) - w[0]), np.abs(np.asarray(tf.t) - w[1:]).max())
  assert worst < 1e-9, worst
  # the bound is finite and small wherever the pair is not degenerate; the self-match is exact
  sel = np.take_along_axis(ref['b_ang'], ref['sel'][..., None], -1)
  assert np.isfinite(sel).all() and pcr.MARGIN * sel.max() < 1e-3, sel.max()
  got = np.take_along_axis(ref['pose'], ref['sel'][..., None, None].repeat(3, -1), 2)[:, :, 0]
  m, frac = pcr.match_poses(got, ref)
  assert np.array_equal(m, ref['sel']) and frac == 0.0
  # a wrong retry is not a match (translations of different retries differ by far more than the bound)
  if retries > 1:
    other = np.take_along_axis(ref['pose'], ((ref['sel'] + 1) % retries)[..., None, None].repeat(3, -1), 2)[:, :, 0]
    assert (pcr.match_poses(other, ref)[0] == -1).mean() > 0.99


def test_planted_pose_cases_select_and_degenerate_as_stated():
  for name, corr, q_xy, retries, winner, kind in pcr.planted_pose_cases():
    assert np.array_equal(q_xy * 8, np.round(q_xy * 8)), name
    ref = pcr.poses_ref64(corr, q_xy, 1, retries, pcr.CELL)
    assert ref['sel'][0, 0] == winner, name
    ratio = ref['ratio'][0, 0]
    # every ratio is exact in f32 as well: the same bits decide on both sides
    assert np.array_equal(ratio.astype(np.float32).astype(np.float64), ratio), name
    if name == 'equal ratios, first wins':
      assert ratio[0] == ratio[1] < ratio[2] and np.abs(ref['pose'][0, 0, 0, 1:] - ref['pose'][0, 0, 1, 1:]).max() > 0.1
    if name == 'smaller ratio last':
      assert ratio[2] < ratio[1] < ratio[0]
    w = ref['pose'][0, 0, winner]
    i_xy, j_xy = ref['i_xy'][0, 0, winner], ref['j_xy'][0, 0, winner]
    tf, _, _ = o_pose.kabsch_algorithm_2d(j_xy, i_xy)
    assert pcr.wrap(float(tf.angle) - w[0]) < 1e-12 and np.abs(np.asarray(tf.t) - w[1:]).max() < 1e-12, name
    if kind == 'degenerate':
      assert w[0] == 0.0 and np.array_equal(w[1:], j_xy.mean(0) - i_xy.mean(0)), name
    if kind == 'antipodal':
      assert abs(w[0]) == np.pi and np.array_equal(w[1:], j_xy.mean(0) + i_xy.mean(0)), name


# -- C. ransac_sample ----------------------------------------------------------------------------------
def test_sampler_shapes_reach_the_multi_chunk_walk_and_the_fast_kernel():
  want = {(65, 64): (65, 2), (67, 63): (66, 2), (5, 7): (1, 1), (128, 66): (132, 3)}
  for X, Y in pcr.SAMPLER_SHAPES:
    assert pcr.chunks_per_lane(X, Y) == want[(X, Y)]
    assert pcr.fast_sampler_dispatch(X, Y)
  assert 67 * 63 - 65 * 64 == 61                      # the ragged last chunk
  assert 65 - 32 * 2 == 1                             # lane 32 owns chunk 64 alone, lanes 33 .. 63 nothing


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('X,Y', pcr.SAMPLER_SHAPES)
def test_sampler_random_inputs_stay_clear_of_cdf_edges(X, Y, clip):
  fq, fm, u = pcr.sampler_random_inputs(X, Y, pcr.SAMPLER_SEEDS[(X, Y)])
  rows, cells, cdf = pcr.sampler_ref(fq, fm, pcr.SAMPLER_SCALE, clip, u)
  near = pcr.edge_distance(cdf, rows, cells, u[..., 1]) <= pcr.BRACKET
  print(f'[sampler] {X}x{Y} clip={clip}: {int(near.sum())} of {near.size} uniforms within 1e-5 of a CDF edge')
  assert near.mean() < 0.01                           # half the GPU test's cap of 2 %
  assert pcr.bracketed(cdf, rows, cells, u[..., 1]).all()
  # the samples spread over the lanes' chunk ranges, not one chunk
  NC, cpl = pcr.chunks_per_lane(X, Y)
  assert len(np.unique(cells // 64)) >= min(NC, 12)
  if (X, Y) == (65, 64):                              # the vectorised restatement is the oracle's sampler
    t = torch.from_numpy
    want = oracle_ops.ransac_sample(t(fq), t(fm), None, pcr.SAMPLER_SCALE, clip, u.shape[1], uniforms=t(u)).numpy()
    assert np.array_equal(want[..., 0], rows) and np.array_equal(want[..., 1] * Y + want[..., 2], cells)


@pytest.mark.parametrize('X,Y', pcr.SAMPLER_SHAPES)
def test_one_hot_rows_return_their_target_in_float64(X, Y):
  fq, fm, u, tg = pcr.one_hot_inputs(X, Y)
  NC, cpl = pcr.chunks_per_lane(X, Y)
  assert {0, X * Y - 1} <= set(tg)
  if X * Y > 64 * cpl:
    assert {63, 64, 64 * cpl - 1, 64 * cpl} <= set(tg)
  t = torch.from_numpy
  want = oracle_ops.ransac_sample(t(fq), t(fm), None, pcr.ONE_HOT_SCALE, True, u.shape[1], uniforms=t(u)).numpy()
  assert (want[..., 0] == 0).all()
  assert np.array_equal(want[..., 1] * Y + want[..., 2], np.broadcast_to(tg[:, None], want.shape[:2]))
  assert X * Y * np.exp(-pcr.ONE_HOT_SCALE) < 2.0 ** -60


def test_row_rule_with_confidence_weights():
  cdf = np.cumsum(np.array([[0.0, 0.25, 0.0, 0.5, 0.25, 0.0]], np.float32), -1)
  u1 = np.array([[0.0, 0.2499, 0.25, 0.74, 0.75, 1 - 2.0 ** -24]], np.float32)
  assert pcr.rows_from_cdf_f32(cdf, u1).tolist() == [[1, 1, 3, 3, 4, 4]]


# -- D. pose_score -------------------------------------------------------------------------------------
def test_pose_score_shapes_reach_every_body():
  bodies = set()
  for X, Y, mask, body in pcr.POSE_SCORE_SHAPES:
    got, RB, NB, seams = pcr.pose_score_body(X, Y, mask)
    assert got == body, (X, Y, mask, got)
    bodies.add(body)
    assert (len(seams) > 0) == (body in ('plain_banded', 'band_db'))
  assert bodies == {'plain', 'plain_banded', 'db128', 'db', 'band_db'}
  assert pcr.pose_score_body(70, 1023, False)[1:] == (24, 3, [23, 46, 69])     # 69 = X - 1: the min(.., NB - 1) row
  assert pcr.pose_score_body(23, 2044, True)[1:] == (12, 2, [11, 22])
  assert pcr.pose_score_body(23, 2044, False)[1:] == (7, 4, [7, 14, 21])
  assert pcr.window_supported(*pcr.WINDOW_SHAPE)
  assert pcr.pose_score_body(*pcr.WINDOW_SHAPE[:2], False)[0] == 'db'
  # the shapes of test_pose_score, for the record
  assert [pcr.pose_score_body(X, Y, False)[0] for X, Y in ((32, 32), (25, 37), (192, 160), (131, 260))] == \
      ['db', 'plain', 'band_db', 'band_db']


@pytest.mark.parametrize('X,Y,mask,body', pcr.POSE_SCORE_SHAPES)
def test_planted_geometry_is_exact_and_lands_where_stated(X, Y, mask, body):
  _, RB, NB, seams = pcr.pose_score_body(X, Y, mask)
  poses = pcr.planted_poses(X, Y)
  rng = np.random.default_rng(3)
  sim = rng.random((len(pcr.PLANT_Q), X, Y))
  val, inb, (i0, i1, j0, j1), u, v = pcr.score_terms64(sim, poses, pcr.PLANT_Q, pcr.CELL)
  # exact coordinates: multiples of 2^-6 cell, representable in f32 with room to spare
  assert np.array_equal(u * 64, np.round(u * 64)) and np.array_equal(v * 64, np.round(v * 64))
  u0, r0 = u[:, 0], i0[:, 0]
  for tgt in (0.0, 0.25, X - 0.25, X - 2.0 ** -6, float(X), -0.25, -3.5):
    assert (u0 == tgt).any(), tgt
  assert inb[u0 == X - 2.0 ** -6, 0].any() and not inb[u0 == X, 0].any() and not inb[u0 < 0, 0].any()
  assert set(range(X)) <= set(r0.tolist())                       # every row, so every seam and its neighbours
  for s in seams:
    for k in (s - 1, s, s + 1):
      if k <= X - 1:
        assert ((r0 == k) & (u0 == k + 0.5)).any() and ((r0 == k) & (u0 == k + 0.75)).any() or k == X - 1
  strip = (u0 == 0.25) | (u0 == X - 0.25)
  assert (i0[strip, 0] == i1[strip, 0]).all() and strip.any()
  # the float64 restatement is the oracle's scoring
  vq = np.ones(len(pcr.PLANT_Q), bool)
  mv = pcr.planted_map_valid(X, Y, seams)
  (pu, pv), taps = pcr.tap_probe(X, Y, seams)
  probe = np.nonzero((u[:, 0] == pu) & (v[:, 0] == pv))[0]
  assert len(probe) == 1
  assert [(i0[probe[0], 0], j0[probe[0], 0]), (i0[probe[0], 0], j1[probe[0], 0]),
          (i1[probe[0], 0], j0[probe[0], 0]), (i1[probe[0], 0], j1[probe[0], 0])] == taps
  t = torch.from_numpy
  old = oracle_ops.DTYPE
  oracle_ops.DTYPE = np.float64
  try:
    for k in range(4 if mask else 1):
      want, ok = pcr.scores64(sim, poses, pcr.PLANT_Q, vq, mv[k], pcr.CELL, mask)
      ref = o_pose.pose_scoring_many(
          oracle_ops.o_geo.Transform2D(poses[:, 0].astype(np.float64), poses[:, 1:].astype(np.float64)), sim,
          pcr.PLANT_Q.astype(np.float64), vq, mv[k], oracle_ops.o_grids.Grid2D((X, Y), pcr.CELL), mask)
      assert np.abs(ref - want).max() < 1e-12
      if mask:
        assert not ok[probe[0], 0]                                 # the planted cell under tap k removes the point
        assert pcr.scores64(sim, poses, pcr.PLANT_Q, vq, np.ones((X, Y), bool), pcr.CELL, True)[1][probe[0], 0]
  finally:
    oracle_ops.DTYPE = old
  assert t is not None


def test_border_flip_rule_accepts_flips_and_rejects_the_rest():
  X, Y = 9, 7
  sim, poses, q_xy, vq, mv, cell = pcr.rotated_case(X, Y, 5, B=1, Nq=6, P=40)
  sim, poses, q_xy, vq, mv = sim[0], poses[0].astype(np.float64), q_xy[0], np.ones(6, bool), np.ones((X, Y), bool)
  # pose 3 puts point 2 a hair inside u = 0
  c, s = np.cos(poses[3, 0]), np.sin(poses[3, 0])
  poses[3, 1] = 2e-5 * cell - (c * q_xy[2, 0] - s * q_xy[2, 1])
  want, ok = pcr.scores64(sim, poses, q_xy, vq, mv, cell, True)
  val = pcr.score_terms64(sim, poses, q_xy, cell)[0]
  assert ok[3, 2]
  flipped = want.copy()
  flipped[3] -= val[3, 2]
  assert pcr.explain_by_border_flips(want, sim, poses, q_xy, vq, mv, cell, 2e-4, 1e-5)[0] == 0
  assert pcr.explain_by_border_flips(flipped, sim, poses, q_xy, vq, mv, cell, 2e-4, 1e-5)[0] == 1
  wrong = want.copy()
  wrong[3] += 0.01
  with pytest.raises(AssertionError):
    pcr.explain_by_border_flips(wrong, sim, poses, q_xy, vq, mv, cell, 2e-4, 1e-5)
  wrong = want.copy()
  wrong[5] += 0.01
  with pytest.raises(AssertionError):
    pcr.explain_by_border_flips(wrong, sim, poses, q_xy, vq, mv, cell, 2e-4, 1e-5)


# -- E. masked_softmax_rows ----------------------------------------------------------------------------
@pytest.mark.parametrize('N', pcr.SOFTMAX_N)
def test_softmax_cases_are_what_their_names_say(N):
  x, m = pcr.softmax_case(N)
  seg = (N + 255) // 256
  assert m[0].any() and m[1].sum() == 1 and m[1, -1] and not m[3].any()
  first = int(np.nonzero(m[2])[0][0])
  assert first % seg == 0 and first // seg == (N - 1) // seg and m[2, first:].all()    # one thread's segment
  if N >= 2:
    assert np.isneginf(x[4, 0]) and m[4, 0] and np.isfinite(x[4][m[4]]).any()
  assert {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 511: 2, 513: 3}[N] == seg
  w, cdf = pcr.softmax_want(x, m)
  assert np.isfinite(w).all() and np.abs(cdf[:, -1] - 1).max() < 1e-12
  assert (w[:3][~m[:3]] == 0).all() and (w[3] > 0).all()
  if N >= 2:
    assert w[4, 0] == 0
