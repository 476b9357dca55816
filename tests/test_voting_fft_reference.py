"""The frequency-domain voting's reference, checked on itself (no GPU): tests/voting_fft_reference.py against its own
sliding-window form and ``oracle/voting.py``; the stage model a permutation of ``np.fft.fft`` at EVERY transform size;
every planted case what its name says; the threshold enumeration; ``MARGIN`` measured from the f32 model against
float64 on every GPU input; and mutants of the reference that the comparison functions of
tests/test_gpu_voting_fft.py must reject.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import voting_fft_reference as V
import test_gpu_voting_fft as G
from oracle import grids as o_grids
from oracle import voting as o_voting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [dict(name='s0', R=3, H=5, W=7, Hm=5, Wm=7, D=3), dict(name='s1', R=4, H=3, W=9, Hm=6, Wm=4, D=6),
         dict(name='s2', R=2, H=8, W=2, Hm=6, Wm=8, D=2)]


def test_fft64_equals_the_direct_form_and_the_oracle():
  for g in SMALL:
    for kind in ('noise', 'offset'):
      q, tv, m, mv = V.build(dict(g, which='min'), kind)
      assert (V.counts64(tv, mv) == V.counts_direct(tv, mv)).all()
      for overlap in (0.05, None):
        a = V.direct64(q, tv, m, mv, overlap)
        b = V.template_matching_fft64(q, tv, m, mv, overlap)
        c = V.scores64(q, tv, m, mv, overlap)
        d = o_voting.template_matching(q, tv, m, mv, min_overlap=overlap)
        fin = np.isfinite(a)
        assert fin.any() and all((np.isfinite(x) == fin).all() for x in (b, c, d))
        scale = np.abs(a[fin]).max()
        assert np.abs(b[fin] - a[fin]).max() < 1e-12 * scale and np.abs(c[fin] - a[fin]).max() < 1e-12 * scale
        assert np.abs(d[fin] - a[fin]).max() < 2e-6 * scale                   # (the oracle sums in f32)
    H, W, Hm, Wm = g['H'], g['W'], g['Hm'], g['Wm']
    ones = V.counts_direct(np.ones((1, H, W), bool), np.ones((Hm, Wm), bool))[0]
    assert (V.counts_all_valid(H, W, Hm, Wm) == ones).all()


def test_stage_model_is_a_permutation_of_the_fft_at_every_size():
  """tools/fft_voting_model.py (float64, index exact) and the f32 model, for every N of ``fft_size``."""
  sys.path.insert(0, os.path.join(ROOT, 'tools'))
  import fft_voting_model as fm
  plans = {192: '3|4,4|4', 384: '3|2|4,4|4', 512: '2|4,4|4,4', 1024: '4,4|4,4|4', 768: '3|4,4|4,4', 12: '3|4'}
  for N in V.SIZES:
    assert V.fft_size(N) == fm.fft_size(N) == N and V.fft_size(N - 1) == N and V.radices(N) == fm.radices(N)
    if N in plans:
      assert V.plan_string(N) == plans[N]
    rng = np.random.default_rng(N)
    x = rng.standard_normal((N, 2)) + 1j * rng.standard_normal((N, 2))
    ref = np.fft.fft(x, axis=0)
    X = fm.dif_forward(x, 0)
    perm = [int(np.argmin(np.abs(ref[:, 0] - X[k, 0]))) for k in range(N)]
    assert sorted(perm) == list(range(N))
    np.testing.assert_allclose(X, ref[perm], atol=1e-9)
    np.testing.assert_allclose(fm.dit_inverse(X, 0) / N, x, atol=1e-9)
    z = (x.real.astype(np.float32), x.imag.astype(np.float32))
    Z = V.dif32(z, 0)
    assert Z[0].dtype == np.float32
    tol = 16 * V.EPS * np.log2(N) * np.sqrt(N) * np.abs(x).max()
    assert np.abs((Z[0] + 1j * Z[1]) - ref[perm]).max() < tol               # the same permutation, f32 accuracy
    back = V.dit32(Z, 0)
    assert np.abs((back[0] + 1j * back[1]) / N - x).max() < tol
  assert [V.smallest_map(N) for N in (16, 24, 1024)] == [5, 7, 257]
  assert all(V.fft_size(3 * V.HM_MAX[N] - 2) == N and V.fft_size(3 * V.HM_MAX[N] + 1) > N for N in V.GPU_SIZES)


def test_case_table():
  geos = V.axis_geometries()
  assert len(geos) == 52 and len({g['name'] for g in geos}) == 52
  reached = set()
  for g in geos:
    geo = V.geometry(g['H'], g['W'], g['Hm'], g['Wm'])
    reached.add((geo['N1'], geo['N2']))
    assert geo['Ho'] > 0 and geo['Wo'] > 0
    big, n_in = (g['Hm'], g['H']) if g['axis'] == 1 else (g['Wm'], g['W'])
    if g['which'] == 'max':
      assert big == V.HM_MAX[g['N']] and n_in == big and (g['N'] % 3 or 3 * n_in <= g['N'])   # N = 3 x 2^a: the fused first stage
    else:
      assert big == V.smallest_map(g['N']) and n_in > big                            # a template larger than the map
  assert reached == {(N, 64) for N in V.GPU_SIZES} | {(64, N) for N in V.GPU_SIZES}
  assert any(3 * g['H'] > g['N'] for g in geos if g['which'] == 'min' and g['axis'] == 1 and g['N'] % 3 == 0)


def test_planted_cases_are_what_their_names_say():
  for g in [g for g in V.axis_geometries() if g['N'] in (16, 24, 48)] + [dict(H=5, W=6, Hm=5, Wm=6)]:
    q, m, want, cells = V.planted(g)
    assert (np.count_nonzero(q.reshape(V.PLANT_R, -1), axis=1) == 1).all()
    assert (np.count_nonzero(m.reshape(-1, V.PLANT_D), axis=0)[:V.PLANT_R] == 1).all()
    ones = np.ones(q.shape[:3], bool)
    direct = V.direct64(q, ones, m, None, None) * (g['H'] * g['W'] / V.PLANT_TCOUNT)
    assert np.abs(direct - want).max() < 1e-15 and (np.count_nonzero(direct) == np.count_nonzero(want))
    assert (np.abs(want[want != 0]) == 0.125).all()
    Hm, Wm = g['Hm'], g['Wm']
    for r, (i0, j0), (u, v) in cells:
      n = np.count_nonzero(want[r])
      rep = (Hm if u in (0, Hm - 1) else 1) * (Wm if v in (0, Wm - 1) else 1)   # the edge padding's replicas
      assert n <= rep and (n > 0 or g.get('which') == 'min') and (q[r, i0, j0, r] != 0) and (m[u, v, r] != 0)
      if (i0, j0) == (0, 0) and u != Hm - 1 and v != Wm - 1 and g.get('which') != 'min':
        assert n == rep                                                     # all replicas inside the output (a last-edge run is cut by the template)
    assert {(u in (0, Hm - 1)) + 2 * (v in (0, Wm - 1)) for _, _, (u, v) in cells} == {0, 1, 2, 3}
  g = V.axis_geometries()[-1]                                               # (N = 1024 on axis 2: against fft64)
  q, m, want, _ = V.planted(g)
  got = V.raw64(q, m) / V.PLANT_TCOUNT
  assert np.abs(got - want).max() < 1e-12


def test_threshold_enumeration():
  """The f32 chain min_overlap x (float)H x (float)H against the double product, min_overlap in the list, H = 4..342."""
  found = V.chain_disagreements()
  table = {(mo, H): (chain, exact) for mo, H, chain, exact in found}
  for (mo, H), want in {(0.02, 20): (7.9999995, 8.0), (0.01, 10): (0.99999994, 1.0), (0.07, 30): (62.999996, 63.0),
                        (0.03, 20): (11.999999, 12.0)}.items():
    assert (mo, H) in table and table[(mo, H)][1] == want[1] and np.float32(table[(mo, H)][0]) == np.float32(want[0])
    assert (mo, H) in V.ROTATED_THRESHOLDS
  assert (0.05, 20) not in table and float(V.threshold_f32_chain(0.05, 20, 20)) == 20.0
  assert len(found) == 40, len(found)
  # f32(min_overlap) cannot carry the rule even with the products in double
  assert float(np.float32(0.02)) * 400 < 8.0 == 0.02 * 20 * 20


def _rotated_templates(min_overlap, H):
  fq, vq, fm, vm = V.rotated_inputs(min_overlap, H)
  t, tv = o_voting.sample_query_templates(fq, vq, V.ROTATED_R, o_grids.Grid2D((H, H), V.ROTATED_CELL))
  return t, tv, fm, vm


def test_threshold_cells_are_present():
  """Cells whose count EQUALS the integer threshold, on the inputs of the GPU's rotated-threshold cases (templates
  sampled by the oracle) and of its explicit-threshold cases."""
  on = {}
  for mo, H in V.ROTATED_THRESHOLDS:
    t, tv, fm, vm = _rotated_templates(mo, H)
    counts, thr = V.counts64(tv, vm), V.threshold(mo, H, H)
    assert float(thr) == round(mo * H * H)
    on[(mo, H)] = int((counts == int(thr)).sum())
  print('cells on the threshold:', on)
  assert all(n > 0 for n in on.values())
  assert on == ON_THRESHOLD
  for H, W, Hm, Wm in V.THRESHOLD_GEOMETRIES:
    area = V.counts_all_valid(H, W, Hm, Wm)
    for k in V.threshold_values(H, W):
      assert (area == k).any() and ((area == k + 1).any() or k == H * W)
    assert area.max() == H * W


# cells with count == threshold: counted on the float64 reference, with the oracle's templates
ON_THRESHOLD = {(0.02, 20): 342, (0.01, 10): 194, (0.07, 30): 121, (0.03, 20): 243, (0.05, 20): 170}


def _gpu_inputs():
  """(name, q, tv, m, mv, thr, tcount, float64 scores, bound, finite) of every axis / square / planted GPU input."""
  for g in V.axis_geometries():
    for kind in ('noise', 'offset'):
      c = V.axis_case(g['name'], kind)
      yield g['name'] + ' ' + kind, c['q'], c['tv'], c['m'], c['mv'], c['thr'], c['tcount'], c['raw'], c['bound'], \
          V.finite_rule(c['counts'], c['thr']), c['counts']
    q, m, want, _ = V.planted(g)
    tc = np.full(V.PLANT_R, V.PLANT_TCOUNT)
    yield g['name'] + ' planted', q, None, m, None, None, tc, want, V.bound(q, m, tc), np.ones(want.shape, bool), None


def test_margin_and_argmax_gaps():
  """The f32 model stays within 0.5 x MARGIN x bound of float64 on every GPU input, MARGIN is the smallest power of
  two that does, the model's counts are the integers, and every case has rotations whose float64 argmax is decided
  (top-two gap > 2 x MARGIN x bound): 0 cases skipped."""
  worst, worst_name, undecided = 0.0, '', []
  inputs = list(_gpu_inputs())
  c = V.axis_case('N1024-square', 'offset')
  inputs.append(('342 x 342', c['q'], c['tv'], c['m'], c['mv'], c['thr'], c['tcount'], c['raw'], c['bound'],
                 V.finite_rule(c['counts'], c['thr']), c['counts']))
  for name, q, tv, m, mv, thr, tc, want, b, fin, counts in inputs:
    got, cnt = V.model32(q, tv, m, mv, thr=thr, tcount=tc, parts=True)
    if counts is not None:
      assert (np.rint(cnt) == counts).all(), name
      assert np.abs(cnt - counts).max() < 0.25, name
      assert (np.isfinite(got) == fin).all(), name
    err = np.abs(got.astype(np.float64) - np.where(fin, want, 0.0))
    share = float((np.where(fin, err, 0.0) / b[:, None, None]).max())
    worst, worst_name = (share, name) if share > worst else (worst, worst_name)
    if counts is not None and G.check_argmax(name, got, want, fin, b) == 0:
      undecided.append(name)
  print(f'worst model error / bound = {worst:.4f} ({worst_name})')
  assert worst <= 0.5 * V.MARGIN, worst
  assert worst > 0.25 * V.MARGIN, worst          # ... and half of it would not do
  assert undecided == []


# ------------------------------- mutants ---------------------------------
def _rejects(fn, *a, **k):
  with pytest.raises(AssertionError):
    fn(*a, **k)


def test_comparison_functions_reject_the_mutants():
  rejected = []
  # a case with cells on the threshold: (0.02, 20), threshold 8
  t, tv, fm, vm = _rotated_templates(0.02, 20)
  counts, thr = V.counts64(tv, vm), V.threshold(0.02, 20, 20)
  tc = tv.sum((-1, -2)).astype(np.float64)
  raw, b = V.raw64(t, fm) / tc[:, None, None], V.bound(t, fm, tc)
  good = np.where(V.finite_rule(counts, thr), raw, -np.inf).astype(np.float32)
  G.check_mask('good', good, counts, thr)
  G.check_scores('good', good, raw, b, 'mutants', where=V.finite_rule(counts, thr))
  _rejects(G.check_mask, '>=', np.where(counts >= thr, raw, -np.inf).astype(np.float32), counts, thr)
  rejected.append('>= instead of >')
  chain = V.threshold_f32_chain(0.02, 20, 20)
  _rejects(G.check_mask, 'chain', np.where(counts > chain, raw, -np.inf).astype(np.float32), counts, thr)
  rejected.append('the f32-chain threshold')
  flipped = V.counts64(tv, vm, flip=False)
  _rejects(G.check_mask, 'flip', np.where(V.finite_rule(flipped, thr), raw, -np.inf).astype(np.float32), counts, thr)
  rejected.append('a flipped mask')
  # floor instead of rint, on the f32 model's own un-rounded counts
  _, cnt = V.model32(t, tv, fm, vm, thr=thr, parts=True)
  assert (np.rint(cnt) == counts).all() and (np.floor(cnt) != counts).any()
  _rejects(G.check_mask, 'floor', np.where(np.floor(cnt) > thr, raw, -np.inf).astype(np.float32), counts, thr)
  rejected.append('floor instead of rint')
  # score mutants, on an offset case with an odd pair group (D = 6: three pairs)
  c = V.axis_case('N48-min-axis1', 'offset')
  fin = V.finite_rule(c['counts'], c['thr'])
  ok = np.where(fin, c['raw'], -np.inf).astype(np.float32)
  assert G.check_case('good', ok, c, 'mutants') > 0
  zero = V.raw64(c['q'], c['m'], pad='zero') / c['tcount'][:, None, None]
  _rejects(G.check_case, 'zero', np.where(fin, zero, -np.inf).astype(np.float32), c, 'mutants')
  rejected.append('zero padding instead of edge padding')
  _rejects(G.check_case, 'tcount', np.where(fin, c['raw'] * c['tcount'][:, None, None], -np.inf).astype(np.float32), c, 'mutants')
  rejected.append('a missing / tcount')
  _rejects(G.check_case, 'Ho', ok[:, :-1], c, 'mutants')
  rejected.append('an Ho off by one')
  drop = V.raw64(c['q'][..., :-1], c['m'][..., :-1]) / c['tcount'][:, None, None]
  _rejects(G.check_case, 'drop', np.where(fin, drop, -np.inf).astype(np.float32), c, 'mutants')
  rejected.append('a dropped last channel')
  # argmax: the two best cells swapped
  r = 0
  w = np.where(fin[r], c['raw'][r], -np.inf).reshape(-1)
  i, j = np.argsort(w)[-2:]
  sw = ok.copy().reshape(ok.shape[0], -1); sw[r, i], sw[r, j] = sw[r, j], sw[r, i]
  _rejects(G.check_argmax, 'swap', sw.reshape(ok.shape), c['raw'], fin, c['bound'])
  # planted: a delta one cell off
  g = V.axis_geometries()[4]
  q, m, want, _ = V.planted(g)
  tcp = np.full(V.PLANT_R, V.PLANT_TCOUNT)
  G.check_planted('good', want.astype(np.float32), want, V.bound(q, m, tcp), 'mutants')
  _rejects(G.check_planted, 'shift', np.roll(want, 1, axis=2).astype(np.float32), want, V.bound(q, m, tcp), 'mutants')
  assert len(rejected) == 8          # every mutant of the list is rejected: none recorded as unrejectable
  G.SHARES.pop('mutants', None)


# ------------------------------- the CPU emulation, one more geometry ---------------------------------
def test_emulation_at_a_plan_with_an_unpaired_radix4_after_the_3():
  """The kernel bodies of voting_fft_body.h on the CPU emulation (tests/emu/voting_fft_emu.cpp) at N = 12 = 3|4
  on one axis and 48 = 3|4,4 on the other: the -inf mask against the integer counts, the scores within
  MARGIN x bound of float64; and the rotated entry's threshold (0.01, 10): threshold 1, the f32 chain's 0.99999994."""
  build = os.path.join(ROOT, 'tests', '_build')
  os.makedirs(build, exist_ok=True)
  so = os.path.join(build, 'libvoting_fft_emu.so')
  src = os.path.join(ROOT, 'tests', 'emu', 'voting_fft_emu.cpp')
  hdrs = [os.path.join(ROOT, 'snap_amd', 'csrc', h) for h in ('voting_fft_body.h', 'rotate_sample.h')]
  if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
    subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-pthread',
                    '-I' + os.path.join(ROOT, 'snap_amd', 'csrc'), src, '-o', so], check=True)
  lib = ctypes.CDLL(so)
  lib.emu_voting_fft_workspace_bytes.restype = ctypes.c_size_t
  lib.emu_voting_fft_workspace_bytes.argtypes = [ctypes.c_int] * 6
  lib.emu_voting_fft_f32.restype = ctypes.c_int
  lib.emu_voting_fft_f32.argtypes = ([ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 +
                                     [ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int])
  lib.emu_voting_fft_rotated_f32.restype = ctypes.c_int
  lib.emu_voting_fft_rotated_f32.argtypes = ([ctypes.c_void_p] * 3 + [ctypes.c_float] + [ctypes.c_void_p] * 2 +
                                             [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                                                   ctypes.c_int])

  def workspace(*geo):
    nb = lib.emu_voting_fft_workspace_bytes(*geo)
    assert nb > 0
    ws = np.zeros(nb + 256, np.uint8)
    return ws, ws.ctypes.data + (-ws.ctypes.data) % 256
  g = dict(name='emu', R=3, H=3, W=12, Hm=4, Wm=16, D=6)
  geo = V.geometry(3, 12, 4, 16)
  assert (geo['N1'], geo['N2']) == (12, 48) and V.plan_string(12) == '3|4'
  q, tv, m, mv = V.build(dict(g, which='min'), 'offset')
  tc = tv.sum((-1, -2)).astype(np.float32)
  thr = V.threshold(0.05, 3, 12)
  ws, wp = workspace(3, 3, 12, 6, 4, 16)
  out = np.full((3, geo['Ho'], geo['Wo']), np.nan, np.float32)
  tvb, mvb = tv.astype(np.uint8), mv.astype(np.uint8)
  assert lib.emu_voting_fft_f32(q.ctypes.data, tvb.ctypes.data, m.ctypes.data, mvb.ctypes.data, tc.ctypes.data,
                                3, 3, 12, 6, 4, 16, float(thr), 1, wp, out.ctypes.data, 32) == 0
  fin = G.check_mask('emulation', out, V.counts64(tv, mv), thr)
  G.check_scores('emulation', out, V.raw64(q, m) / tc.astype(np.float64)[:, None, None], V.bound(q, m, tc), 'emu', where=fin)
  # the rotated entry takes the threshold itself
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import grids
  mo, H = 0.01, 10
  fq, vq, fm, vm = V.rotated_inputs(mo, H)
  R, D = V.ROTATED_R, V.ROTATED_D
  t, tv = _rotated_templates(mo, H)[:2]
  tfm = pev._template_transforms(R, grids.Grid2D((H, H), V.ROTATED_CELL), 'cpu')[: R // 4].contiguous().numpy()
  ws, wp = workspace(R, H, H, D, H, H)
  out = np.full((R, 2 * H - 1, 2 * H - 1), np.nan, np.float32)
  vqb, vmb = vq.astype(np.uint8), vm.astype(np.uint8)
  assert lib.emu_voting_fft_rotated_f32(fq.ctypes.data, vqb.ctypes.data, tfm.ctypes.data, V.ROTATED_CELL,
                                        fm.ctypes.data, vmb.ctypes.data, R, H, D, H, H, mo * H * H, wp,
                                        out.ctypes.data, 32) == 0
  counts = V.counts64(tv, vm)
  assert (counts == 1).any()
  G.check_mask('emulated rotated entry', out, counts, V.threshold(mo, H, H))
  # ... where the f32 chain of products (what the entry formed from an f32 min_overlap) lets a count of 1 pass
  chain = float(V.threshold_f32_chain(mo, H, H))
  assert chain < 1.0
  assert lib.emu_voting_fft_rotated_f32(fq.ctypes.data, vqb.ctypes.data, tfm.ctypes.data, V.ROTATED_CELL,
                                        fm.ctypes.data, vmb.ctypes.data, R, H, D, H, H, chain, wp,
                                        out.ctypes.data, 32) == 0
  with pytest.raises(AssertionError):
    G.check_mask('the f32 chain', out, counts, V.threshold(mo, H, H))
  assert int((np.isfinite(out) & (counts == 1)).sum()) == int((counts == 1).sum())
  G.SHARES.pop('emu', None)

