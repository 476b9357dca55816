"""CPU pins of the sampling contract (snap_vote_sample_f32 / snap_vote_sample_back_f32, include/snap_hip.h): the numpy
restatement ``vote_sample_reference`` against published Philox vectors, against the smoother's independent dense
formulation (the forward-filter / backward-sample identity), and the seeded statistical test of the GPU suite run on
the reference sampler alone, which is where its seed and bound come from."""
import functools

import numpy as np

import vote_filter_reference as flt
import vote_sample_reference as ref
import vote_smooth_reference as smo

# The seeded statistical test (here and in test_gpu_vote_sample.py): 65536 tracks, this seed.  Z_REFERENCE is the
# largest |z| the REFERENCE sampler reaches (frame 0 against the smoothed marginal, the last frame against the belief);
# the GPU test allows Z_REFERENCE + 1.  test_seeded_statistics_of_the_reference_sampler pins both numbers.
STAT_TRACKS = 65536
STAT_SEED = 0x5EED0BADC0FFEE
Z_REFERENCE = 3.64


def test_philox_known_answers():
  """The vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)."""
  h = lambda s: np.array([int(w, 16) for w in s.split()], np.uint64)
  for counter, key, want in (
      ('0 0 0 0', '0 0', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
      ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
      ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1')):
    got = ref.philox4x32_10(h(counter), h(key))
    assert [f'{int(w):08x}' for w in got] == want.split(), (counter, key)


def test_uniforms_are_the_53_bit_construction():
  u = ref.uniforms(1000, 0x0123456789ABCDEF, -3, 1)
  assert u.shape == (1000, 2) and (u >= 0).all() and (u < 1).all()
  counter = np.array([[7, (-3) & 0xFFFFFFFF, 1, 0]], np.uint64)
  x = [int(w) for w in ref.philox4x32_10(counter, np.array([0x89ABCDEF, 0x01234567], np.uint64))[0]]
  assert u[7, 0] == (((x[0] >> 5) << 26) + (x[1] >> 6)) / 2.0 ** 53
  assert u[7, 1] == (((x[2] >> 5) << 26) + (x[3] >> 6)) / 2.0 ** 53
  assert (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53)).all()
  assert not (ref.uniforms(8, 1, 0, 0) == ref.uniforms(8, 1, 1, 0)).any()     # streams differ
  assert not (ref.uniforms(8, 1, 0, 0) == ref.uniforms(8, 1, 0, 1)).any()     # purposes differ
  assert 0.45 < u.mean() < 0.55


def test_dense_draw_is_the_inverse_cdf():
  for c in ref.sample_inputs():
    if c['votes'].size > 50000:
      continue
    m = ref.model(c['votes'], c['scale'])
    rng = np.random.default_rng(1)
    u = ref.given_uniforms(m, rng)
    idx = ref.draw(m, u)
    if not m['Z'] > 0:
      assert (idx == -1).all()
      continue
    assert (m['p'][idx] > 0).all(), c['name']
    assert ref.member(m, idx, u, 0.0).all(), c['name']
    # the strict "exceeds": u = C(c) / Z exactly belongs to the next cell with mass
    assert idx[0] == np.nonzero(m['p'] > 0)[0][0] and idx[1] == np.nonzero(m['p'] > 0)[0][-1]
    got = ref.vote_sample(c['votes'], 64, 5, 2, c['scale'])
    assert np.allclose(np.exp(got[1]), m['p'][got[0]] / m['Z'], rtol=1e-12), c['name']
    assert got[3].tolist() == [m['mass'], m['bad']]


@functools.lru_cache(maxsize=None)
def _identity_track():
  """[4, 5, 6], three frames, eps = 1e-2: votes, taps, scale, the reference filter's beliefs (rounded to f32, as the
  kernel's are) and the smoother module's dense alpha-beta marginals."""
  rng = np.random.default_rng(11)
  R, Ho, Wo, N, eps, scale = 4, 5, 6, 3, 1e-2, 2.0
  votes = [rng.standard_normal((R, Ho, Wo)).astype(np.float32) for _ in range(N)]
  taps = [None]
  for t in range(1, N):
    off = np.array([[-1, 1], [1, -2], [0, 1], [-2, 0]], np.int32) * (1 if t == 1 else -1)
    taps.append((flt.rand_taps(rng, 1, 3)[0], -1 if t == 1 else 2, flt.rand_taps(rng, R, 2), flt.rand_taps(rng, R, 3),
                 off))
  beliefs = [flt.vote_filter(None, votes[0], smo.still_taps(R), scale, eps)[0].astype(np.float32)]
  for t in range(1, N):
    beliefs.append(flt.vote_filter(beliefs[-1], votes[t], taps[t], scale, eps)[0].astype(np.float32))
  gamma = smo.dense_smoothing(votes, taps, scale, eps, beliefs)
  return votes, taps, eps, beliefs, gamma


def test_backward_conditional_satisfies_the_ffbs_identity():
  """sum_x gamma_{t+1}(x) q(x' | x) == gamma_t(x'), to 1e-9 of the largest entry.  gamma_{t+1} is the smoother
  module's dense alpha-beta marginal; gamma_t is the smoothing recursion on it with the smoother module's DENSE kernel
  (``dense_kernel``: unit masses pushed through the predict step, nothing of the window) and the masses of the f32
  belief the sampler is given -- the belief IS the sampler's alpha_t, so this is the identity the sampler can and must
  satisfy exactly.  Against the alpha-beta gamma_t from the raw votes, whose alpha_t the f32 belief only approximates,
  the deviation is that of the belief's rounding: |belief| 2^-24 per cell, relative, < 2e-6 of the largest entry."""
  votes, taps, eps, beliefs, gamma = _identity_track()
  n = votes[0].size
  for t in (1, 0):
    bm = ref.back_model(beliefs[t], taps[t + 1], eps)
    q = np.stack([ref.conditional(bm, x) for x in range(n)])          # [x, x']
    assert np.allclose(q.sum(1), 1.0, atol=1e-12)
    got = gamma[t + 1] @ q
    alpha = bm['p'] / bm['sum_p']
    K = smo.dense_kernel(beliefs[t], taps[t + 1], eps)                # [x, x']
    want = alpha * (K.T @ (gamma[t + 1] / (K @ alpha)))
    dev, dev_ab = np.abs(got - want).max() / want.max(), np.abs(got - gamma[t]).max() / gamma[t].max()
    print(f'frame {t}: deviation {dev:.3g} of the largest entry; from the raw-vote alpha-beta {dev_ab:.3g}')
    assert dev <= 1e-9
    assert dev_ab <= 2e-6


def test_reference_back_step_edges():
  f = {c['name']: c for c in ref.back_inputs()}
  rng = np.random.default_rng(3)
  for name, c in f.items():
    if c['belief'].size > 50000:
      continue
    bm = ref.back_model(c['belief'], c['taps'], c['eps'])
    nxt = ref.back_chains(bm, rng, 12)
    uni = rng.random((len(nxt), 2))
    prev, jumped, stats, count = ref.vote_sample_back(c['belief'], nxt, c['taps'], c['eps'], 1, 0, uni)
    assert prev[2] == -1 and prev[3] == -1 and jumped[2] == -1 and jumped[3] == -1
    assert ((prev >= 0) == (jumped >= 0)).all() and (bm['p'][prev[prev >= 0]] > 0).all()
    for x, u, p, j in zip(nxt, uni, prev, jumped):
      assert ref.back_admissible(bm, int(x), u[0], u[1], int(p), int(j), 0.0)[0], name
    if name == 'never_jumps':
      assert (jumped <= 0).all()
    if name == 'always_jumps':
      assert (jumped[[0, 1]] == 1).all() and (jumped[4:] == 1).all()
    assert count.tolist() == [(prev >= 0).sum(), (jumped == 1).sum(), bm['bad']]
  # a chain whose window is empty, eps = 0: rotation 5 of the ragged case reads only rows below the volume
  c = f['never_jumps']
  bm = ref.back_model(c['belief'], c['taps'], c['eps'])
  x = np.ravel_multi_index((5, 10, 10), bm['shape'])
  assert ref.window(bm, x)[2] == 0.0 and ref.back_one(bm, x, 0.3, 0.3) == (-1, -1)


def test_seeded_statistics_of_the_reference_sampler():
  z0, z2, n0, n2 = ref.stat_reference(ref.stat_scene(), STAT_TRACKS, STAT_SEED)
  print(f'max |z|: frame 0 {z0:.3f} over {n0} cells, last frame {z2:.3f} over {n2} cells')
  assert n0 >= 40 and n2 >= 40                      # the test is about most of the 120 cells
  assert max(z0, z2) <= Z_REFERENCE
  # among ~200 nearly independent z the largest is above 2 with probability 1 - 0.954^200: a sampler that merely
  # returned the mode, or one whose counts were too regular, would not be here
  assert max(z0, z2) >= 1.5
