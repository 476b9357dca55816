"""The stateless sequence operators: fusing frames with known relative motion, one step of the recursive filter, of its
backward smoother, of its pair statistics, of forward-filter / backward-sample and of the Viterbi recursion, and the
walks of the backward ones over a whole track.  ``tracks`` holds the classes that carry the state between steps."""
import math

import numpy as np
import torch

from snap_amd import ops
from snap_amd.models.pose_exhaustive_voting import exhaustive_indices_to_tfm
from snap_amd.models.votes.lattice import _check_planes, _linear_to_indices, _no_motion, sequence_shift_table
from snap_amd.models.votes.motion import _motion_tables, _still_log_taps, _still_taps, motion_taps


def fuse_votes(volumes, q0_t_q, grid, num_rotations, weights=None):
  """Fuse the vote volumes of N query frames with known relative motion into the anchor frame's volume
  (``ops.vote_fuse`` on ``sequence_shift_table``).  ``volumes``: f32 [N, R, 2H-1, 2W-1] or a list of N volumes;
  ``q0_t_q``: Transform2D [N], corner frames, m_t_qn = m_t_q0 @ q0_t_qn; ``weights``: None or N per-frame factors
  (a sequence of numbers or a tensor) -> (fused [R, 2H-1, 2W-1], count int32 [2] = (finite cells, NaN cells)).  The
  fused score exists only where every frame sees the pose (-inf elsewhere): it is again a vote volume, for
  ``poses_from_votes`` and ``posterior_from_votes``."""
  if not isinstance(volumes, torch.Tensor):
    volumes = torch.stack(list(volumes))
  if volumes.dim() != 4 or volumes.shape[1] != num_rotations:
    raise ValueError(f'fuse_votes: volumes [N, {num_rotations}, Ho, Wo], got {tuple(volumes.shape)}')
  shifts = sequence_shift_table(q0_t_q, grid, num_rotations)
  if shifts.shape[0] != volumes.shape[0]:
    raise ValueError(f'fuse_votes: {volumes.shape[0]} volumes for {shifts.shape[0]} relative poses')
  if weights is not None:
    weights = torch.as_tensor(weights, dtype=torch.float32).to(volumes.device).contiguous()
  return ops.vote_fuse(volumes.contiguous(), shifts.to(volumes.device), weights)


def _forward_tables(state, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, log):
  """What a forward step (``filter_votes``; ``log``: ``viterbi_votes``) runs on -> (state, taps): the still tables for
  the first frame of a track (``state`` None), else ``state`` contiguous and the increment's motion tables, on the
  votes' device."""
  if state is None:
    return None, (_still_log_taps if log else _still_taps)(int(num_rotations), str(votes.device))
  taps = _motion_tables(cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, votes.device, log)
  return state.contiguous(), taps


def _backward_taps(fn, belief, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate):
  """What a backward step (``smooth_votes``, ``pair_statistics``, ``sample_back``) opens with: the check of the
  filtered belief, then the tables of the filter step it undoes, on the belief's device."""
  _check_planes(fn, belief, num_rotations, 'belief')
  return motion_taps(next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate, device=belief.device)


def _track_lists(fn, **sequences):
  """What a walk over a track opens with: the per-frame ``sequences`` (keyword = their name in the message; the
  increments last) as lists of one length N >= 1, else ValueError with the counts.  Entry t of the increments is the
  step into frame t; None = no motion is spelled out (entry 0 is never read: a track starts from a uniform prior)."""
  lists = [list(v) for v in sequences.values()]
  if not lists[0] or any(len(v) != len(lists[0]) for v in lists):
    counts = [f'{len(v)} {name.replace("_", " ")}' for name, v in zip(sequences, lists)]
    raise ValueError(f'{fn}: {", ".join(counts[:-1])} and {counts[-1]}')
  lists[-1] = [inc if inc is not None else _no_motion() for inc in lists[-1]]
  return lists


def filter_votes(belief, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0,
                 uniform_mix=1e-3, truncate=3.0):
  """One step of the recursive pose filter (``ops.vote_filter`` on ``motion_taps``): ``belief`` [R, 2H-1, 2W-1] is the
  log-space belief after the previous frame, or None to start a track (a uniform prior; ``cur_t_prev`` is then
  ignored); ``votes`` the new frame's volume; ``cur_t_prev`` the odometry increment (Transform2D, corner frames,
  m_t_prev = m_t_cur @ cur_t_prev) with standard deviations ``sigma_xy`` (metres) / ``sigma_yaw`` (radians);
  ``temperature`` multiplies the votes; ``uniform_mix`` is the share of a uniform distribution mixed into the
  predicted prior (the track can recover from a pose it had ruled out) -> dict of device tensors: ``belief``
  [R, 2H-1, 2W-1] (normalised log-probabilities, -inf = impossible: a vote volume for ``poses_from_votes`` /
  ``posterior_from_votes`` / ``refine_poses``), ``log_evidence`` (of the frame under the predicted prior),
  ``mass_kept`` (the share of the previous belief that stayed inside the volume), ``count`` int32 [4] and ``stats``
  f32 [4] (the op's raw rows)."""
  _check_planes('filter_votes', votes, num_rotations, 'votes')
  belief, taps = _forward_tables(belief, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate,
                                 log=False)
  out, stats, count = ops.vote_filter(belief, votes.contiguous(), taps, temperature, uniform_mix)
  return dict(belief=out, log_evidence=stats[0], mass_kept=stats[1], count=count, stats=stats)


def smooth_votes(belief, smoothed_next, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                 truncate=3.0):
  """One backward step of the smoother that goes with ``filter_votes`` (``ops.vote_smooth`` on ``motion_taps``):
  ``belief`` [R, 2H-1, 2W-1] is the filter's belief after frame t, ``smoothed_next`` the smoothed belief of frame
  t + 1 (for the last frame of a track: its filtered belief), ``next_t_cur`` the increment the filter was given at
  frame t + 1 (its ``cur_t_prev``) and the noise parameters that step's: ``motion_taps`` is deterministic on the host,
  so the tables are the filter's bit for bit -> dict of device tensors: ``smoothed`` [R, 2H-1, 2W-1] (normalised
  log-probabilities of p(x_t | all frames)), ``log_norm`` (0 up to rounding where beliefs and increment belong
  together), ``mass_kept`` (the filter's, of that step), ``count`` int32 [4] and ``stats`` f32 [4] (the op's raw rows)."""
  taps = _backward_taps('smooth_votes', belief, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate)
  out, stats, count = ops.vote_smooth(belief.contiguous(), smoothed_next.contiguous(), taps, uniform_mix)
  return dict(smoothed=out, log_norm=stats[0], mass_kept=stats[1], count=count, stats=stats)


def smooth_track(beliefs, increments, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3, truncate=3.0,
                 details=False):
  """The backward recursion over a track: ``beliefs`` are the N filtered beliefs (``filter_votes`` in frame order),
  ``increments`` the N increments the filter was given (entry 0 is ignored: a track starts from a uniform prior;
  None = no motion) -> the list of the N smoothed volumes, p(x_t | frames 0 .. N-1); the last is ``beliefs[-1]``
  itself.  With ``details`` the list holds ``smooth_votes``' dicts (None for the last frame)."""
  beliefs, increments = _track_lists('smooth_track', beliefs=beliefs, increments=increments)
  smoothed, steps = [None] * len(beliefs), [None] * len(beliefs)
  smoothed[-1] = beliefs[-1]
  for t in range(len(beliefs) - 2, -1, -1):
    steps[t] = smooth_votes(beliefs[t], smoothed[t + 1], increments[t + 1], grid, num_rotations, sigma_xy, sigma_yaw,
                            uniform_mix, truncate)
    smoothed[t] = steps[t]['smoothed']
  return steps if details else smoothed


def pair_statistics(belief, smoothed_next, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                    truncate=3.0):
  """The tap posteriors of one filter step given all frames (``ops.vote_pairs`` on ``motion_taps``): arguments as
  ``smooth_votes`` -> dict of device tensors: ``hist_k`` float64 [Tk], ``hist_a`` [R, Ta], ``hist_b`` [R, Tb] (the
  posterior mass of the stay branch by tap, per axis; entry t of a row belongs to the offset first + t of that row's
  table), ``stay`` and ``jump`` (they sum to 1: ``jump`` is the share of the step's posterior that went through the
  uniform mix, i.e. the track was lost and re-acquired), ``log_norm`` (0 up to rounding where the arguments belong
  together), ``mass_kept``, ``count`` int32 [4], ``stats`` float64 [4], and ``taps``, the tuple used."""
  taps = _backward_taps('pair_statistics', belief, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate)
  hist_k, hist_a, hist_b, stats, count = ops.vote_pairs(belief.contiguous(), smoothed_next.contiguous(), taps,
                                                        uniform_mix)
  return dict(hist_k=hist_k, hist_a=hist_a, hist_b=hist_b, stay=stats[0], jump=stats[1], log_norm=stats[2],
              mass_kept=stats[3], count=count, stats=stats, taps=taps)


def track_statistics(beliefs, smoothed, increments, grid, num_rotations, sigma_xy, sigma_yaw, uniform_mix=1e-3,
                     truncate=3.0):
  """``pair_statistics`` of every step of a track: ``beliefs`` the N filtered beliefs, ``smoothed`` the N smoothed
  volumes (``smooth_track``), ``increments`` the N increments the filter was given (entry 0 ignored; None = no motion)
  -> the list of the N - 1 dicts, entry t for the step from frame t to frame t + 1."""
  beliefs, smoothed, increments = _track_lists('track_statistics', beliefs=beliefs, smoothed_volumes=smoothed,
                                               increments=increments)
  return [pair_statistics(beliefs[t], smoothed[t + 1], increments[t + 1], grid, num_rotations, sigma_xy, sigma_yaw,
                          uniform_mix, truncate)
          for t in range(len(beliefs) - 1)]


def sample_votes(votes, grid, num_rotations, num, seed, stream=0, temperature=1.0):
  """``num`` poses drawn from the pose distribution of a vote volume or a belief (``ops.vote_sample``): ``votes``
  [R, 2H-1, 2W-1]; ``seed`` (64 bits) and ``stream`` (int32; the frame number, say) key the Philox draws, so the same
  arguments give the same poses; ``temperature`` multiplies the votes -> dict of device tensors: ``linear`` int32
  [num] (the linear lattice index, -1 when no cell has mass), ``indices`` int32 [num, 3] = (r, a, b), ``m_t_q``
  (``exhaustive_indices_to_tfm`` of the indices: Transform2D [num], the cells' centre poses, no sub-cell jitter),
  ``log_prob`` f32 [num] (of the drawn cells), ``count`` int32 [2] and ``stats`` f32 [2] (the op's raw rows)."""
  _check_planes('sample_votes', votes, num_rotations, 'votes')
  linear, log_prob, stats, count = ops.vote_sample(votes.contiguous(), num, seed, stream, temperature)
  indices = _linear_to_indices(linear, votes.shape)
  return dict(linear=linear, indices=indices, m_t_q=exhaustive_indices_to_tfm(indices, grid, num_rotations),
              log_prob=log_prob, count=count, stats=stats)


def sample_back(belief, nxt, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, seed, stream, uniform_mix=1e-3,
                truncate=3.0):
  """One backward step of forward-filter / backward-sample (``ops.vote_sample_back`` on ``motion_taps``): ``belief``
  [R, 2H-1, 2W-1] is the filter's belief after frame t, ``nxt`` int32 [B] the chains' linear indices at frame t + 1,
  ``next_t_cur`` the increment the filter was given at frame t + 1 and the noise parameters that step's (as in
  ``smooth_votes``: the tables are the filter's bit for bit) -> dict of device tensors: ``linear`` int32 [B] (the
  chains' cells at frame t, -1 = none), ``jumped`` int32 [B] (1: the step was the uniform jump, 0: transported, -1: no
  predecessor), ``mass_kept``, ``count`` int32 [3] and ``stats`` f32 [2] (the op's raw rows)."""
  taps = _backward_taps('sample_back', belief, next_t_cur, grid, num_rotations, sigma_xy, sigma_yaw, truncate)
  prev, jumped, stats, count = ops.vote_sample_back(belief.contiguous(), nxt.contiguous(), taps, uniform_mix, seed,
                                                    stream)
  return dict(linear=prev, jumped=jumped, mass_kept=stats[0], count=count, stats=stats)


def sample_tracks(beliefs, increments, grid, num_rotations, sigma_xy, sigma_yaw, num, seed, uniform_mix=1e-3,
                  truncate=3.0):
  """``num`` whole tracks drawn from p(x_0 .. x_{N-1} | all frames) by forward-filter / backward-sample: ``beliefs``
  are the N filtered beliefs (``filter_votes`` in frame order), ``increments`` the N increments the filter was given
  (entry 0 is ignored; None = no motion).  ``sample_votes`` on the last belief with stream N - 1, then ``sample_back``
  down to frame 0 with stream t -> dict of device tensors with ``VoteViterbi.path(end=...)``'s shapes: ``linear`` int32
  [N, num], ``indices`` int32 [N, num, 3] (-1 where a track has no pose), ``m_t_q`` (Transform2D [N * num],
  frame-major) and ``jumps`` bool [N, num] (the step into frame t was the uniform jump; frame 0: False)."""
  beliefs, increments = _track_lists('sample_tracks', beliefs=beliefs, increments=increments)
  N = len(beliefs)
  cur = sample_votes(beliefs[-1], grid, num_rotations, num, seed, N - 1)['linear']
  linear, jumps = [cur], []
  for t in range(N - 2, -1, -1):
    step = sample_back(beliefs[t], cur, increments[t + 1], grid, num_rotations, sigma_xy, sigma_yaw, seed, t,
                       uniform_mix, truncate)
    jumps.append(step['jumped'] == 1)
    cur = step['linear']
    linear.append(cur)
  jumps.append(torch.zeros_like(cur, dtype=torch.bool))
  linear = torch.stack(linear[::-1])
  indices = _linear_to_indices(linear, beliefs[-1].shape)
  return dict(linear=linear, indices=indices,
              m_t_q=exhaustive_indices_to_tfm(indices.reshape(-1, 3), grid, num_rotations),
              jumps=torch.stack(jumps[::-1]))


def _viterbi_log_weights(uniform_mix, n):
  """(log_stay, log_jump) = (float32(log1p(-eps)), float32(log(eps) - log(n))) as Python floats; -inf at eps = 1 / 0."""
  eps = float(uniform_mix)
  if not 0.0 <= eps <= 1.0:
    raise ValueError(f'viterbi_votes: uniform_mix must lie in [0, 1], got {uniform_mix}')
  with np.errstate(divide='ignore'):
    return float(np.float32(np.log1p(-np.float64(eps)))), float(np.float32(np.log(np.float64(eps)) - math.log(n)))


def viterbi_votes(score, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, temperature=1.0,
                  uniform_mix=1e-3, truncate=3.0):
  """One forward step of the most-likely-track recursion (``ops.vote_viterbi`` on ``motion_log_taps``), the max-product
  companion of ``filter_votes`` with the same arguments: ``score`` [R, 2H-1, 2W-1] is the previous step's ``score``
  (the log score of the best path into every pose), or None to start a track (``cur_t_prev`` is then ignored) -> dict
  of device tensors: ``score`` [R, 2H-1, 2W-1] (a vote volume for ``poses_from_votes``), ``back`` int32 [R, 2H-1, 2W-1]
  (the linear index of every pose's best predecessor, -1 = none), ``peak_prev`` (M, the maximum of the previous score,
  which the step subtracted: the sum of these over a track restores the path's total), ``top`` (the largest score),
  ``count`` int32 [6] and ``stats`` f32 [2] (the op's raw rows); and what the step was run with, for
  ``VoteViterbi.path``: ``log_taps`` (the table tuple) and ``log_weights`` = (log_stay, log_jump) as Python floats.
  The transition is max((1 - eps) T, eps / n): log_stay = float32(log1p(-eps)), log_jump = float32(log(eps) - log(n)),
  eps = ``uniform_mix``."""
  _check_planes('viterbi_votes', votes, num_rotations, 'votes')
  log_stay, log_jump = _viterbi_log_weights(uniform_mix, votes.numel())
  score, taps = _forward_tables(score, votes, cur_t_prev, grid, num_rotations, sigma_xy, sigma_yaw, truncate, log=True)
  out, back, stats, count = ops.vote_viterbi(score, votes.contiguous(), taps, temperature, log_stay, log_jump)
  return dict(score=out, back=back, peak_prev=stats[0], top=stats[1], count=count, stats=stats, log_taps=taps,
              log_weights=(log_stay, log_jump))


def _entered_by_jump(cur, prev, best_prev, log_taps, shape, log_stay, log_jump):
  """Whether the step into the cells ``cur`` int32 [B] (their predecessors ``prev`` = back[cur]) was the uniform jump,
  from the step's tables alone, on the device -> bool [B].  A jump has prev == J (``best_prev``, the previous frame's
  best cell).  So has a transported step out of J, which the kernel takes iff log_stay + m2 >= log_jump, and then m2
  is the f32 value of the tap triple that leads from ``cur`` to J (d = 0 there): fl(ltb + fl(lta + ltk)), the largest
  over the rotation taps that reach J's plane.  f32 addition is monotone, so that triple's stay >= log_jump also
  implies that the kernel did not jump: the rule below is the kernel's decision exactly."""
  ltk, lk, lta, ltb, off = log_taps
  R, Ho, Wo = shape
  P = Ho * Wo
  x, j = cur.clamp(min=0).long(), best_prev.clamp(min=0).long()
  r, a, b = x // P, (x % P) // Wo, x % Wo
  kj, aj, bj = j // P, (j % P) // Wo, j % Wo
  ta, tb = aj - a - off[r, 0].long(), bj - b - off[r, 1].long()
  inside = (ta >= 0) & (ta < lta.shape[1]) & (tb >= 0) & (tb < ltb.shape[1])
  planes = torch.remainder(r[:, None] + lk + torch.arange(ltk.shape[0], device=cur.device)[None], R)
  m0 = torch.where(planes == kj, ltk[None], ltk.new_full((), -math.inf)).max(-1).values
  m2 = ltb[r, tb.clamp(0, ltb.shape[1] - 1)] + (lta[r, ta.clamp(0, lta.shape[1] - 1)] + m0)
  transported = inside & (m2.new_tensor(log_stay) + m2 >= log_jump)
  return (cur >= 0) & (best_prev >= 0) & (prev == best_prev) & ~transported
