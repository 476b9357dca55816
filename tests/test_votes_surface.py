"""The public surface of ``pose_exhaustive_voting`` after the vote-volume host layer moved to ``snap_amd.models.votes``:
every name the module defined before the split is still an attribute of it, and a moved one is the package's own
object, not a wrapper."""
import importlib
import inspect

from snap_amd.models import pose_exhaustive_voting as pev

# Every name pose_exhaustive_voting.py defined before the split (dir() of the module at that commit, filtered to the
# names it defined itself), by the module that holds it now.
SURFACE = {
    'pose_exhaustive_voting': (
        'FFT_MIN_CELLS FFT_WORKSPACE_BUDGET STACK_MIN_CELLS STACK_SHIFT VOTING_METHOD _correlate '
        '_index_to_tfm_constants _match _overlap_count _stacked _template_transforms _use_fft exhaustive_index_to_tfm '
        'exhaustive_indices_to_tfm exhaustive_pose_voting exhaustive_tfm_to_index get_grid_center_transform '
        'sample_query_templates template_matching'),
    'votes.lattice': (
        '_check_planes _gt_index _host_f64 _host_transform_f64 _linear_to_indices _no_motion _shift_table_f64 '
        '_wrap_angle sequence_shift_table'),
    'votes.analysis': (
        'RECALL_THRESHOLDS _chi2_3_cdf _mode_pose_and_jacobian _modes_of_peaks chi2_3_quantile coverage_table '
        'credible_from_votes modes_from_votes nees_table poses_from_votes posterior_from_votes recall_from_votes '
        'recall_table recall_thresholds'),
    'votes.refine': '_bin_cos_sin _refine_constants _refine_lattice_f64 refine_lattice refine_poses',
    'votes.motion': (
        'FILTER_MAX_TAPS_K FILTER_MAX_TAPS_XY FILTER_MIN_TAP _axis_taps _motion_axes _motion_tables _still_log_taps '
        '_still_tables _still_taps motion_log_taps motion_taps'),
    'votes.sequence': (
        '_entered_by_jump _viterbi_log_weights filter_votes fuse_votes pair_statistics sample_back sample_tracks '
        'sample_votes smooth_track smooth_votes track_statistics viterbi_votes'),
    'votes.noise': (
        'NOISE_CANDIDATES NOISE_MIN_SIGMA_INDEX NOISE_UNIFORM_MIX_RANGE _expected_log_taps _noise_candidates '
        'fit_motion_noise motion_noise_objective noise_m_step'),
    'votes.odometry': 'ODOMETRY_MAX_S _increment_shifts estimate_increments increment_from_votes increment_lattice',
    'votes.frames': (
        'PRIOR_MAX_COMPONENTS PRIOR_MAX_QUADRATIC PosePrior _prior_rows pose_prior prior_votes rebase_table '
        'rebase_votes'),
    'votes.temper': (
        'TemperatureFit _hermite_root _ladder_f32 fit_temperature solve_temperature temper_votes temperature_ladder'),
    'votes.tracks': 'VoteFilter VoteViterbi viterbi_track',
    'votes.localize': 'localize_exhaustive localize_sequence',
}
SWITCHES = ('STACK_SHIFT', 'STACK_MIN_CELLS', 'VOTING_METHOD', 'FFT_MIN_CELLS', 'FFT_WORKSPACE_BUDGET')


def test_every_name_is_still_an_attribute_and_moved_ones_are_the_packages_own():
  assert sum(len(names.split()) for names in SURFACE.values()) == 103
  for where, names in SURFACE.items():
    module = importlib.import_module('snap_amd.models.' + where)
    for name in names.split():
      obj = getattr(pev, name)
      assert obj is getattr(module, name), name
      if inspect.isfunction(obj) or inspect.isclass(obj):
        assert obj.__module__ == module.__name__, name     # defined there: the same object, not a wrapper


def test_patched_switches_are_defined_in_the_voting_module_itself():
  packaged = [importlib.import_module('snap_amd.models.' + where) for where in SURFACE if where.startswith('votes.')]
  for name in SWITCHES:
    assert name in vars(pev), name
    assert not any(hasattr(module, name) for module in packaged), name
  # read at call time: a patched switch changes the next call
  keep = pev.STACK_SHIFT
  try:
    pev.STACK_SHIFT = 1
    assert not pev._stacked(36, (128, 128))
  finally:
    pev.STACK_SHIFT = keep
  assert pev._stacked(36, (128, 128))
