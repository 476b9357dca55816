"""The vote-volume toolkit: inference over the [R, 2H-1, 2W-1] volumes of ``exhaustive_pose_voting``.  Host code only;
every operator's kernel is a wrapper of ``snap_amd.ops``.  None of this has a counterpart in the reference.

* ``lattice``: the index lattice's shared pieces (plane checks, ground-truth index, linear -> (r, a, b), shift table);
* ``analysis``: one volume -> peaks, posterior, credible regions, modes, expected recall, and their evaluation tables;
* ``refine``: peaks -> continuous poses on the two planes;
* ``motion``: an odometry increment -> the tap tables of the sequence kernels;
* ``sequence``: the stateless sequence operators (fuse, filter, smooth, pair statistics, sample, Viterbi step);
* ``noise``: EM fit of the motion noise;  ``odometry``: the increment between two frames from their votes;
* ``frames``: a change of map frame, and position / heading priors;  ``temper``: temperature ladders and calibration;
* ``raster``: road / lane raster priors on the map grid, their strength ladder and its calibration;
* ``tracks``: ``VoteFilter`` and ``VoteViterbi``, the stateful tracks over all of the above;
* ``localize``: ``localize_exhaustive`` / ``localize_sequence``, voting followed by the analysis.

``snap_amd.models.pose_exhaustive_voting`` re-exports every name of these modules and is what callers import.  The
modules need its voting and index <-> transform functions, and it imports them at its bottom: it is imported first
here, so that either entry point finds the other complete."""
from snap_amd.models import pose_exhaustive_voting  # noqa: F401
