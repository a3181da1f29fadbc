"""analysis — the reference's src/analysis module, restricted to what runs on the GPU:
seq::{edit_distance, hamming_distance, transition_transversion_ratio} and
stat::p_distance_matrix."""
from . import seq  # noqa: F401
from . import stat  # noqa: F401
