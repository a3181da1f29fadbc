"""analysis::stat::p_distance_matrix (src/analysis/stat.rs:138-152) on the MI355X.

The N x N matrix of the fraction of columns at which two rows of a Tile differ.  The GPU counts
the unequal bytes (bg_mismatch_matrix: integers only); the division by the column count is done
here in float32, exactly as the reference's `count as f32 / columns as f32`, which makes the floats
bit-identical.  There is no CPU path: raises NativeUnavailable without the library or a GPU.
"""
import numpy as np

from .. import _device
from ..ds.sequence import Sequence


def p_distance(counts, columns):
    """counts (uint32 array) -> float32 p-distances: float32(count) / float32(columns).
    columns == 0 gives NaN everywhere (0.0 / 0.0, stat.rs:147)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(counts).astype(np.float32) / np.float32(columns)


def p_distance_matrix(tile):
    """Array2<f32> of the reference as a (rows, rows) float32 array.  columns is the first row's
    length (Tile::size); rows of other lengths are compared over the shorter of the two (zip).
    An empty tile raises what Tile.size() raises, where the reference panics."""
    _, columns = tile.size()
    rows = [bytes(s.chain) if isinstance(s, Sequence) else bytes(s) for s in tile]
    return p_distance(_device.handle().mismatch_matrix(rows), columns)
