"""analysis::seq on the MI355X: edit_distance (src/analysis/seq.rs:105-130), hamming_distance
(:74-83) and transition_transversion_ratio (:152-174).

The unit-cost Levenshtein recurrence is the linear-gap global DP with byte equality scored
0 / -1 and open = extend = -1, so edit_distance = -score of that alignment.  It runs on the
aligner's GPU kernels (score only, no traceback) through bg_edit_distance_batch; there is no CPU
path.  Raises NativeUnavailable without the library or a GPU.

hamming_distance and transition_transversion_ratio count unequal bytes (and, among them, the
transitions C<->T and A<->G) of two equal-length sequences with bg_hamming_batch's kernel; the
GPU returns integers and the ratio is finished here in float64, as the reference computes it.
"""
from .. import _device, error
from ..ds.sequence import Sequence


def _bytes(s):
    return bytes(s.chain) if isinstance(s, Sequence) else bytes(s)


def edit_distance(seq1, seq2):
    """Ok(usize) of the reference: the minimum number of substitutions, insertions and
    deletions turning seq1 into seq2 (raw bytes, no case folding)."""
    return _device.handle().edit_distance_batch([(_bytes(seq1), _bytes(seq2))])[0]


def edit_distance_batch(pairs):
    """edit_distance over many pairs in one GPU batch."""
    return _device.handle().edit_distance_batch([(_bytes(a), _bytes(b)) for a, b in pairs])


def _counts(pairs, transitions):
    mis, ts, status = _device.handle().hamming_batch(
        [(_bytes(a), _bytes(b)) for a, b in pairs], transitions=transitions)
    if any(status):
        # Err(BioError::InvalidInputSize): seq1.len() != seq2.len() (seq.rs:81, 153-155)
        raise error.InvalidInputSize("Provided inputs have invalid size!")
    return mis, ts


def hamming_distance(seq1, seq2):
    """Ok(usize) of the reference: the number of positions at which the two sequences differ;
    raises error.InvalidInputSize when their lengths differ."""
    return _counts([(seq1, seq2)], False)[0][0]


def hamming_distance_batch(pairs):
    """hamming_distance over many pairs in one GPU batch."""
    return _counts(pairs, False)[0]


def tstv_ratio(mismatches, transitions):
    """transitions / (mismatches - transitions) with the reference's f64 semantics (seq.rs:173):
    inf when every mismatch is a transition, NaN when there is no mismatch at all."""
    t, v = float(transitions), float(mismatches) - float(transitions)
    if v == 0.0:
        return float("nan") if t == 0.0 else float("inf")
    return t / v


def transition_transversion_ratio(seq1, seq2):
    """Ok(f64) of the reference; raises error.InvalidInputSize when the lengths differ."""
    mis, ts = _counts([(seq1, seq2)], True)
    return tstv_ratio(mis[0], ts[0])


def transition_transversion_ratio_batch(pairs):
    """transition_transversion_ratio over many pairs in one GPU batch."""
    mis, ts = _counts(pairs, True)
    return [tstv_ratio(h, t) for h, t in zip(mis, ts)]
