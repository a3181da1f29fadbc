"""The distance family on the GPU: analysis::seq::hamming_distance (src/analysis/seq.rs:74-83),
transition_transversion_ratio (:152-174) and analysis::stat::p_distance_matrix
(src/analysis/stat.rs:138-152) through bg_hamming_batch / bg_mismatch_matrix.

The yardstick is NumPy on the host, independent of the code under test: byte inequality of the
two rows, and the four transition pairs written out.  Counts are integers, so every comparison
is exact; the float results are compared as bit patterns.
"""
import os
import random

import numpy as np
import pytest

from conftest import REF_FIX, read_fasta

pytestmark = pytest.mark.gpu

SEG = 65536            # BG_DIST_SEG (biogarden_amd/csrc/bg_dist.h): bytes of a pair per workgroup
TRANSITIONS = ((ord("C"), ord("T")), (ord("T"), ord("C")), (ord("A"), ord("G")), (ord("G"), ord("A")))


def np_counts(a, b):
    """(mismatches, transitions) of two equal-length byte strings."""
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    ts = np.zeros(len(x), dtype=bool)
    for p, q in TRANSITIONS:
        ts |= (x == p) & (y == q)
    return int((x != y).sum()), int(ts.sum())


def np_matrix(rows_a, rows_b):
    out = np.zeros((len(rows_a), len(rows_b)), dtype=np.uint32)
    for i, a in enumerate(rows_a):
        x = np.frombuffer(a, np.uint8)
        for j, b in enumerate(rows_b):
            n = min(len(a), len(b))
            out[i, j] = (x[:n] != np.frombuffer(b, np.uint8)[:n]).sum()
    return out


def rand_bytes(seed, n, alpha):
    rng = np.random.default_rng(seed)
    return np.frombuffer(bytes(alpha), np.uint8)[rng.integers(0, len(alpha), n)].tobytes()


@pytest.fixture(scope="module")
def handle():
    from biogarden_amd import _native
    h = _native.Handle(0)
    yield h
    h.close()


def test_reference_goldens():
    from biogarden_amd.analysis import seq
    from biogarden_amd.ds.sequence import Sequence
    inp = read_fasta(os.path.join(REF_FIX, "input", "hamming_distance.fasta"))
    a, b = inp[0][1], inp[1][1]
    assert len(a) == len(b) == 952 and sum(x != y for x, y in zip(a, b)) == 477
    assert seq.hamming_distance(Sequence(a), Sequence(b)) == 477                    # integration.rs:63-67
    assert seq.hamming_distance(Sequence("GAGCCTACTAACGGGAT"), Sequence("CATCGTAATGACGGCCT")) == 7
    inp = read_fasta(os.path.join(REF_FIX, "input", "transversions.fasta"))
    a, b = inp[0][1], inp[1][1]
    assert len(a) == len(b) == 838
    assert (sum(x != y for x, y in zip(a, b)), sum((x, y) in TRANSITIONS for x, y in zip(a, b))) == (282, 189)
    assert seq.transition_transversion_ratio(Sequence(a), Sequence(b)) == 2.032258064516129   # :76-80
    a = Sequence("TTAGGGACTGGATTATTTCGTGATCGTTGTAGTTATTGGAAGTACGGGCATCAACCCAGTT")
    b = Sequence("TCAACGGCTGGATAATTTCGCGATCGTGCTGGTTACTGGCGGTACGAGTGTTCCTTTGGGT")
    assert seq.transition_transversion_ratio(a, b) == 1.875                          # seq.rs:148-150
    assert seq.hamming_distance_batch([(a, b), (b, a)]) == [23, 23]
    assert seq.transition_transversion_ratio_batch([(a, b)]) == [1.875]


def test_unequal_lengths_raise():
    from biogarden_amd import error
    from biogarden_amd.analysis import seq
    for fn in (seq.hamming_distance, seq.transition_transversion_ratio):
        with pytest.raises(error.InvalidInputSize):
            fn(b"ACGT", b"ACG")
    with pytest.raises(error.InvalidInputSize):
        seq.hamming_distance_batch([(b"AC", b"AG"), (b"", b"A")])


LENGTHS = [1, 3, 5, 15, 17, 63, 65, 255, 257, 1023, 4097, SEG + 1, 2 * SEG + 17, 0, 4, 16, 64, 256]
ALPHABETS = [b"ACGT", b"acgtU", bytes(range(256))]


def test_pair_batch(handle):
    """Every length class and alphabet in ONE batch, the odd lengths first so that later pairs
    start at odd device offsets; unequal pairs in between get status 2 and zero counts."""
    pairs, want, low = [], [], []
    for k, n in enumerate(LENGTHS):
        for m, alpha in enumerate(ALPHABETS):
            a, b = rand_bytes(1000 + 8 * k + m, n, alpha), rand_bytes(5000 + 8 * k + m, n, alpha)
            if alpha == b"acgtU":
                low.append(len(pairs))
            pairs.append((a, b))
            want.append(np_counts(a, b) + (0,))
        if k % 4 == 1:
            pairs.append((rand_bytes(k, n + 3, b"ACGT"), rand_bytes(k + 1, n, b"ACGT")))
            want.append((0, 0, 2))
    mis, ts, st = handle.hamming_batch(pairs)
    assert list(zip(mis, ts, st)) == want
    # acgtU holds no upper-case A, C, G, T: no transitions, many mismatches
    assert all(ts[i] == 0 for i in low) and sum(mis[i] for i in low) > 0
    # the transition count may be skipped
    mis2, ts2, st2 = handle.hamming_batch(pairs, transitions=False)
    assert (mis2, ts2, st2) == (mis, None, st)
    assert handle.hamming_batch([]) == ([], [], [])


def test_exhaustive_byte_pairs(handle):
    """All 65 536 (a, b) byte combinations once: 65 280 mismatches, exactly 4 transitions."""
    a = np.repeat(np.arange(256, dtype=np.uint8), 256).tobytes()
    b = np.tile(np.arange(256, dtype=np.uint8), 256).tobytes()
    assert handle.hamming_batch([(a, b), (b"x" + a, b"x" + b)]) == ([65280, 65280], [4, 4], [0, 0])


def test_deterministic(handle):
    n = 2 * SEG + 17
    pair = (rand_bytes(77, n, b"ACGT"), rand_bytes(78, n, b"ACGT"))
    first = handle.hamming_batch([pair])
    assert first == handle.hamming_batch([pair])
    assert (first[0][0], first[1][0]) == np_counts(*pair)


@pytest.mark.parametrize("rows,L", [(1, 1), (2, 5), (63, 17), (64, 256), (65, 257), (130, 1000), (3, 0),
                                    (300, 4099)])
def test_matrix_symmetric(handle, rows, L):
    from biogarden_amd.analysis import stat
    from biogarden_amd.ds.tile import Tile
    # a few distinct rows, mutated: distances spread between 0 and L
    base = [rand_bytes(100 + r, L, b"ACGT") for r in range(4)]
    rng = random.Random(rows * 7919 + L)
    data = []
    for r in range(rows):
        row = bytearray(base[r % 4])
        for _ in range(rng.randint(0, max(1, L // 3)) if L else 0):
            row[rng.randrange(L)] = rng.choice(b"ACGT")
        data.append(bytes(row))
    got = handle.mismatch_matrix(data)
    want = np_matrix(data, data)
    assert got.dtype == np.uint32 and got.shape == (rows, rows)
    assert (got == want).all()
    assert (got == got.T).all() and (np.diag(got) == 0).all()
    p = stat.p_distance_matrix(Tile(data))
    assert p.dtype == np.float32 and p.shape == (rows, rows)
    if L == 0:
        assert np.isnan(p).all()
    else:
        ref = want.astype(np.float32) / np.float32(L)
        assert (p.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("na,nb,L", [(65, 130, 300), (1, 200, 33)])
def test_matrix_two_sets(handle, na, nb, L):
    A = [rand_bytes(300 + i, L, b"ACGT") for i in range(na)]
    B = [rand_bytes(900 + j, L, b"ACGT") for j in range(nb)]
    B[nb // 2] = A[0]
    got = handle.mismatch_matrix(A, B)
    assert got.shape == (na, nb) and (got == np_matrix(A, B)).all()
    assert got[0, nb // 2] == 0


def test_matrix_ragged(handle):
    """Rows of different lengths follow the reference's zip: min(len_i, len_j) bytes."""
    from biogarden_amd.analysis import stat
    from biogarden_amd.ds.tile import Tile
    lens = [100, 0, 1, 17, 64, 99, 33]
    data = [rand_bytes(40 + i, n, bytes(range(256))) for i, n in enumerate(lens)]
    got = handle.mismatch_matrix(data)
    want = np_matrix(data, data)
    assert (got == want).all() and (got == got.T).all() and (np.diag(got) == 0).all()
    p = stat.p_distance_matrix(Tile(data))
    ref = want.astype(np.float32) / np.float32(100)
    assert (p.view(np.uint32) == ref.view(np.uint32)).all()
    other = [rand_bytes(60 + j, n, bytes(range(256))) for j, n in enumerate([5, 100, 0, SEG + 3])]
    data[0] = rand_bytes(59, SEG + 9, bytes(range(256)))
    assert (handle.mismatch_matrix(data, other) == np_matrix(data, other)).all()
    assert handle.mismatch_matrix(data, []).shape == (7, 0)
    assert handle.mismatch_matrix([]).shape == (0, 0)


def test_prepared_batch_survives(handle, oracle):
    """The distance calls use buffers of their own: a batch prepared before them still executes
    and fetches the oracle's alignments."""
    import parity_util
    from biogarden_amd import _native
    from biogarden_amd.alignment.aligner import AlignmentResult
    from biogarden_amd.ds.sequence import Sequence
    rng = random.Random(5)
    pairs = []
    for n1, n2 in ((300, 120), (64, 65), (1, 40), (500, 500)):
        s1 = parity_util.rand_seq(rng, n1, parity_util.DNA)
        pairs.append((s1, parity_util.mutate(rng, s1, parity_util.DNA)[:n2] or b"A"))
    handle.prepare("semiglobal", pairs, _native.builtin_scoring(_native.BG_UNIT), -1, -1)
    rows = [rand_bytes(i, 777, b"ACGT") for i in range(70)]
    assert (handle.mismatch_matrix(rows) == np_matrix(rows, rows)).all()
    assert handle.hamming_batch([(rows[0], rows[1])])[0] == [np_counts(rows[0], rows[1])[0]]
    handle.execute()
    res = [AlignmentResult(r["score"], Sequence(r["aligned1"]), Sequence(r["aligned2"]), r["status"],
                           r["end"], r["start"]) for r in handle.fetch()]
    parity_util.check_results(oracle, "semiglobal", pairs, res, "unit", -1, -1)
