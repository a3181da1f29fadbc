"""Host side of the distance family (no GPU): bg_hamming_batch / bg_mismatch_matrix are declared,
exported and bound; a NULL handle is an argument error; the two pure finishing functions
(analysis.seq.tstv_ratio, analysis.stat.p_distance) have the reference's float semantics
(seq.rs:173 in f64, stat.rs:147 in f32)."""
import math
import os
import re

import numpy as np

from conftest import ROOT

NAMES = ("bg_hamming_batch", "bg_mismatch_matrix")


def test_symbols_declared_exported_and_bound():
    from biogarden_amd import _native
    with open(os.path.join(ROOT, "include", "biogarden_gpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = _native.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in _native.EXPORTS, name
    assert L.bg_abi_version() == 2


def test_null_handle_is_an_argument_error():
    from biogarden_amd import _native
    L = _native.lib()
    assert L.bg_hamming_batch(None, 0, None, None, None, None, None, None, None) == -1
    assert L.bg_mismatch_matrix(None, 0, None, None, 0, None, None, None) == -1


def test_tstv_ratio():
    from biogarden_amd.analysis.seq import tstv_ratio
    assert tstv_ratio(282, 189) == 2.032258064516129        # integration.rs:76-80
    assert tstv_ratio(23, 15) == 1.875                       # seq.rs:148-150
    assert tstv_ratio(5, 0) == 0.0
    for h in (1, 7, 1 << 40):
        assert tstv_ratio(h, h) == math.inf                  # t / 0.0, t > 0
    assert math.isnan(tstv_ratio(0, 0))                      # 0.0 / 0.0


def test_p_distance_bit_patterns():
    from biogarden_amd.analysis.stat import p_distance
    for L in (1, 3, 7, 1000, 10000, (1 << 24) + 1, (1 << 30) - 1, 0):
        cs = [c for c in (0, 1, 2, 3, 999, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 30) - 1)
              if c <= L] or [0]
        counts = np.array([cs, cs[::-1]], dtype=np.uint32)
        got = p_distance(counts, L)
        assert got.dtype == np.float32 and got.shape == counts.shape
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.array([[np.float32(c) / np.float32(L) for c in row] for row in counts.tolist()],
                            dtype=np.float32)
        assert (got.view(np.uint32) == want.view(np.uint32)).all() or L == 0, L
        if L == 0:
            assert np.isnan(got).all()                       # the diagonal included (stat.rs:147)
