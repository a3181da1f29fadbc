"""hamming_distance, transition_transversion_ratio and p_distance_matrix through the C++ facade
(include/biogarden.hpp), compiled like test_cpp_facade.py's sources: the reference's goldens and
doctests and a 3 x 3 matrix on the GPU."""
import subprocess

import pytest

from conftest import REF_FIX
from test_cpp_facade import build


def test_dist_source_compiles(tmp_path):
    build("test_dist.cpp", tmp_path / "test_dist")


@pytest.mark.gpu
def test_dist_through_the_facade(tmp_path):
    exe = build("test_dist.cpp", tmp_path / "test_dist")
    r = subprocess.run([exe, REF_FIX], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dist ok" in r.stdout
