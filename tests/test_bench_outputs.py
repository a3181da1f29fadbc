"""bench.py's `--dump-outputs` and the plain / `--full` split.

CPU: the writer's formats, caller order and its fixed seeded sample beyond the size cap.
GPU: a plain run of a tiny batch times exactly --steps steps, leaves every leg that needs a run
of its own to `--full`, and dumps what the oracle computes for the same seeded pairs."""
import json
import os
import sys

import numpy as np
import pytest

import bench


def _strings(rng, lens):
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]


def test_dump_formats_and_order(tmp_path):
    rng = np.random.default_rng(3)
    s1, s2 = _strings(rng, [5, 0, 9]), _strings(rng, [5, 0, 9])
    bench.dump_outputs(str(tmp_path / "d"), [0, 4, 0], [7, -3, 2 ** 31 - 1], s1, s2)
    got = {n[:-4]: np.load(tmp_path / "d" / n) for n in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["aligned1", "aligned2", "len", "score", "status"]
    for n in ("status", "score", "len"):
        assert got[n].dtype == np.float64
    assert got["status"].tolist() == [0, 4, 0]
    assert got["score"].tolist() == [7, -3, 2 ** 31 - 1]
    assert got["len"].tolist() == [5, 0, 9]
    for n, s in (("aligned1", s1), ("aligned2", s2)):
        assert got[n].dtype == np.float32
        assert np.array_equal(got[n], np.concatenate(s).astype(np.float32))


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    rng = np.random.default_rng(4)
    s1, s2 = _strings(rng, [300, 77]), _strings(rng, [300, 77])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [0, 0], [1, 2], s1, s2)
    flat = np.concatenate(s1).astype(np.float32)
    a, b = np.load(tmp_path / "a" / "aligned1.npy"), np.load(tmp_path / "b" / "aligned1.npy")
    assert a.shape == (100,) and np.array_equal(a, b)
    keep = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(flat.size, 100, replace=False))
    assert np.array_equal(a, flat[keep])


def test_dump_cap_fits_the_budget():
    # two aligned-string files of float32 plus three per-pair float64 files of the metric batch
    assert 2 * 4 * bench.DUMP_MAX_ELEMS + 3 * 8 * 256 <= 64 * 10 ** 6


def test_steps_below_one_are_refused(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--steps" in capsys.readouterr().err


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, monkeypatch, capsys, oracle):
    npairs, n1, n2 = 6, 300, 280
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                      "--pairs", str(npairs), "--len1", str(n1), "--len2", str(n2),
                                      "--dump-outputs", str(out)])
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["metric"] == bench.METRIC and d["unit"] == "GCUPS" and d["dtype"] == "int32"
    assert d["higher_is_better"] is True and d["all_status_ok"] is True
    cells = npairs * n1 * n2
    # the line rounds both figures (3 and 4 decimals)
    assert d["value"] == pytest.approx(cells / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    for leg in ("steady_state", "affine", "configs", "host_to_host", "cpu_baseline"):
        assert d[leg] is None, leg

    pairs = bench.make_pairs(npairs, n1, n2, bench.SEED)
    status, score, ln = (np.load(out / (n + ".npy")) for n in ("status", "score", "len"))
    a1, a2 = np.load(out / "aligned1.npy"), np.load(out / "aligned2.npy")
    assert status.shape == score.shape == ln.shape == (npairs,)
    want1, want2 = b"", b""
    for p, (s1, s2) in enumerate(pairs):
        st, sc, o1, o2 = oracle.align("semiglobal", s1, s2, "blosum62", -1, -2, exact=True)
        assert st == 0 and status[p] == 0
        assert score[p] == sc and ln[p] == len(o1)
        want1, want2 = want1 + o1, want2 + o2
    assert a1.dtype == np.float32 and a1.tobytes() == np.frombuffer(want1, np.uint8).astype(np.float32).tobytes()
    assert a2.tobytes() == np.frombuffer(want2, np.uint8).astype(np.float32).tobytes()
