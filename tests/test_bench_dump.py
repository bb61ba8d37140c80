"""bench.py --dump-outputs / --full (CPU only): the dump keeps small images whole and larger ones
as the same seeded sample in every run, in float32 / float64 within the size limit; --full is
what turns the CPU baseline on, and --steps / --dump-outputs are validated before any GPU call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_small_image_dumped_whole(tmp_path):
    img = (np.arange(3 * 5 * 7, dtype=np.uint32) * 997 % 65536).astype(np.uint16).reshape(3, 5, 7)
    img[0, 0, 0] = 65535
    bench.dump_outputs(str(tmp_path / "d"), img, rejected=np.array([[3, 4]], dtype=np.uint64), shiftx=np.array([-2, 5]))
    got = {n: np.load(tmp_path / "d" / n) for n in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["rejected.npy", "shiftx.npy", "stack.npy"]
    assert got["stack.npy"].dtype == np.float32 and np.array_equal(got["stack.npy"], img.reshape(-1))
    assert got["rejected.npy"].dtype == np.float64 and got["rejected.npy"].tolist() == [[3.0, 4.0]]
    assert got["shiftx.npy"].dtype == np.float64 and got["shiftx.npy"].tolist() == [-2.0, 5.0]


def test_large_image_sampled_the_same_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    n = 4001
    img = np.arange(n, dtype=np.uint16)          # value = flat index: the sample shows its indices
    bench.dump_outputs(str(tmp_path / "a"), img)
    bench.dump_outputs(str(tmp_path / "b"), img.copy())
    a, b = np.load(tmp_path / "a" / "stack.npy"), np.load(tmp_path / "b" / "stack.npy")
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < n      # distinct indices, ascending
    # a changed element inside the sample shows in the dump
    img2 = img.copy()
    img2[int(a[500])] += 1
    bench.dump_outputs(str(tmp_path / "c"), img2)
    assert np.flatnonzero(np.load(tmp_path / "c" / "stack.npy") != a).tolist() == [500]


def test_default_sample_within_the_size_limit():
    assert bench.DUMP_SAMPLE * 4 <= 48 * 10**6      # float32 sample + the small arrays stay below 64 MB


def test_full_turns_the_cpu_baseline_on(monkeypatch):
    assert not _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1").cpu_baseline
    assert not _parse(monkeypatch, "--no-cpu-baseline").cpu_baseline
    a = _parse(monkeypatch, "--full", "--steps", "3")
    assert a.full and a.cpu_baseline and a.steps == 3
    assert not _parse(monkeypatch, "--full", "--no-cpu-baseline").cpu_baseline


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1"), ("--gpus", "2", "--dump-outputs", "x")])
def test_bad_arguments_refused(monkeypatch, capsys, argv):
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, *argv)
    assert e.value.code == 2
