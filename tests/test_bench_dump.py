"""bench.py --dump-outputs on CPU: the files it writes for a stand-in batch
(every frame's length and CRC-32, a fixed seeded sample of bitstreams as
float32), their size bound, and that two runs write the same files."""
import importlib
import os
import zlib

import numpy as np
import pytest


class _Pipe:
    """Stands in for zwebp.Pipeline: n finished bitstreams."""

    def __init__(self, n, size, seed):
        rs = np.random.RandomState(seed)
        self.n = n
        self._out = [rs.randint(0, 256, size + 7 * i, dtype=np.uint8).tobytes() for i in range(n)]

    def output(self, i):
        return self._out[i]


@pytest.fixture()
def bench(monkeypatch):
    if "GPU_MAX_HW_QUEUES" not in os.environ:  # bench.py sets a default at import: undone after the test
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")
    return importlib.import_module("bench")


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files(bench, tmp_path):
    pipes = [(_Pipe(50, 1000, 1), 1), (_Pipe(3, 500, 2), 1)]
    outs = [p.output(i) for p, _ in pipes for i in range(p.n)]
    bench.dump_outputs(np, str(tmp_path / "a"), pipes, 4)
    a = _load(str(tmp_path / "a"))
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["bitstream_bytes.npy"].tolist() == [len(o) for o in outs]
    assert a["bitstream_crc32.npy"].tolist() == [zlib.crc32(o) for o in outs]
    picked = a["sample_frames.npy"].astype(int).tolist()
    assert picked[:4] == [0, 1, 2, 3] and len(set(picked)) == len(picked) == 32
    for i in picked:
        v = a[f"bitstream_{i}.npy"]
        assert v.dtype == np.float32 and v.astype(np.uint8).tobytes() == outs[i]
    assert len(a) == 3 + len(picked)
    # the same batch again: the same files, value for value
    bench.dump_outputs(np, str(tmp_path / "b"), pipes, 4)
    b = _load(str(tmp_path / "b"))
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_outputs_size_bound(bench, tmp_path, monkeypatch):
    """The sample stops at the byte budget; lengths and CRCs still cover every frame."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 2500)
    bench.dump_outputs(np, str(tmp_path), [(_Pipe(10, 1000, 3), 1)], 4, "rank1_")
    a = _load(str(tmp_path))
    assert a["rank1_sample_frames.npy"].tolist() == [0, 1]
    assert len(a["rank1_bitstream_bytes.npy"]) == 10 and len(a) == 5


def test_dump_budget_within_64mb(bench):
    # float32 sample (4 bytes per bitstream byte) + two float64 entries per frame of a
    # 1 Mi-frame batch + npy headers stay under the 64 MB the option promises
    assert 4 * bench.DUMP_SAMPLE_BYTES + 2 * 8 * (1 << 20) + (1 << 20) <= 64 * 10**6
