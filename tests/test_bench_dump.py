"""bench.py --dump-outputs on the host: the whole frame under the budget, a fixed seeded pixel sample above it."""
import numpy as np

import bench


def test_whole_frame_and_counts(tmp_path):
    f = np.random.default_rng(1).random((108, 192, 5), dtype=np.float32)
    bench.dump_outputs(str(tmp_path), f, [7, 8, 9, 0, 2])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["counts.npy", "frame.npy"]
    assert np.array_equal(np.load(tmp_path / "frame.npy"), f)
    c = np.load(tmp_path / "counts.npy")
    assert c.dtype == np.float64 and c.tolist() == [7, 8, 9, 0, 2]


def test_large_frame_is_sampled_within_the_budget(tmp_path):
    f = np.arange(2160 * 3840 * 5, dtype=np.float32).reshape(2160, 3840, 5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), f, [1, 2, 3, 4, 5])
        assert sum(p.stat().st_size for p in (tmp_path / d).iterdir()) <= 64_000_000
    s, px = np.load(tmp_path / "a" / "frame_sample.npy"), np.load(tmp_path / "a" / "frame_sample_pixels.npy")
    assert s.dtype == np.float32 and px.dtype == np.float64 and len(np.unique(px)) == len(px) == s.shape[0]
    assert np.array_equal(s, f.reshape(-1, 5)[px.astype(np.int64)])
    assert np.array_equal(px, np.load(tmp_path / "b" / "frame_sample_pixels.npy"))
