"""bench.py --dump-outputs without a GPU: what it writes for an output that fits the 64 MB bound, and the fixed sample of rows it
writes for one that does not (the headline frame's RGBA output is 298 MB as float32)."""
import numpy as np
import pytest

import bench


def _total_bytes(d):
    return sum(f.stat().st_size for f in d.iterdir())


def test_small_output_is_written_whole(tmp_path):
    out = np.random.default_rng(1).integers(0, 256, (30, 48, 4), dtype=np.uint8)
    assert bench.dump_outputs(str(tmp_path), out) == ["output"]
    got = np.load(tmp_path / "output.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, out)


def test_large_output_is_a_fixed_sample_of_rows(tmp_path):
    out = np.random.default_rng(2).integers(0, 256, (3240, 5760, 4), dtype=np.uint8)
    for d in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / d), out) == ["output", "output_rows"]
    assert 0.9 * bench.DUMP_LIMIT_BYTES < _total_bytes(tmp_path / "a") <= bench.DUMP_LIMIT_BYTES
    rows, got = np.load(tmp_path / "a" / "output_rows.npy"), np.load(tmp_path / "a" / "output.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float32
    idx = rows.astype(np.int64)
    assert (idx == rows).all() and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < out.shape[0]
    np.testing.assert_array_equal(got, out[idx])
    # the same rows in every run
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "output_rows.npy"))


def test_ranks_share_the_bound(tmp_path):
    out = np.ones((1620, 5760, 4), dtype=np.float32)
    names = [bench.dump_outputs(str(tmp_path), out, rank=r, world=4) for r in range(4)]
    assert names == [[f"output_rank{r}", f"output_rows_rank{r}"] for r in range(4)]
    assert _total_bytes(tmp_path) <= bench.DUMP_LIMIT_BYTES


def test_a_row_over_the_bound_is_refused(tmp_path):
    out = np.zeros((4, 4_000_000, 4), dtype=np.uint8)  # one row is 64 MB as float32: no sample of whole rows fits
    with pytest.raises(ValueError, match="exceeds"):
        bench.dump_outputs(str(tmp_path), out)
    assert not list(tmp_path.iterdir())
