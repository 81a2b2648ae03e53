"""bench.py's own contract: a plain run measures the headline only and says so in its line; --dump-outputs writes the last
timed step's RGB24 images (a seeded sample of whole rows + a checksum of every row) as float .npy files within the size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _row_checksums(img, width):
    v = img[:, :3 * width].astype(np.int64)
    return (v * (np.arange(3 * width) % 251 + 1)).sum(axis=1)


def test_dump_outputs_writes_a_seeded_row_sample_and_exact_row_checksums(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(7)
    W, H = 100, 70
    imgs = [torch.randint(0, 256, (H + 3, 3 * W + 16), dtype=torch.uint8, generator=g) for _ in range(5)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), imgs, W, H)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["rgb_row_checksums.npy", "rgb_rows.npy", "rgb_rows_index.npy"]
    for n in names:  # the same images give the same files
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes(), n
    sums = np.load(tmp_path / "a" / "rgb_row_checksums.npy")
    rows = np.load(tmp_path / "a" / "rgb_rows.npy")
    index = np.load(tmp_path / "a" / "rgb_rows_index.npy")
    assert sums.dtype == np.float64 and rows.dtype == np.float32 and index.dtype == np.float64
    assert sums.shape == (5, H) and rows.shape == (len(index), 3 * W) and 0 < len(index) <= bench.DUMP_MAX_ROWS
    for i, im in enumerate(imgs):
        assert np.array_equal(sums[i], _row_checksums(im.numpy()[:H], W))
    for (i, y), row in zip(index.astype(int), rows):
        assert 0 <= y < H and np.array_equal(row, imgs[i].numpy()[y, :3 * W].astype(np.float32))


def test_dump_outputs_stays_within_its_budget(tmp_path, monkeypatch):
    bench = _bench()
    W, H, n = 64, 50, 40
    budget = 20_000
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    imgs = [torch.full((H, 3 * W), i, dtype=torch.uint8) for i in range(n)]
    bench.dump_outputs(str(tmp_path), imgs, W, H, "_rank1")
    files = sorted(os.listdir(tmp_path))
    assert files == ["rgb_row_checksums_rank1.npy", "rgb_rows_index_rank1.npy", "rgb_rows_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= budget + 3 * 128  # (+ the .npy headers)
    sums = np.load(tmp_path / "rgb_row_checksums_rank1.npy")
    assert sums.shape[0] == n and sums.shape[1] < H  # rows summed in bands to fit
    for i in range(n):
        assert sums[i].sum() == _row_checksums(imgs[i].numpy(), W).sum()


@pytest.mark.gpu
def test_plain_run_times_the_steps_it_is_given_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--images", "2", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["metric"] == "megapixels/sec HEIC grid->RGB24" and res["unit"] == "MP/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert "not run" in res["config"]["parity"] and "cpu_baseline" not in res and res["dist"] is None
    sums = np.load(out / "rgb_row_checksums.npy")
    rows = np.load(out / "rgb_rows.npy")
    index = np.load(out / "rgb_rows_index.npy").astype(int)
    assert sums.shape == (2, 3024) and rows.shape == (len(index), 3 * 4032)
    assert (sums > 0).all()  # every row of both images was written
    for (i, y), row in zip(index, rows):
        assert sums[i, y] == (row.astype(np.int64) * (np.arange(3 * 4032) % 251 + 1)).sum()
