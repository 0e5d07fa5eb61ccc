"""bench.py --dump-outputs: the timed path's last results as float32 / float64
.npy files, whole while they fit DUMP_BUDGET_BYTES and as a fixed seeded
sample beyond it; and --full, which alone keeps the legs besides the headline."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_flags_default_off_and_steps_are_checked():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_small_results_are_written_whole(tmp_path):
    arrays = {"f32": torch.arange(7, dtype=torch.float32) / 3, "bf16": torch.tensor([1.5, -2.25], dtype=torch.bfloat16),
              "f64": torch.tensor([1.0 / 3], dtype=torch.float64), "i64": torch.tensor([2 ** 40 + 1, -5]),
              "a/b c": torch.zeros(2, 3)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["a_b_c.npy", "bf16.npy", "f32.npy", "f64.npy", "i64.npy"]
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert got["f32"].dtype == np.float32 and np.array_equal(got["f32"], arrays["f32"].numpy())
    assert got["bf16"].dtype == np.float32 and got["bf16"].tolist() == [1.5, -2.25]
    assert got["f64"].dtype == np.float64 and got["f64"][0] == 1.0 / 3
    assert got["i64"].dtype == np.float64 and got["i64"].tolist() == [2.0 ** 40 + 1, -5.0]
    assert got["a_b_c"].shape == (2, 3)
    bench.dump_outputs(str(tmp_path), {"f32": arrays["f32"]}, rank=1)
    assert np.array_equal(np.load(tmp_path / "f32.rank1.npy"), got["f32"])


def test_large_results_are_sampled_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    big = torch.arange(6000, dtype=torch.float32)
    view = torch.arange(40 * 70, dtype=torch.float32).view(40, 70)[:, :61]  # a strided view, as the clipped rows
    small = torch.arange(5, dtype=torch.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "view": view, "small": small})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "small.npy", "view.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in files}
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert a["small.npy"].tolist() == [0, 1, 2, 3, 4]  # under its share: whole
    assert a["big.npy"].shape == (4000 // 3 // 4,) and a["view.npy"].shape == (4000 // 3 // 4,)
    # a sample holds elements of the array, at sorted positions spread over it
    assert np.all(np.diff(a["big.npy"]) >= 0) and a["big.npy"][0] < 300 and a["big.npy"][-1] > 5700
    assert np.all(np.isin(a["view.npy"], view.numpy())) and np.all(a["view.npy"] % 70 < 61)
    for n in files:  # the same positions in every run
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n))
    for r in range(2):  # the ranks of a multi-GPU run share the budget
        bench.dump_outputs(str(tmp_path / "c"), {"big": big}, rank=r, world=2)
    assert sorted(os.listdir(tmp_path / "c")) == ["big.rank0.npy", "big.rank1.npy"]
    assert sum(np.load(tmp_path / "c" / n).nbytes for n in os.listdir(tmp_path / "c")) <= 4000


@pytest.mark.gpu
def test_headline_dump_is_the_fedavg_of_the_seeded_rows(tmp_path, cuda_device):
    """Config 2's headline in process, twice: the dumped averages are those of
    the bench's own rows (fp32 chain of K terms against float64: |d| <=
    K 2^-24 sum|w_i p_i|, as each product and each partial sum rounds once),
    and a second run reproduces them bit for bit."""
    dumps = []
    for d in ("a", "b"):
        a = bench.parse(["--config", "cfg2", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
                         "--dump-outputs", str(tmp_path / d)])
        line, keep = bench.measure_headline(a, 1, 0, cuda_device, bench.SOLO)
        assert keep is None and line["cpu_baseline"] is None
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        dumps.append({n: np.load(tmp_path / d / n) for n in sorted(os.listdir(tmp_path / d))})
    assert list(dumps[0]) == ["fedavg_float32.npy"]
    got = dumps[0]["fedavg_float32.npy"]
    assert got.dtype == np.float32 and np.array_equal(got, dumps[1]["fedavg_float32.npy"])

    a = bench.parse(["--config", "cfg2", "--steps", "1", "--warmup", "0", "--full"])
    _, (bucket, ns) = bench.measure_headline(a, 1, 0, cuda_device, bench.SOLO)
    g = bucket.groups[torch.float32]
    assert got.shape == (g.length,)
    K = g.rows.shape[0]
    w = torch.tensor(bucket.weights(ns), dtype=torch.float32).double()[:, None]
    terms = g.rows[:, :g.length].cpu().double() * w
    err = (torch.from_numpy(got).double() - terms.sum(0)).abs()
    assert torch.all(err <= K * 2.0 ** -24 * terms.abs().sum(0))
