"""CPU: bench.py's host-side pieces — what a plain run and a --full run switch on, and the files
--dump-outputs writes (names, dtypes, the seeded row sample, the size bound)."""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_measures_the_headline_only(capsys):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.cpu_seconds == 0 and a.no_extras and a.no_perf
    assert capsys.readouterr().err == ""
    # options that only trim a --full run are named on stderr, and still do nothing
    a = bench.parse(["--cpu-seconds", "5", "--no-perf"])
    assert a.cpu_seconds == 0 and a.no_extras and a.no_perf
    err = capsys.readouterr().err
    assert "--cpu-seconds" in err and "--no-perf" in err and "--full" in err
    bench.parse(["--cpu-sec=5"])   # an abbreviation argparse accepts is named too
    assert "--cpu-seconds" in capsys.readouterr().err


def test_full_run_keeps_todays_defaults_and_trims(capsys):
    a = bench.parse(["--full"])
    assert a.cpu_seconds == 12.0 and not a.no_extras and not a.no_perf
    a = bench.parse(["--full", "--cpu-seconds", "3", "--no-extras", "--dump-outputs", "d"])
    assert a.cpu_seconds == 3.0 and a.no_extras and not a.no_perf and a.dump_outputs == "d"
    assert capsys.readouterr().err == ""


def _outputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (B, bench.N_FULL), dtype=torch.int8, generator=g),
            torch.randint(0, 2, (B,), dtype=torch.uint8, generator=g),
            torch.randint(1, 9, (B,), dtype=torch.int32, generator=g))


@pytest.mark.parametrize("B", [5, bench.DUMP_ROWS + 88])
def test_dump_outputs_files(tmp_path, B):
    out = _outputs(B, B)
    d1, d2 = str(tmp_path / "a" / "b"), str(tmp_path / "c")   # missing parents are created
    bench.dump_outputs(d1, out)
    bench.dump_outputs(d2, _outputs(B, B + 1))
    assert sorted(os.listdir(d1)) == ["ck.npy", "ck_rows.npy", "iters.npy", "status.npy"]
    got = {n[:-4]: np.load(os.path.join(d1, n)) for n in os.listdir(d1)}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    n = min(B, bench.DUMP_ROWS)
    rows = got["ck_rows"].astype(np.int64)
    assert rows.shape == (n,) and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < B
    # the same rows whatever the data: two builds' dumps line up codeblock for codeblock
    assert np.array_equal(got["ck_rows"], np.load(os.path.join(d2, "ck_rows.npy")))
    assert got["ck"].shape == (n, bench.N_FULL)
    assert np.array_equal(got["ck"], out[0].numpy()[rows])
    assert np.array_equal(got["status"], out[1].numpy()) and np.array_equal(got["iters"], out[2].numpy())
    assert not np.array_equal(got["ck"], np.load(os.path.join(d2, "ck.npy")))


def test_dump_of_the_default_batch_stays_under_64_MB(tmp_path):
    """The files dump_outputs really writes for the default batch, summed."""
    B = bench.parse([]).batch
    assert B == 4096
    out = (torch.zeros((B, bench.N_FULL), dtype=torch.int8), torch.zeros((B,), dtype=torch.uint8),
           torch.zeros((B,), dtype=torch.int32))
    bench.dump_outputs(str(tmp_path), out)
    total = sum(os.path.getsize(os.path.join(tmp_path, n)) for n in os.listdir(tmp_path))
    assert 0 < total < 64e6
