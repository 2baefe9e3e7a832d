"""bench.py --dump-outputs / --full: the files a dump holds (exact integers
as float32 / float64, one seeded sample of the groups past the byte budget),
and on the GPU one small plain run: the line's fields, no CPU baseline
without --full, the dumped arrays against the line's own statistics."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_exact_and_sampled(tmp_path):
    import torch
    G = 1000
    i64 = torch.arange(G, dtype=torch.int64)
    named = {"a8": (i64 % 251).to(torch.uint8), "b16": (i64 - 500).to(torch.int16),
             "c32": torch.arange(2 * G, dtype=torch.int32) - 7, "d64": i64 * 3,
             "e64": i64 - 5,                                   # negative: as a u64 past 2^53, so halves
             "f64": torch.arange(3 * G, dtype=torch.int64) + (1 << 60)}
    stats = np.arange(9, dtype=np.uint64)
    d = str(tmp_path / "all")
    bench.dump_outputs(d, "", G, named, stats, 1 << 30)
    got = _load(d)
    assert set(got) == {"a8", "b16", "c32", "d64", "e64_lo32", "e64_hi32", "f64_lo32", "f64_hi32", "stats"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["a8"].dtype == np.float32 and np.array_equal(got["a8"], named["a8"].numpy())
    assert got["b16"].dtype == np.float32 and np.array_equal(got["b16"], named["b16"].numpy())
    assert got["c32"].shape == (G, 2) and np.array_equal(got["c32"], named["c32"].numpy().reshape(G, 2))
    assert got["d64"].dtype == np.float64 and np.array_equal(got["d64"], named["d64"].numpy())
    for k, shape in (("e64", (G,)), ("f64", (G, 3))):
        back = (got[k + "_hi32"].astype(np.uint64) << np.uint64(32)) | got[k + "_lo32"].astype(np.uint64)
        assert np.array_equal(back.view(np.int64), named[k].numpy().reshape(shape))
    assert np.array_equal(got["stats"], np.arange(9))

    # past the budget: the same sorted sample of the groups from every array, the same on every run
    d2, d3 = str(tmp_path / "s1"), str(tmp_path / "s2")
    bench.dump_outputs(d2, "w_", G, named, stats, 20000)
    bench.dump_outputs(d3, "w_", G, named, stats, 20000)
    s1, s2 = _load(d2), _load(d3)
    assert sorted(s1) == sorted(s2) and all(np.array_equal(s1[k], s2[k]) for k in s1)
    assert sum(os.path.getsize(os.path.join(d2, f)) for f in os.listdir(d2)) <= 20000 + 128 * len(s1)
    keep = s1["w_sample_groups"].astype(np.int64)
    assert 0 < len(keep) < G and np.all(np.diff(keep) > 0) and keep[-1] < G
    assert np.array_equal(s1["w_a8"], named["a8"].numpy()[keep])
    assert np.array_equal(s1["w_c32"], named["c32"].numpy().reshape(G, 2)[keep])
    assert np.array_equal(s1["w_d64"], named["d64"].numpy()[keep])


def test_steps_checked_before_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    G, steps = 2048, 3
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--groups", str(G), "--dump-outputs", d], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == 1
    assert line["unit"] == "decisions/s" and line["higher_is_better"] is True and line["dtype"] == "u8/u64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(G * steps / (line["ms_per_step"] * steps * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None                       # --full only
    got = _load(d)
    assert {"new_commit", "committed", "n_entries", "digest", "median", "new_head", "append_head", "min_apply",
            "publish", "ssn", "stats"} <= set(got)
    assert "sample_groups" not in got                         # 2048 groups: far under the budget
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert all(v.shape[0] == G for k, v in got.items() if k != "stats")
    # the dumped arrays are the last step's: they add up to the statistics that step left
    assert int((got["committed"] == 1).sum()) == line["stats"]["advanced"]
    assert int(got["n_entries"].sum()) == line["stats"]["committed_entries"]
    assert line["stats"]["decisions"] == G
