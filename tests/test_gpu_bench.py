"""bench.py's plain run and --dump-outputs at a tiny configuration (64 envs, T = 8): the result
line holds the headline fields and none of the --full legs, --steps sets the timed steps, and two
runs with the same arguments dump the same arrays (seeded inputs, deterministic kernels)."""
import glob
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(monkeypatch, capsys, out_dir, steps):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                                      "--envs", "64", "--frag", "8", "--dump-outputs", str(out_dir)])
    bench.main()
    line = capsys.readouterr().out.strip().splitlines()[-1]
    return json.loads(line), {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(out_dir, "*.npy"))}


def test_plain_run_result_line_and_reproducible_dump(tmp_path, monkeypatch, capsys):
    res, a = _run(monkeypatch, capsys, tmp_path / "a", 2)
    _, b = _run(monkeypatch, capsys, tmp_path / "b", 2)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["dtype"] == "fp32" and res["higher_is_better"] is True
    assert res["unit"] == "env-steps/s" and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(8 * 64 / (res["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"pcie_inclusive", "cpu_baseline", "cpu_baseline_all_cores"} & set(res)
    names = {f"{k}_{p}" for p in range(4) for k in ("params", "adam_m", "adam_v", "stats", "records",
                                                    "last_values", "adv_norm")} | {"kl_coeff"}
    assert set(a) == set(b) == names
    for k in names:
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert sum(x.nbytes for x in a.values()) < 64 << 20
    for p in range(4):
        assert a[f"params_{p}"].shape == (13253,)
        assert a[f"stats_{p}"].shape == (10 * 4, 8)        # 10 epochs x (8 * 64 / 128) minibatches
        assert a[f"records_{p}"].shape[0] == 8 * 64        # fewer rows than the sample keeps: all of them
        assert np.abs(a[f"adam_v_{p}"]).max() > 0          # the update ran


def test_steps_below_one_is_refused(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.main()
