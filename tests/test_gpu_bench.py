"""bench.py as a command: a plain run does the headline run only, ``--full`` adds every other measurement to the same line.
The workload is shrunk with ``--n-total`` (K stays 128, so the timed steps take the benchmark's own kernels); nothing here
asserts a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric": "mbar_adaptive_iterations_per_sec", "unit": "iter/s", "higher_is_better": True, "dtype": "f64", "n_gpus": 1,
            "steps": 3, "warmup": 1}
# what the line carries only with --full
BEYOND = ("cpu_baseline", "wallclock_to_converge_s", "iterations_to_converge", "converged", "per_solve", "max_abs_error_vs_analytic_f",
          "gnorm_at_solution", "api_end_to_end", "config2", "config4", "config4_one_device", "config5", "scaling_model",
          "speedup_vs_cpu_baseline")
DUMPED = ("f_k", "psum", "gnorm", "max_delta", "iterations_nr_sci")


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--n-total", "200000", *extra], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-800:])
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    for key, val in HEADLINE.items():
        assert line[key] == val, key
    assert line["value"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-12)
    return line


def test_help_names_the_full_option():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_run_alone(tmp_path):
    line = run_bench("--dump-outputs", str(tmp_path / "out"))
    assert line["full"] is False
    assert not [k for k in BEYOND if k in line]
    assert "measured_mfma_f64_peak_tflops" not in line["roofline"]
    # the figures that come out of the timed steps' own timers stay in the plain line
    assert line["roofline"]["launches"] > 0 and line["roofline"]["avg_launch_ms"] > 0
    assert line["ms_per_step_outside_the_sweeps"] < line["ms_per_step"]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".npy" for n in DUMPED)
    f_k = np.load(tmp_path / "out" / "f_k.npy")
    assert f_k.shape == (128,) and f_k.dtype == np.float64 and np.all(np.isfinite(f_k))
    assert list(np.load(tmp_path / "out" / "iterations_nr_sci.npy"))[0] == 3


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements_to_the_same_line():
    line = run_bench("--full", "--cpu-sample", "20000")
    assert line["full"] is True
    # (scaling_model and config4_one_device belong to the 1e7-sample workload, config4 to 8 GPUs: present, and null at this size)
    assert not [k for k in BEYOND if k not in line]
    assert line["converged"] is True and np.isfinite(line["max_abs_error_vs_analytic_f"])
    assert set(line["per_solve"]) == {"adaptive_min_sc_iter_0", "adaptive_min_sc_iter_2", "adaptive_min_sc_iter_0_warm_start"}
    assert line["cpu_baseline"]["value"] > 0 and line["api_end_to_end"]["finite"] is True
    assert line["config2"]["sci_converged"] is True and line["config5"]["finite"] is True
    assert line["roofline"]["measured_mfma_f64_peak_tflops"] > 0
    assert line["scaling_model"] is None and line["config4_one_device"] is None and line["config4"] is None
