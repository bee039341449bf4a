"""bench.py's own plumbing on the CPU: argument handling, the self-launch of N ranks (`--gpus 2` without a launcher starts
`python -m torch.distributed.run` as a child), the row partition + gloo gather, and the JSON line's contract fields.  The renders
come from the CPU emulator of the kernel source (RTC_BENCH_CPU_STANDIN=1: a rehearsal of the plumbing, never a measurement)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv, env_extra=None):
    env = dict(os.environ, RTC_BENCH_CPU_STANDIN="1")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_gpus_2_launches_its_own_ranks():
    """`python bench.py --gpus 2` with WORLD_SIZE unset: two ranks are started by bench.py itself, rank 0 prints the one line."""
    j = run_bench("--gpus", "2", "--workload", "smoke", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["warmup"] == 1
    # the N-rank line proves its frame too: gathered rows == the whole frame rendered by one rank
    assert j["parity"]["gathered_frame_equals_single_gpu_frame"] is True and j["parity"]["pixels"] == 64 * 36
    assert j["config"]["process_group"] == {"world_size": 2, "backend": "gloo"}
    assert j["config"]["frames_in_flight"] == 3 and j["scaling"] == "strong" and j["value"] > 0
    assert "STAND-IN" in j["data"]
    assert j["config"]["partition"].startswith("bands") and "band_partition" not in j     # 3 frames < 2 N: every frame cut into bands
    # enough frames queued (>= 2 N): whole frames round-robin over the ranks, the band partition measured beside it
    f = run_bench("--gpus", "2", "--workload", "smoke", "--steps", "5", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert f["config"]["partition"].startswith("frames") and f["steps"] == 5 and f["n_gpus"] == 2
    assert f["parity"]["gathered_frame_equals_single_gpu_frame"] is True
    assert f["band_partition"]["parity"]["gathered_frame_equals_single_gpu_frame"] is True and f["band_partition"]["value"] > 0
    assert f["config"]["unique_rays_per_frame"] == j["config"]["unique_rays_per_frame"]
    one = run_bench("--gpus", "1", "--workload", "smoke", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--extra-workloads", "")
    # same frame, same unique rays, whatever the partition
    assert one["config"]["unique_rays_per_frame"] == j["config"]["unique_rays_per_frame"]
    assert one["config"]["frames_in_flight"] == j["config"]["frames_in_flight"]


def test_bench_line_contract_fields_single_rank():
    j = run_bench("--workload", "smoke", "--steps", "2", "--warmup", "1", "--full", "--extra-workloads", "")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "parity", "ms_per_step_incl_d2h"):
        assert k in j, k
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["traffic"] is None
    a = r["algorithmic_bytes"]
    c = r["counters_rank0"]
    # the figure is recomputable from the line's own counters; kernel-argument-resident records are not in it
    want = sum(a["by_unit"].values())
    assert a["counted"] == want and a["memory"] == min(want, a["cap_4x_ideal"]) == r["algorithmic_bytes_per_launch"]
    assert a["by_unit"]["node"] + (a["lds"] and 128 * (c["accel_nodes"] - c["accel_nodes_kernarg"])) == 128 * (c["accel_nodes"] - c["accel_nodes_kernarg"])
    assert a["by_unit"]["analytic"] + (a["lds"] and 128 * (c["analytic_tests"] - c["analytic_tests_kernarg"])) == 128 * (c["analytic_tests"] - c["analytic_tests_kernarg"])
    assert a["lds"] == 0      # the emulator reports no LDS-resident tables
    assert c["accel_nodes_kernarg"] > 0 and c["analytic_tests_kernarg"] > 0      # this scene's planes and BVH root travel in the kernel arguments
    assert j["cpu_baseline"]["kind"] == "port" and j["cpu_baseline"]["cores"] >= 1
    p = j["parity"]
    assert p["primary_hit_mismatches"] == 0 and p["max_abs_drgb"] <= 1e-5 and p["pixels"] > 0 and p["timed_frame_equals_checked_frame"]


def test_plain_run_is_the_headline_and_dumps_the_last_frame(tmp_path):
    """Without --full: the contract keys and nothing measured after the timed steps; --dump-outputs writes the frame of the last timed
    step, the same bits as a whole-frame render of the workload, at N = 1 and gathered from N = 2 ranks."""
    from emu_lib import emu
    import bench
    one, two = tmp_path / "n1", tmp_path / "n2"
    j = run_bench("--workload", "smoke", "--steps", "4", "--warmup", "0", "--dump-outputs", str(one))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config"):
        assert k in j, k
    assert j["steps"] == 4 and j["warmup"] == 0 and j["value"] > 0 and j["ms_per_step"] > 0 and j["dtype"] == "f64" and j["higher_is_better"] is True
    for k in ("roofline", "valu", "parity", "cpu_baseline", "host_pixels", "ms_per_step_incl_d2h", "one_shot", "config3", "band_partition"):
        assert k not in j, k
    assert "secondary" not in j["config"]
    cam, world, _ = bench.make_workload("smoke")
    want, _ = emu().render(emu().build_world(world), cam, bench.default_fuel("smoke"), want_hits=False)
    got = np.load(one / "rgb.npy")
    assert got.dtype == np.float64 and got.shape == (cam.vsize, cam.hsize, 3)
    assert np.array_equal(got.reshape(-1, 3), want)
    f = run_bench("--gpus", "2", "--workload", "smoke", "--steps", "5", "--warmup", "1", "--dump-outputs", str(two))
    assert f["n_gpus"] == 2 and f["steps"] == 5 and "parity" not in f and "band_partition" not in f
    assert np.array_equal(np.load(two / "rgb.npy"), got)


def test_dump_outputs_samples_a_frame_over_the_budget(tmp_path, monkeypatch):
    """A frame larger than the budget (4K f64: 199 MB of 64 MB) is written as a fixed seeded pixel sample, the same pixels on every
    run (here at a budget of 1 MB)."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 ** 6)
    frame = np.arange(360 * 640 * 3, dtype=np.float64).reshape(360, 640, 3)
    bench.dump_outputs(str(tmp_path / "a"), frame)
    bench.dump_outputs(str(tmp_path / "b"), frame)
    assert not (tmp_path / "a" / "rgb.npy").exists()
    px, rgb = np.load(tmp_path / "a" / "rgb_sample_pixel.npy"), np.load(tmp_path / "a" / "rgb_sample.npy")
    assert px.dtype == np.float64 and rgb.dtype == np.float64 and rgb.shape == (px.size, 3) and px.size > 0
    assert np.array_equal(rgb, frame.reshape(-1, 3)[px.astype(np.int64)])
    assert np.array_equal(px, np.load(tmp_path / "b" / "rgb_sample_pixel.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
