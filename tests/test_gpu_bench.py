"""bench.py end to end on the GPU box, small shapes: the JSON contract, the self-launched multi-rank path and the native
communicator (RCCL with one rank; two ranks over the shared-memory transport -- RCCL refuses two ranks on one GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--pairs", "60", "--height", "256", "--width", "384", "--steps", "3", "--warmup", "1", "--sustained-s", "1"]


def run_bench(args, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, cwd=ROOT, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]            # ONE JSON line on stdout, nothing else (RCCL's banner goes to stderr)
    return json.loads(lines[0])


def one_launch(lib, seed, pairs, pair_offset=0, H=256, W=384):
    """(4, pairs, n_rows, n_cols): ONE launch over bench.py's synthetic stack of `seed` (its --seed + rank), as a rank issues it."""
    from pyorc_amd import DeviceFrames, _lib, window

    n_rows, n_cols = window.get_array_shape((H, W), (32, 32), (16, 16))
    frames = DeviceFrames.empty((pairs + 1, H, W), np.uint8)
    _lib.check(lib.lspiv_synth_particles_dev(frames.c_ptr, pairs + 1, H, W, seed, 0.02))
    _lib.check(lib.lspiv_synchronize())
    out = DeviceFrames.empty((4 * pairs, n_rows, n_cols), np.float32)
    _lib.check(lib.lspiv_piv_pairs_dev_at(frames.c_ptr, 0, pairs + 1, H, W, 32, 32, 16, 16, -1.0, pair_offset, out.c_ptr, None, None))
    _lib.check(lib.lspiv_synchronize())
    return out.to_host().reshape(4, pairs, n_rows, n_cols)


def load_dump(d):
    """The four arrays of a --dump-outputs directory, decoded: finite values + their <name>_nonfinite codes."""
    out = []
    for name in ("u", "v", "corr", "s2n"):
        val, code = np.load(os.path.join(d, f"{name}.npy")), np.load(os.path.join(d, f"{name}_nonfinite.npy"))
        assert val.dtype == code.dtype == np.float32 and val.shape == code.shape, name
        assert np.isfinite(val).all() and np.isin(code, (0, 1, 2, 3)).all() and np.all(val[code != 0] == 0), name
        out.append(np.select([code == 1, code == 2, code == 3], [np.nan, np.inf, -np.inf], val))
    return np.stack(out)


@pytest.mark.gpu
def test_bench_json_contract_single_gpu(gpu):
    d = run_bench(SMALL + ["--cpu-pairs", "4", "--full"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frame-pairs/s" and d["value"] > 0
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["higher_is_better"] is True
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert r["algorithmic_bytes_per_pair"] == 2 * 256 * 384 + 16 * d["config"]["windows_per_pair"]
    # round 5: the dominant kernel timed INSIDE the launch as issued (library events), the burst's sustained twin
    assert "kernel_timing" in r and r["kernel_ms_per_launch"] > 0 and r["kernel_ms_same_launch_rescue_off"] > 0
    assert r["kernel_ms_per_launch"] <= r["launch_ms_with_rescue_kernels"] * 1.05
    assert d["sustained_pairs_per_s"] > 0 and d["config"]["sustained"]["steps"] >= 50 and d["config"]["sustained"]["seconds"] >= 1.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0
    assert c["parity_nan_mismatch"] == 0 and c["parity_max_rel_err_vs_oracle"] <= 1e-4 and "parity_float64_ties" in c and c["parity_windows_ill_posed"] == 0


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(gpu, tmp_path):
    """A run without --full: the headline keys and nothing measured after the timed steps; --dump-outputs writes the last step's
    u, v, corr, s2n (float32, one plane per pair) as finite arrays plus their non-finite codes, the same bits from run to run, and
    decoded they are what one launch over the same stack returns."""
    args = ["--pairs", "60", "--height", "256", "--width", "384", "--steps", "3", "--warmup", "1", "--dump-outputs"]
    d = run_bench(args + [str(tmp_path / "a")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frame-pairs/s" and d["dtype"] == "f32"
    # ms_per_step is rounded to 1e-4 ms: allow for that rounding
    assert abs(d["value"] - 60 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-4 / d["ms_per_step"] + 1e-4
    assert not {"roofline", "cpu_baseline", "sustained_pairs_per_s"} & set(d) and "other_configs" not in d["config"]
    run_bench(args + [str(tmp_path / "b")])
    a, b = load_dump(tmp_path / "a"), load_dump(tmp_path / "b")
    ref = one_launch(gpu, 20260927 + 2, 60)
    assert a.shape == ref.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(a, ref, equal_nan=True)


@pytest.mark.gpu
def test_bench_launches_its_own_ranks_and_gathers_over_the_native_comm(gpu, tmp_path):
    """`python bench.py --gpus 2` starts two ranks itself; on a 1-GPU box they share the device over the shared-memory
    transport (LSPIV_BENCH_SAME_DEVICE): sharding, pipelined all-gather, max-over-ranks timing and the bit check."""
    d = run_bench(SMALL + ["--gpus", "2", "--strong-pairs", "300", "--full", "--dump-outputs", str(tmp_path)], {"LSPIV_BENCH_SAME_DEVICE": "1"})
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "cpu_baseline" not in d
    # rank 0 dumps the gathered block its caller receives: every rank's 60 pairs (rank r: stack seed --seed + r, pairs 60 r ...)
    ref = np.concatenate([one_launch(gpu, 20260927 + 2 + r, 60, pair_offset=60 * r) for r in range(2)], axis=1)
    got = load_dump(tmp_path)
    assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)
    comm = d["config"]["comm"]
    assert comm["transport"] == "shm" and comm["ranks_reported_by_transport"] == 2
    assert comm["allgather_matches_single_launch"] is True and comm["same_device_plumbing_test"] is True
    assert comm["allgather_bytes_per_rank_per_step"] == 4 * 4 * 60 * d["config"]["windows_per_pair"]
    # round 4: the step is the library's own sharded path, and the line diagnoses itself
    assert "ShardedPivDev" in comm["path"] and comm["mode"] == "weak" and comm["pairs_total"] == 120 and comm["pairs_rank0"] == 60
    for key in ("kernel_ms_while_gather_in_flight", "gather_ms_overlapped", "exposed_comm_ms", "gather_end_after_kernel_end_ms",
                "allgather_ms_alone", "kernel_ms_alone", "allgather_bytes_received_per_rank_per_step", "rccl_env", "gather_stream_priority"):
        assert key in comm, key
    assert comm["kernel_ms_while_gather_in_flight"] > 0 and comm["gather_ms_overlapped"] > 0 and comm["gather_stream_priority"] == "high"
    assert abs(comm["exposed_comm_ms"] - (d["ms_per_step"] - comm["kernel_ms_while_gather_in_flight"])) < 1e-3
    assert d["config"]["binary"]["binary_hash_matches"] is True
    # round 6: the weak line also carries ONE strong pass -- north_star's reading -- timed after the weak region:
    # a fixed total cut over the ranks on the anchors (300 pairs of this small grid, anchors of 25: 150 + 150)
    assert comm["strong_pairs_total"] == 300 and comm["strong_pairs_rank0"] == 150 and comm["strong_ms_per_step"] > 0
    assert abs(comm["strong_pairs_per_s"] - 300 / (comm["strong_ms_per_step"] * 1e-3)) / comm["strong_pairs_per_s"] < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 8])
def test_bench_at_the_rank_counts_of_the_scaling_run(gpu, n):
    """The driver's N = 4 and 8: n self-launched ranks -- block sizes, the gathered (n, 4, pairs, windows) result against ONE launch,
    the max-over-ranks clock and the weak-scaling value.  4 ranks share device 0 over the shared-memory transport (5 processes with
    the device open, this one included); 8 ranks get one device each: on one device they would be 9 processes holding it at once,
    more than a shared GPU node lets one job open.  The 8-rank sharding of pyorc_amd.shard over the native shared-memory
    communicator runs on CPU ranks in tests/test_shard_gloo.py (world 8)."""
    from pyorc_amd import _lib

    found = _lib.device_count()
    if n > 4 and found < n:
        pytest.skip(f"needs {n} GPUs (one rank per device), found {found}")
    d = run_bench(["--pairs", "25", "--height", "256", "--width", "384", "--steps", "2", "--warmup", "1", "--gpus", str(n), "--full"],
                  {"LSPIV_BENCH_SAME_DEVICE": "1"} if n <= 4 else {})
    comm = d["config"]["comm"]
    assert d["n_gpus"] == n and d["scaling"] == "weak" and comm["ranks_reported_by_transport"] == n
    assert comm["pairs_total"] == 25 * n and comm["pairs_rank0"] == 25 and comm["allgather_matches_single_launch"] is True
    assert comm["allgather_bytes_received_per_rank_per_step"] == (n - 1) * comm["allgather_bytes_per_rank_per_step"]
    assert abs(d["value"] - 25 * n / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3


@pytest.mark.gpu
def test_bench_strong_mode_cuts_a_fixed_total(gpu):
    """`--strong`: a fixed total (here 150 pairs) cut over the ranks on the walking kernels' anchors (75 + 75), value = total / time."""
    d = run_bench(SMALL + ["--gpus", "2", "--strong", "--strong-pairs", "150", "--full"], {"LSPIV_BENCH_SAME_DEVICE": "1"})
    comm = d["config"]["comm"]
    assert d["scaling"] == "strong" and comm["mode"] == "strong" and comm["pairs_total"] == 150 and comm["pairs_rank0"] == 75
    assert comm["allgather_matches_single_launch"] is True
    assert abs(d["value"] - 150 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3


@pytest.mark.gpu
def test_bench_over_rccl_with_one_rank(gpu):
    """The RCCL transport itself (librccl.so dlopen'ed by the C library, ncclCommInitRank, ncclAllGather on a second
    stream, all-reduce for the timing), with the one rank a 1-GPU box allows."""
    d = run_bench(SMALL + ["--gpus", "1", "--cpu-pairs", "0", "--no-extras", "--full"], {"LSPIV_BENCH_FORCE_COMM": "1"})
    comm = d["config"]["comm"]
    assert comm["transport"] == "rccl" and comm["ranks_reported_by_transport"] == 1
    assert comm["allgather_matches_single_launch"] is True
    assert comm["rccl_env"].get("NCCL_MAX_NCHANNELS") == "16"       # the default cap on RCCL's CU take is in force and recorded


@pytest.mark.gpu
def test_bench_falls_back_to_shared_memory_when_rccl_cannot_be_brought_up(gpu):
    """Round 6: RCCL has never met two ranks on the boxes this was built on.  A node on which it cannot be brought up must still yield a
    line that says so: the ranks vote on their communicator and, unless all of them succeeded, all of them fall back to the shared-memory
    transport and the line carries the error.  Provoked here with two ranks on ONE device, which RCCL refuses ("Duplicate GPU")."""
    d = run_bench(SMALL + ["--gpus", "2", "--strong-pairs", "300", "--full"], {"LSPIV_BENCH_SAME_DEVICE": "1", "LSPIV_COMM": "rccl"})
    comm = d["config"]["comm"]
    assert d["n_gpus"] == 2 and comm["transport"] == "shm" and comm["ranks_reported_by_transport"] == 2
    assert "rccl_error" in comm and "rank" in comm["rccl_error"] and "diagnosis" in comm["note"]
    assert comm["allgather_matches_single_launch"] is True and d["value"] > 0
