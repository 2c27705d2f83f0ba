"""Multi-rank path with the REAL kernels: two fresh processes share cuda:0, collectives over gloo
(the boxes of the pool have one GPU; on an 8-GPU node the same code runs over RCCL).  Checks that
ShardedPSF.from_lens(...).psf_volume over 2 ranks equals ONE psf_lr call over the whole grid --
same verified batch-global Newton trip tables, PSFs equal up to LDS-atomic summation order -- and
that `python bench.py --gpus 2` starts its own ranks and exits 0."""
import json
import tempfile
import os
import socket
import subprocess
import time
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env(**kw):
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", **kw)
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 8])
def test_ranks_equal_one_call_over_the_whole_grid(world):
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_worker.py")],
                              env=_env(RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_PORT=port),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=420))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, f"rank failed:\n{so}\n{se[-3000:]}"
    rec = [json.loads(so.strip().splitlines()[-1]) for so, _ in outs]
    r0 = next(r for r in rec if r["rank"] == 0)
    assert r0["max_abs_diff_L"] <= 3e-6 and r0["max_abs_diff_R"] <= 3e-6
    assert r0["tables"] == r0["solo_tables"]
    assert all(r["empty_shard_ok"] for r in rec)
    assert r0["stepper_max_abs_diff"] == 0.0 and all(r["divergence_detected"] for r in rec)
    print(f"{world}-rank vs solo:", r0["max_abs_diff_L"], r0["max_abs_diff_R"], "own tables differ:",
          r0["own_tables_differ"], r0["tables"])


@pytest.mark.gpu
def test_config3_whole_grid_sharded_over_eight_ranks(tmp_path, oracle):
    """BASELINE config 3 as stated: the 65536-point dense PSFNet grid (32 x 32 x 64 Gaussian-warped depth planes,
    deeplens/psfnet.py:220-239) x 8192 spp x 21 x 21 as ONE batch sharded over 8 ranks -- against ONE call of the CPU
    oracle over the whole batch: the batch-global Newton trip tables (deeplens/surfaces.py:547) of both passes,
    all 65536 chief-ray centres, every pixel of every L and R PSF."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from conftest import load_state, ulp_diff
    world, ks, spp = 8, 21, 8192
    st = load_state("rf50mm")
    g = torch.Generator().manual_seed(808)
    u = torch.rand(2, spp, generator=g).numpy()
    uc = torch.rand(2, 2048, generator=g).numpy()
    x2, y2 = oracle.pupil_samples(u[0], u[1], st["pupil_r"])
    xc, yc = oracle.pupil_samples(uc[0], uc[1], st["pupil_r"] * 0.25)
    pupil = np.empty(4, dtype=object)
    pupil[:] = [x2, y2, xc, yc]
    np.save(tmp_path / "pupil.npy", pupil, allow_pickle=True)
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_c3_worker.py")],
                              env=_env(RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_PORT=port,
                                       SDIRT_C3_DIR=str(tmp_path)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    # the oracle's whole-batch call (671 M rays, ~45 bytes each in flight) runs while the ranks render
    pts = bench.volume_points(world, "c3")
    N = pts.shape[0]
    assert N == 65536
    oracle.set_num_threads(bench.available_cores())
    lo, ro, co, ok, tp, tc = oracle.psf(st, pts.numpy(), x2, y2, xc, yc, ks, dp=(0.78, 1.44, 0.3, 0.5), return_trips=True)
    assert ok
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=900))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, f"rank failed:\n{so}\n{se[-3000:]}"
    r = np.load(tmp_path / "result.npz")
    assert np.array_equal(r["trips_psf"], tp), (r["trips_psf"], tp)
    assert np.array_equal(r["trips_center"], tc), (r["trips_center"], tc)
    cu = ulp_diff(r["center"], co)
    dl = np.abs(r["L"] - lo).reshape(N, -1).max(1)
    dr = np.abs(r["R"] - ro).reshape(N, -1).max(1)
    print(f"config 3 whole grid: N={N} spp={spp} ks={ks} over {world} ranks; trips primary {tp.tolist()} chief {tc.tolist()} "
          f"(launch rounds {int(r['launches'])}, re-launches {int(r['relaunches'])}); centres max {int(cu.max())} ulp "
          f"({int((cu > 0).sum())} of {cu.size} differ); max|dL| {dl.max():.3e} (point {int(dl.argmax())}) "
          f"max|dR| {dr.max():.3e} (point {int(dr.argmax())}) of peak 1")
    assert cu.max() <= 1
    # measured over four runs: max|dL| 5.2e-6 ... 5.6e-6, max|dR| 4.6e-6 ... 7.2e-6 (the one worst pixel of 57.8 M): fp32 sums of
    # up to 8192 terms in LDS-atomic order here, in sample order in the oracle (and in the reference's index_put_) -- 8192 x 4
    # additions each rounded at ~2^-24 of a peak-sized sum; the bound leaves room for the arrival order of another run
    assert dl.max() <= 1.5e-5 and dr.max() <= 1.5e-5


@pytest.mark.gpu
def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: spawns 2 ranks, prints ONE JSON
    line carrying both rates, exits 0.  (gloo dry-run backend: both ranks share cuda:0.)"""
    env = _env(SDIRT_BENCH_BACKEND="gloo", SDIRT_GATHER_TRIAL="0")       # (the trial has its own test below)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--workload", "c3", "--sustain-seconds", "0", "--full"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["gather"] is True
    assert res["value"] > 0 and res["value_no_gather"] > 0


@pytest.mark.gpu
def test_bench_config3_with_eight_ranks_on_one_gpu():
    """BASELINE config 3 as the driver would launch it on a node -- `bench.py --gpus 8 --workload c3`:
    8 ranks x 8192 points, 8192 spp, ks 21, pupil broadcast, mask all-reduce, all-gather of the
    65536-point volume to every rank -- on the ONE GPU of this pool (gloo dry-run backend: the
    control path is the node's, the numbers mean nothing).  One JSON line, n_gpus 8, rc 0."""
    env = _env(SDIRT_BENCH_BACKEND="gloo", SDIRT_GATHER_TRIAL="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2",
                        "--warmup", "1", "--workload", "c3", "--sustain-seconds", "0", "--full"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 8 and res["config"]["gather"] is True and res["config"]["name"] == "c3"
    assert res["config"]["points_per_gpu"] == 8192 and res["value"] > 0 and res["value_no_gather"] > 0
    log = os.environ.get("SDIRT_TEST_LOG_DIR")
    if log:
        with open(os.path.join(log, "bench_gpus8_dryrun_c3.log"), "w") as f:
            f.write(lines[0] + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["allgather", "direct"])
def test_bench_strong_scaling_config2_with_eight_ranks_on_one_gpu(algo, tmp_path):
    """`bench.py --gpus 8` -- strong scaling is the DEFAULT for N > 1: config 2's ONE 16384-point volume
    cut into 8 shards of 2048 points, the 554 MB volume all-gathered to every rank (485 MB received per rank and step),
    with both gather algorithms -- on the one GPU of this pool (gloo dry run: the control path is the node's, the numbers
    mean nothing).  The JSON line (< 4 KB) carries what makes a real 8-GPU run interpretable: the BASELINE config by name,
    scaling, world size, gather bytes / ms / gather_bound."""
    env = _env(SDIRT_BENCH_BACKEND="gloo", SDIRT_GATHER_ALGO=algo)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
                        "--sustain-seconds", "0", "--full", "--detail-file", str(tmp_path / "detail.json")],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    assert len(lines[0]) < 4000
    res = json.loads(lines[0])
    assert res["n_gpus"] == 8 and res["world_size"] == 8 and res["scaling"] == "strong"
    assert res["config"]["workload"].startswith("BASELINE config 2") and "16384 points" in res["config"]["workload"]
    assert json.load(open(tmp_path / "detail.json"))["config"]["points_total"] == 16384
    assert res["config"]["points_per_gpu"] == 2048 and res["config"]["name"] == "c2" and res["config"]["gather"] is True
    assert res["value"] > 0 and res["value_no_gather"] > 0
    # rays of ONE 16384-point volume per step, whatever the number of ranks
    assert abs(res["value"] * res["ms_per_step"] * 1e-3 / (16384 * 4096) - 1) < 1e-4
    g = res["gather"]
    assert g["algo"] == algo and g["world_size"] == 8 and g["backend"] == "gloo"
    assert abs(g["gb_received_per_rank_per_step"] - 2 * 7 * 2048 * 65 * 65 * 4 / 1e9) < 1e-6        # 0.485 GB (six digits on the line)
    assert g["ms"] > 0 and g["compute_ms"] > 0 and isinstance(g["gather_bound"], bool)
    assert g["collectives_per_step"] == 1                      # one [2048, 2, 65, 65] block per rank, rendered in place
    log = os.environ.get("SDIRT_TEST_LOG_DIR")
    if log:
        with open(os.path.join(log, f"bench_gpus8_dryrun_c2_strong_{algo}.log"), "w") as f:
            f.write(lines[0] + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("fake", [None, "hang", "raise"])
def test_bench_gather_trial_and_its_deadline(fake, tmp_path):
    """`bench.py --gpus 4` with no gather algorithm named: the run ends with the K timed steps once more on 'direct'
    (gather.trial: both figures, checksums of both volumes, which one `value` is) -- and an experiment that hangs or raises
    (SDIRT_BENCH_FAKE_TRIAL) costs nothing: rank 0 prints the record it already had, every rank leaves, rc 0."""
    env = _env(SDIRT_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SDIRT_GATHER_ALGO", "SDIRT_GATHER_TRIAL"):
        env.pop(k, None)
    if fake:
        env.update(SDIRT_BENCH_FAKE_TRIAL=fake, SDIRT_BENCH_TRIAL_DEADLINE_S="8")
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1",
                        "--workload", "c3", "--sustain-seconds", "0", "--full", "--detail-file", str(tmp_path / "detail.json")],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 4000, p.stdout
    res = json.loads(lines[0])
    g = res["gather"]
    assert res["n_gpus"] == 4 and res["value"] > 0 and g["volume_checksums_equal"] is True
    t = g["trial"]
    if fake is None:
        assert t["direct_ms_per_step"] > 0 and t["allgather_ms_per_step"] > 0 and t["direct_volume_checksums_equal"] is True
        assert t["direct_gather_ms"] > 0
        assert t["adopted"] in ("allgather", "direct") and g["algo"] == t["adopted"]
        assert res["value_allgather"] > 0 and res["value_direct"] > 0
        assert res["value"] == pytest.approx(res["value_" + t["adopted"]], rel=1e-5)
    else:
        assert t["adopted"] == "allgather" and g["algo"] == "allgather"
        assert ("no result within" in t["direct"]) if fake == "hang" else ("SDIRT_BENCH_FAKE_TRIAL" in t["direct"])
        assert "value_direct" not in res
    assert time.time() - t0 < 600
    log = os.environ.get("SDIRT_TEST_LOG_DIR")
    if log:
        with open(os.path.join(log, f"bench_gpus4_dryrun_c3_trial_{fake or 'ran'}.log"), "w") as f:
            f.write(lines[0] + "\n")


@pytest.mark.gpu
def test_rccl_backend_accepts_the_collectives_of_the_multi_gpu_path():
    """tests/rccl_single_rank_worker.py: backend "nccl" (= RCCL) with one rank on the one GPU."""
    env = _env(MASTER_PORT=str(_free_port()))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_single_rank_worker.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "rccl single-rank collectives ok" in p.stdout


@pytest.mark.gpu
def test_the_multi_rank_step_over_rccl_on_one_gpu():
    """`bench.py --workload sweep`: the loop `--gpus N` runs, with every collective issued on a world-1 RCCL process group --
    pupil broadcast on its own communicator and stream, the mask all-reduce on the read-back stream, the shard rendered in
    place into the [n, 2, ks, ks] block that ONE all-gather moves -- for config 2 cut to the step of a rank of 1 / 2 / 4 / 8.
    Every k-th point keeps the whole volume's batch-global trip tables; ONE JSON line on stdout (RCCL's banner goes to stderr)."""
    detail = os.path.join(os.environ.get("SDIRT_TEST_LOG_DIR") or tempfile.mkdtemp(), "bench_sweep_detail.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "sweep", "--detail-file", detail], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < 4000, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert set(d["sweep_summary"]) >= {"single_gpu_loop_16384", "world8_shard_2048", "world8_shard_2048_two_streams"}
    rows = json.load(open(detail))["shard_sweep"]
    assert {"single_gpu_loop_16384", "world1_shard_16384", "world2_shard_8192", "world4_shard_4096", "world8_shard_2048"} <= set(rows)
    for name, r in rows.items():
        assert r["relaunches_in_timed_region"] == 0 and r["kernel_ms"] > 0, (name, r)
        # physical figures only: wall time between two fences / steps
        assert r["ms_per_step"] > 0 and r["host_us_per_step"] > 0 and 0.0 < r["efficiency"] <= 1.05, (name, r)
        assert r.get("gpu_idle_us_per_step", 0.0) >= 0.0
        if name.startswith("world"):
            assert r["trip_tables_equal_full_batch"] and r["gather_ms"] > 0, (name, r)
            assert r["steps"] >= (500 if r["points_per_step"] <= 4096 else 100)
    # one render stream, every collective in the loop: the kernel's own end-of-launch cost is what is left (1.150 of 8.86 / 8
    # = 0.96 by the kernel alone, profiles/r06/end_ab_product.txt)
    # (a sanity bound, not a performance gate: measured 0.89-0.93 on five boxes of the pool with 0.11-0.16 ms of host work per
    # step, profiles/r06/bench_c2_detail.json; the boxes are shared and differ)
    assert rows["world8_shard_2048"]["efficiency"] > 0.7 and rows["world8_shard_2048"]["host_us_per_step"] < 1000
    assert rows["world8_shard_2048"]["points_per_step"] == 2048
    log = os.environ.get("SDIRT_TEST_LOG_DIR")
    if log:
        with open(os.path.join(log, "bench_sweep.json"), "w") as f:
            f.write(lines[0] + "\n")
