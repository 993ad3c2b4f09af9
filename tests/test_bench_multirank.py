"""bench.py as the driver launches it for N > 1 (python -m torch.distributed.run ... bench.py --gpus N ...), world 2 on CPU:
the script's own control flow -- both gather algorithms and the no-gather form in one run, max-over-ranks timing, ONE JSON
line from rank 0 -- over gloo with the emulated library (tests/bench_dryrun.py).  The second gather algorithm runs under a
watchdog: when it never returns, every rank gives up and the line is still printed."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, extra_env, timeout, torchrun=True, gpus=None, extra_args=()):
    env = dict(os.environ)
    env.update(extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):          # (the launch decides them)
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    args = [os.path.join(ROOT, "tests", "bench_dryrun.py"), "--gpus", str(world if gpus is None else gpus), "--steps", "1",
            "--warmup", "1", "--sentences", "4500", "--model", "uni32k"] + list(extra_args)
    if torchrun:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + args
    else:
        cmd = [sys.executable] + args
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, lines


def test_bench_two_ranks_times_both_gathers_and_prints_one_line():
    p, lines = _run(2, {}, 600, extra_args=["--full"])      # (--full: the roofline's profiled loop too)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["scaling"] == "weak" and d["unit"] == "sentences/s"
    for k in ("value_gather_all_gather", "value_gather_p2p_exact", "value_gather_none"):
        assert d[k] > 0, k
    assert d["value"] == max(d["value_gather_all_gather"], d["value_gather_p2p_exact"])
    # the gather-bound model travels with the line: payload, what the links would have to carry, the predicted step and scaling
    gb = d["config"]["gather_bound"]
    assert gb["world"] == 2 and gb["payload_bytes_per_rank"] > 0 and gb["ids_wire_bytes"] in (2, 4) and gb["count_wire_bytes"] in (1, 2, 4)
    assert gb["predicted_step_ms"] >= gb["encode_ms"] > 0 and 0 < gb["predicted_scaling_vs_one_gpu"] <= 2.0
    assert abs(gb["ingest_bytes_per_rank_per_step"] - gb["payload_bytes_per_rank"]) < 1e-6          # one peer
    assert "gathers in flight" in d["config"]["gather"] and "count" in d["config"]["gather"]
    assert d["config"]["sentences_per_gpu"] == 4500 and "dp2" in d["config"]["sharding"]
    assert d["roofline"]["kernel"]


def test_bench_watchdog_prints_the_line_when_the_second_gather_hangs():
    p, lines = _run(2, {"SPMX_DRYRUN_HANG": "p2p_exact", "SPMX_BENCH_GATHER_DEADLINE_S": "8"}, 600)
    assert len(lines) == 1, (p.stdout[-1500:], p.stderr[-1500:])
    d = json.loads(lines[0])
    assert d["value"] == d["value_gather_all_gather"] > 0 and d["value_gather_none"] > 0
    assert "given up" in d["gather_p2p_exact"] and "value_gather_p2p_exact" not in d
    assert p.returncode == 0, p.stderr[-2000:]


def test_bench_watchdog_prints_the_line_when_the_first_gather_hangs():
    """No gather algorithm has run on more than one GPU before the driver's node: the no-gather form makes the line, every
    gather runs under the watchdog; when the first one never returns the line is still printed and says what it holds."""
    p, lines = _run(2, {"SPMX_DRYRUN_HANG": "all_gather", "SPMX_BENCH_GATHER_DEADLINE_S": "8"}, 600)
    assert len(lines) == 1, (p.stdout[-1500:], p.stderr[-1500:])
    d = json.loads(lines[0])
    assert d["value"] == d["value_gather_none"] > 0 and d["n_gpus"] == 2
    assert "given up" in d["gather_all_gather"] and "value_gather_all_gather" not in d
    assert d["config"]["gather"].startswith("none")
    assert p.returncode == 0, p.stderr[-2000:]


def test_bench_started_plainly_with_gpus_2_launches_two_ranks_itself():
    """`python bench.py --gpus 2` without torch.distributed.run: the script starts its ranks itself -- it must never run one
    rank and print n_gpus 1 (round-4 verdict: the only multi-GPU evidence there will be is one driver command)."""
    p, lines = _run(2, {}, 600, torchrun=False)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and "dp2" in d["config"]["sharding"] and d["value_gather_none"] > 0


def test_bench_refuses_a_gpus_flag_that_disagrees_with_the_launch():
    p, lines = _run(2, {}, 600, torchrun=True, gpus=4)
    assert p.returncode != 0 and not lines
    assert "refusing" in (p.stderr + p.stdout)


def test_bench_one_rank_runs_the_multi_rank_control_flow():
    """SPMX_BENCH_ONE_RANK_GATHER=1: process group, both gather algorithms, reserved CUs and the watchdog with ONE rank --
    how the N > 1 code is run on a one-GPU box (scripts/r05_last.sh); here over gloo with the emulated library."""
    env = dict(os.environ, SPMX_BENCH_ONE_RANK_GATHER="1", MASTER_PORT=str(_free_port()))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_dryrun.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                        "--sentences", "3000", "--model", "uni32k", "--no-second-model", "--no-side-configs", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.stdout[-1000:], p.stderr[-2000:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1
    for k in ("value_gather_all_gather", "value_gather_p2p_exact", "value_gather_none"):
        assert d[k] > 0, k
    assert d["config"]["gather"].startswith("ids:")


def test_bench_plain_line_and_dumped_outputs():
    """A plain one-GPU run (no --full): the headline and nothing measured beside it, and --dump-outputs writes the last
    timed step's ids of a fixed sample of the batch -- the same files from run to run, the oracle's ids."""
    import tempfile

    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from tests import oraclelib
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SPMX_BENCH_ONE_RANK_GATHER"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    with tempfile.TemporaryDirectory() as td:
        dumps = []
        for run in ("a", "b"):
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_dryrun.py"), "--gpus", "1", "--steps", "3",
                                "--warmup", "1", "--sentences", "3000", "--model", "uni32k", "--dump-outputs", os.path.join(td, run)],
                               cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            assert p.returncode == 0 and len(lines) == 1, (p.stdout[-1000:], p.stderr[-2000:])
            d = json.loads(lines[0])
            assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "sentences/s" and d["higher_is_better"]
            assert d["ms_per_step"] > 0 and abs(d["value"] - 3000 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
            for k in ("roofline", "long_piece_model", "c3", "c5", "end_to_end", "end_to_end_python", "cpu_baseline"):
                assert k not in d, k
            files = sorted(os.listdir(os.path.join(td, run)))
            assert files == ["id_count.npy", "id_offsets.npy", "ids.npy"], files
            dumps.append({f[:-4]: np.load(os.path.join(td, run, f)) for f in files})
        a, b = dumps
        for k in a:
            assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
        text, offs = bench.corpus_for("uni32k", 3000, 20250227, False)
        oids, oio = oraclelib.OracleLib().load(bench.model_blob("uni32k")).encode_batch(text, offs)
        oio = np.asarray(oio).astype(np.int64)
        assert a["id_count"][0] == oio[-1]
        # (a batch smaller than the sample: every sentence, in order)
        assert np.array_equal(a["id_offsets"], np.stack([oio[:-1], oio[1:]], axis=1).astype(np.float64))
        assert np.array_equal(a["ids"], np.asarray(oids)[:oio[-1]].astype(np.float32))
