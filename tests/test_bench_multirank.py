"""bench.py's multi-GPU control flow at world_size 2, on CPU (gloo).

The driver runs `torch.distributed.run --nproc-per-node N bench.py` on an
8-GPU node; no session here has one.  This runs bench.main() itself in two
gloo ranks with the device pieces stood in: the engine by a CPU stand-in that
answers from the oracle (so the parity sample is meaningful and the step
counts are the sequential TimedT's), torch.cuda's synchronisation by no-ops,
the library's RCCL job by nothing (the stand-in all-reduces its statistics
over gloo, as tw_run's reduction does over RCCL).  What is checked is bench.py's
own logic: BASELINE config 3's strong split (one batch over the ranks, rank 0
printing the whole job's line), the weak line measured after it and reported
beside it, the geometry choice per rank share, the barrier + max-over-ranks
timing, and the parity sample rank 0 keeps at N > 1."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Stats:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _worker(rank, world, port, out_path, argv):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "time-warp_amd"), os.path.join(ROOT, "oracle")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import io
    from contextlib import redirect_stdout

    import torch
    import torch.distributed as dist

    import oracle
    from timewarp import dist as twd
    from timewarp import engine as eng_mod

    real_init, real_reduce = dist.init_process_group, twd.reduce_stats
    dist.init_process_group = lambda backend=None, **kw: real_init("gloo", **kw)
    torch.cuda.set_device = lambda *a, **k: None
    torch.cuda.synchronize = lambda *a, **k: None
    twd.library_comm = lambda world, rank: None
    twd.reduce_stats = lambda local, device=None: real_reduce(local)

    class FakeEngine:
        """tw_run's contract on CPU: the oracle's results, job-wide statistics."""

        def __init__(self, device, comm=None):
            self.geo, self.tie = None, "fifo"

        def load(self, scn, geometry=None):
            self.scn, self.geo = scn, geometry or "dense"
            return self

        def geometry(self):
            return self.geo

        def set_tie_mode(self, t):
            self.tie = t
            return self

        def reset(self):
            pass

        def run(self):
            self.res, self.h = oracle.run_batch(self.scn, threads=2)
            r = self.res
            loc = {"events": int(r["events"].sum()), "delivered": int(r["delivered"].sum()),
                   "dropped": int(r["dropped"].sum()), "undeliverable": int(r["undeliverable"].sum()),
                   "replicas_error": int((r["status"] >= 3).sum())}
            job = real_reduce(loc)
            return _Stats(events=int(job["events"]), delivered=int(job["delivered"]), dropped=int(job["dropped"]),
                          undeliverable=int(job["undeliverable"]),
                          sends=int(job["delivered"] + job["dropped"] + job["undeliverable"]), launches=1,
                          replicas_error=int(job["replicas_error"]))

        def results(self):
            return self.res

        def hashes(self):
            return self.h

        def launch_ms(self):
            return np.array([1.0])

        def lpb_windows(self):
            return (1, 1)

        def close(self):
            pass

    eng_mod.Engine = FakeEngine
    import bench

    sys.argv = ["bench.py"] + argv
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    if rank == 0:
        with open(out_path, "w") as f:
            f.write(buf.getvalue())


def test_bench_plain_run_and_dump(tmp_path, oracle_mod):
    """A plain run (no --full) at N = 1: the line keeps its headline keys and
    carries nothing of the oracle or the host table check; --dump-outputs
    writes the last step's results and hashes as float64, the same files for
    the same arguments."""
    from timewarp import scenarios

    lines, dumps = [], []
    for i in range(2):
        out, d = str(tmp_path / f"line{i}.txt"), tmp_path / f"dump{i}"
        argv = ["--gpus", "1", "--config", "token_ring", "--replicas", "8", "--nodes", "8", "--duration-s", "5",
                "--host-tables", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)]
        mp.spawn(_worker, args=(1, _free_port(), out, argv), nprocs=1, join=True)
        lines.append([ln for ln in open(out).read().splitlines() if ln.startswith("{")])
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    assert len(lines[0]) == 1
    line = json.loads(lines[0][0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "events/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["ms_per_step"] > 0 and line["value"] > 0 and "token-ring" in line["metric"]
    for k in ("cpu_baseline", "parity_sample", "weak_line"):
        assert k not in line
    assert "host_check_equal" not in line["setup"] and "traffic_source" not in line["roofline"]
    scn = scenarios.token_ring(n_nodes=8, n_replicas=8, launch_duration=5_000_000, drop_log2=10)
    ores, ohashes = oracle_mod.run_batch(scn, threads=4)
    a, b = dumps
    assert set(a) == set(b) and {"results.npy", "hashes.npy", "hash_fold.npy", "stats.npy"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    assert np.array_equal(a["results_replicas.npy"], np.arange(8))
    for j, f in enumerate(("final_t", "events", "delivered", "dropped", "undeliverable", "status", "main_exc",
                           "threads")):
        assert np.array_equal(a["results.npy"][:, j], ores[f].astype(np.float64)), f
    h = (a["hashes.npy"][..., 0].astype(np.uint64) << np.uint64(32)) | a["hashes.npy"][..., 1].astype(np.uint64)
    assert np.array_equal(h, ohashes)
    fold = (a["hash_fold.npy"][:, 0].astype(np.uint64) << np.uint64(32)) | a["hash_fold.npy"][:, 1].astype(np.uint64)
    assert np.array_equal(fold, ohashes.sum(axis=1, dtype=np.uint64))


def test_bench_dump_samples_large_outputs(tmp_path):
    """dump_outputs keeps a fixed seeded sample of a batch whose hashes pass
    its cap: the same rows every time, the fold over every replica's hashes."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from timewarp.abi import RESULT_DTYPE

    R, N = 3000, 1025
    assert R * N > bench.DUMP_MAX_HASHES
    rng = np.random.default_rng(1)
    res = np.zeros(R, RESULT_DTYPE)
    res["events"] = rng.integers(0, 1 << 40, R)
    hashes = rng.integers(0, 1 << 63, (R, N)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    for i in range(2):
        bench.dump_outputs(str(tmp_path / str(i)), 0, 1, res, hashes, {"events": 7, "launches": 1})
    a, b = ({f.name: np.load(f) for f in sorted((tmp_path / str(i)).iterdir())} for i in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["hashes_replicas.npy"].astype(np.int64)
    assert rows.size == bench.DUMP_MAX_HASHES // N and np.all(np.diff(rows) > 0)
    h = (a["hashes.npy"][..., 0].astype(np.uint64) << np.uint64(32)) | a["hashes.npy"][..., 1].astype(np.uint64)
    assert np.array_equal(h, hashes[rows])
    assert a["results.npy"].shape == (R, len(bench.DUMP_FIELDS))
    assert np.array_equal(a["results.npy"][:, 1], res["events"].astype(np.float64))
    fold = (a["hash_fold.npy"][:, 0].astype(np.uint64) << np.uint64(32)) | a["hash_fold.npy"][:, 1].astype(np.uint64)
    assert np.array_equal(fold, hashes.sum(axis=1, dtype=np.uint64))


@pytest.mark.parametrize("weak", [False, True])
def test_bench_two_ranks(tmp_path, oracle_mod, weak):
    out = str(tmp_path / "line.txt")
    argv = ["--config", "token_ring", "--replicas", "8", "--nodes", "8", "--duration-s", "5", "--host-tables",
            "--steps", "1", "--warmup", "0", "--cpu-seconds", "1", "--full"] + (["--weak"] if weak else [])
    mp.spawn(_worker, args=(2, _free_port(), out, argv), nprocs=2, join=True)
    lines = [ln for ln in open(out).read().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    from timewarp import scenarios

    assert d["n_gpus"] == 2 and d["steps"] == 1
    # the whole job's events: one batch of 8 replicas (strong) or 8 per rank (weak)
    total = 16 if weak else 8
    scn = scenarios.token_ring(n_nodes=8, n_replicas=total, launch_duration=5_000_000, drop_log2=10)
    ores, _ = oracle_mod.run_batch(scn, threads=4)
    assert d["config"]["events_per_step"] == int(ores["events"].sum())
    assert d["config"]["replicas_total"] == total
    assert d["config"]["replicas_rank0"] == (8 if weak else 4)
    assert d["scaling"] == ("weak" if weak else "strong")
    # batched logical processes for a share of <= 8,192 replicas (a power of two)
    assert d["config"]["geometry"] == "lpb"
    assert d["parity_sample"]["bit_exact"] and "rank 0" in d["parity_sample"]["against"]
    assert "cpu_baseline" not in d  # rank 0 at N = 1 only
    if weak:
        assert "weak_line" not in d
    else:
        assert d["config"]["baseline_config"] is None  # (only the 65,536-replica batch is config 3)
        w = d["weak_line"]
        assert w["scaling"] == "weak" and w["replicas_per_gpu"] == 8 and w["replicas_total"] == 16
        assert w["value"] > 0 and w["ms_per_step"] > 0
