"""bench.py's strong-scaling share options on one GPU (--assign cost / --share R/N): the share a rank of an N-rank
run would replay, bin-packed on shard.doc_costs, runs, reports itself as that share, and its documents replay
without error. The N > 1 path itself (shard / gather over a process group) is tests/test_distributed.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("assign", ["uniform", "cost"])
def test_bench_share_of_a_strong_run(assign):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "3", "--docs", "96", "--ops-per-doc", "512",
           "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--assign", assign, "--share", "1/4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    c = out["config"]
    assert c["docs_per_node"] == 96
    assert c["docs_rank0"] == 24 if assign == "uniform" else 16 <= c["docs_rank0"] <= 32
    assert c["docs_in_error_rank0"] == 0
    assert "share 1/4" in c["parallelism"] and assign in c["parallelism"]
    assert out["value"] > 0


SMALL = ["--config", "3", "--docs", "96", "--ops-per-doc", "512", "--steps", "2", "--warmup", "1"]


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(extra), capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_bench_prepare_fills_the_workload_cache(tmp_path):
    """--prepare needs no GPU: it writes the workload's cache entry (keyed by the workload and the generator's
    sources) with the values derived from it, and a second call finds that entry instead of writing another."""
    import numpy as np

    from fluidframework_amd import gen
    cache = str(tmp_path / "gen")
    _bench(*SMALL, "--prepare", "--gen-cache", cache)
    entries = os.listdir(cache)
    assert len(entries) == 1 and entries[0].startswith("c3_d96_o512_strong_uniform_r0of1-")
    d = os.path.join(cache, entries[0])
    b = gen.generate(gen.config3(512), ids=np.arange(96))
    assert np.array_equal(np.load(os.path.join(d, "ops.npy")), b.ops)
    assert np.array_equal(np.load(os.path.join(d, "op_off.npy")), b.op_off)
    assert int(np.load(os.path.join(d, "local_events.npy"))[0]) == int(((b.ops["kind"] & 0x80) != 0).sum())
    stamp = os.path.getmtime(os.path.join(d, "ops.npy"))
    _bench(*SMALL, "--prepare", "--gen-cache", cache)
    assert os.listdir(cache) == entries and os.path.getmtime(os.path.join(d, "ops.npy")) == stamp


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain run measures the headline figure only (cpu_baseline and end_to_end are null) and --dump-outputs
    saves the last timed step's per-document results as float64: the digests are the oracle's for the same logs,
    and a run from the cached workload dumps the same arrays."""
    import numpy as np

    import oracle_client as oc
    from fluidframework_amd import gen
    cache = str(tmp_path / "gen")
    _bench(*SMALL, "--prepare", "--gen-cache", cache)
    outs = []
    for run, cache_arg in (("a", cache), ("b", "none")):
        r = _bench(*SMALL, "--gen-cache", cache_arg, "--dump-outputs", str(tmp_path / run))
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["cpu_baseline"] is None and line["end_to_end"] is None
        assert line["config"]["docs_in_error_rank0"] == 0
        outs.append({n: np.load(str(tmp_path / run / (n + ".npy"))) for n in ("digests", "errors", "work")})
        assert all(a.dtype == np.float64 and a.shape[0] == 96 for a in outs[-1].values())
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n]), n
    b = gen.generate(gen.config3(512), ids=np.arange(96))
    _, odig, oerr = oc.replay_batch(b, threads=4)
    assert (oerr == 0).all() and (outs[0]["errors"][:, 0] == 0).all()  # column 1 is the failing event (-1: none)
    d = outs[0]["digests"].astype(np.uint64)
    assert np.array_equal((d[:, 0] << np.uint64(32)) | d[:, 1], odig)
    assert outs[0]["work"][:, 0].sum() == 96 * 512  # every sequenced message applied


@pytest.mark.gpu
def test_bench_full_adds_the_cpu_baseline_and_the_end_to_end_runs():
    line = json.loads(_bench(*SMALL, "--gen-cache", "none", "--full").stdout.strip().splitlines()[-1])
    assert line["cpu_baseline"]["value"] > 0 and "digests match GPU: True" in line["cpu_baseline"]["sample"]
    modes = line["end_to_end"]["modes"]
    assert sorted(modes) == ["overlapped", "pinned", "serial"] and all(m["digests_equal"] for m in modes.values())


@pytest.mark.gpu
def test_bench_two_rank_rehearsal_on_one_gpu():
    """The multi-rank path of bench.py end to end on real hardware: torch.distributed.run with two ranks, both on
    device 0 with gloo collectives (--rehearse): the node's documents bin-packed over the ranks, the barriers, the
    max-reduced interval, the summed work and the digest all-gather. RCCL itself needs one GPU per rank (the driver's
    8-GPU runs); this rehearses everything around it."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse",
           "--config", "3", "--docs", "96", "--ops-per-doc", "512", "--steps", "1", "--warmup", "0",
           "--no-cpu-baseline", "--no-e2e"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    c = out["config"]
    assert out["n_gpus"] == 2 and c["docs_per_node"] == 96 and c["docs_rank0"] == 48
    assert c["docs_in_error_rank0"] == 0 and "REHEARSAL" in c["parallelism"]
    assert out["value"] > 0
