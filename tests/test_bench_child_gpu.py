"""bench.py run the way the driver runs it — a child process, the launcher's own rank children — on one GPU: `--gpus 2 --shared-gpu`
is the dry run of the N-rank line (ranks share GPU 0, exchange staged through gloo), `--cpu-full` the full-size parity leg at a size
the oracle finishes in seconds. First contact of `python bench.py --gpus N` must not be the 8-GPU box. A plain run carries the headline
figure alone; the legs beside the timed steps are asked for with `--full`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("config", ["cfg3", "cfg2", "merge"])
def test_two_rank_line_through_the_launcher(config):
    out = _run("--full", "--gpus", "2", "--shared-gpu", "--config", config, "--reads", "20000", "--steps", "1", "--warmup", "0",
               "--cpu-sample-reads", "2000", "--launch-timeout", "600")
    assert out["n_gpus"] == 2 and out["steps"] == 1 and out["scaling"] == "weak" and out["value"] > 0
    assert out["roofline"] and out["roofline"]["bound"] == "hbm" and out["roofline"]["kernels"]
    assert out["exchange"] and out["exchange"]["world_size"] == 2
    if config == "merge":
        assert out["merge"]["words_union"] <= out["merge"]["words_self"] + out["merge"]["words_other"]
    else:
        assert out["cpu_baseline"] and out["cpu_baseline"]["cores"] == 1 and out["cpu_baseline"]["value"] > 0
        k = 31
        assert out["distinct_kmers_in_index"] <= 2 * 20000 * (150 - k + 1)
        assert all(s > 0 for s in out["exchange"]["sent_bytes_per_rank_step"])
        # the line carries its own denominator: the same configuration on one GPU (rank 0's share, built directly after the timed steps) ...
        one = out["one_gpu_same_config"]
        assert one["value"] > 0 and one["ms_per_step"] > 0 and abs(out["scaling_vs_one_gpu_same_config"] - out["value"] / one["value"]) < 0.01
        # ... and says what crossed the links: the library's choice at two ranks is "replicate" (one link per pair of GPUs bounds every protocol
        # that ships words: the reads cross as bit planes instead)
        assert out["exchange"]["protocol_asked"] == "auto" and out["exchange"]["protocol"] == "replicate"
        # ... and carries its own correctness verdict: the sharded index against every rank's word stream (count, set checksum, structure, every
        # inserted k-mer found in exactly one share), and the CPU leg's sample rebuilt on the GPU with the oracle's bytes
        sc = out["set_check"]
        assert sc["ok"] is True and sc["validate_violations"] == 0 and sc["members_ok"] is True and sc["members_found"] == sc["kmers_inserted"] == 2 * 20000 * (150 - k + 1)
        assert sc["count"] == out["distinct_kmers_in_index"] and sc["repeats_implied"] == sc["kmers_inserted"] - sc["count"] >= 0
        assert sc["repeats_implied"] != 0 or (sc["checksums_equal"] is True and sc["checksum_index"] == sc["checksum_word_streams"])
        ps = out["parity_sample"]
        assert ps["equal"] is True and ps["sha256"] == ps["sha256_oracle"] and ps["bytes"] == ps["bytes_oracle"] > 0 and ps["reads"] == 2000 and ps["first_difference_at"] is None
    # an algorithmic rate above the HBM peak is a bookkeeping error (bench.py asserts it too)
    assert all(r["frac"] is None or r["frac"] <= 1.0 for r in out["roofline"]["kernels"])


# what a leg beside the timed steps puts on the line: a plain run has none of them
SIDE_LEGS = ("parity_sample", "parity_full_size", "set_check", "sharded_overhead", "one_gpu_same_config", "scaling_vs_one_gpu_same_config",
             "serialize", "fasta_inclusive", "per_record")


def test_plain_line_is_the_headline_figure_alone():
    """Without `--full` a run times its steps and prints the line: the headline keys mean what they always did, the figures the timed steps
    leave behind (roofline, count) are there, and no leg that takes a run of its own has run. `--full` brings them back."""
    argv = ("--gpus", "1", "--config", "cfg2", "--reads", "40000", "--steps", "2", "--warmup", "1")
    out = _run(*argv)
    assert out["metric"] == "k-mers inserted/sec (build index)" and out["unit"] == "k-mers/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
    assert (out["n_gpus"], out["steps"], out["warmup"]) == (1, 2, 1) and out["ms_per_step"] > 0
    # value = k-mers of a step / time of a step (ms_per_step is rounded to a microsecond: well within 1 % at this size)
    assert abs(out["value"] - 40000 * 120 / (out["ms_per_step"] * 1e-3)) <= 0.01 * out["value"]
    assert 0 < out["distinct_kmers_in_index"] <= 40000 * 120
    assert out["roofline"] and out["roofline"]["kernels"] and "roofline_error" not in out
    assert out["cpu_baseline"] is None and out["h2d_inclusive"] is None and out["value_h2d_inclusive"] is None and out["exchange"] is None
    assert not [k for k in SIDE_LEGS if k in out]
    full = _run(*argv, "--full", "--cpu-sample-reads", "5000", "--no-h2d")
    assert full["cpu_baseline"]["value"] > 0 and full["serialize"]["bytes"] > 0 and full["parity_sample"]["equal"] is True
    same = ("metric", "unit", "higher_is_better", "dtype", "config", "distinct_kmers_in_index")
    assert {k: full[k] for k in same} == {k: out[k] for k in same}


def test_default_line_carries_parity_sample():
    """The N = 1 line of a `--full` run: the CPU leg's sample is built once more on the GPU after the timed region and byte-compared with the oracle's index of it."""
    out = _run("--full", "--config", "cfg2", "--reads", "40000", "--steps", "1", "--warmup", "0", "--cpu-sample-reads", "5000", "--no-h2d")
    ps = out["parity_sample"]
    assert ps["equal"] is True and ps["reads"] == 5000 and ps["sha256"] == ps["sha256_oracle"] and ps["bytes"] == ps["bytes_oracle"] > 0
    assert ps["distinct_kmers"] == ps["distinct_kmers_oracle"] <= 5000 * 120
    assert "set_check" not in out and "roofline_error" not in out


def test_launcher_reports_a_failing_rank():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    # K = 32 is not a supported word layout: every rank fails after the rendezvous; the launcher must come back non-zero, promptly
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--shared-gpu", "--reads", "2000", "--k", "32", "--steps", "1",
                        "--warmup", "0", "--no-cpu-baseline", "--launch-timeout", "300"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_full_size_parity_leg_at_a_small_size():
    out = _run("--full", "--config", "cfg2", "--reads", "30000", "--steps", "1", "--warmup", "0", "--cpu-full", "--no-h2d")
    p = out["parity_full_size"]
    assert p["equal"] is True and p["sha256"] == p["sha256_oracle"] and p["bytes"] == p["bytes_oracle"] > 0
    assert p["distinct_kmers"] == p["distinct_kmers_oracle"] == out["distinct_kmers_in_index"]
    assert p["first_difference_at"] is None


def test_full_size_parity_leg_of_the_merge_at_a_small_size():
    """`--config merge --cpu-full`: the oracle builds both operands, merges them, and BOTH resulting indexes are byte-compared (the merged one
    and other, whose Vec buckets the merge sorted); the CPU baseline of that line is the oracle's merge."""
    out = _run("--full", "--config", "merge", "--reads", "30000", "--steps", "2", "--warmup", "1", "--cpu-full", "--no-h2d")
    p = out["parity_full_size"]
    assert p["equal"] is True and p["sha256"] == p["sha256_oracle"] and p["bytes"] == p["bytes_oracle"] > 0
    o = p["other_after_merge"]
    assert o["equal"] is True and o["sha256"] == o["sha256_oracle"] and 0 < o["bytes"] < p["bytes"]
    assert p["distinct_kmers"] == p["distinct_kmers_oracle"] == out["merge"]["words_union"]
    assert out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["value"] > 0 and "merge" in out["cpu_baseline"]["sample"]


def test_dump_outputs_is_the_timed_index_and_repeats(tmp_path):
    """`--dump-outputs DIR`: the index the last timed step left, as .npy files; the same arguments give the same files."""
    import numpy as np

    argv = ("--config", "cfg2", "--reads", "20000", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-h2d", "--no-serialize")
    outs = [_run(*argv, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    assert all(o["steps"] == 2 and o["ms_per_step"] > 0 for o in outs)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(n + ".npy" for n in outs[0]["dump_outputs"]["arrays"]) == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    count, nbuckets, nbytes = np.load(tmp_path / "a" / "summary.npy").tolist()
    assert count == outs[0]["distinct_kmers_in_index"] > 0 and nbuckets > 0 and nbytes > 0
