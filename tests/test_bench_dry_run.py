"""bench.py's own control flow for N > 1 on CPU: `bench.py --gpus 2 --dry-run-cpu` under gloo with the
CPU emulation of the device phases named through VOXELS_HIP_LIBRARY (the script itself never refers to it) - rank
bookkeeping, the transport negotiation (the emulation has no RCCL: the torch.distributed fallback and what the line says
about it), the halo exchange, the timed loop with its barriers and MAX over ranks, the digest all-reduce, the coarse
levels on rank 0 (CoarseLevels) and the JSON line - so that the first launch on a real 8-GPU node cannot die in Python
nobody ran.  The numbers of such a line mean nothing; its structure and its self-check do."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from emu_lib import emu_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("axis,port", [("y", "29621"), ("z", "29623")])
def test_bench_two_ranks_on_cpu(axis, port):
    from voxels_amd import build
    emu_library()  # (built; the path goes to the ranks through the environment)
    path = build.build_emu()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="2", OMP_NUM_THREADS="2", VOXELS_HIP_LIBRARY=path)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--n", "128", "--levels", "3",
           "--slab-axis", axis, "--dry-run-cpu", "--full", "--no-cpu-baseline", "--no-extra", "--no-isolated"]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=900) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, se[-3000:])
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and not [l for l in outs[1][0].splitlines() if l.startswith("{")], "rank 0 prints ONE JSON line, rank 1 none"
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1 and line["scaling"] == "strong"
    cfg = line["config"]
    assert cfg["multi_gpu_check"] == "equal"
    assert cfg["halo_transport"] == "torch-distributed" and cfg["c_abi_rccl_error"], "the emulation has no RCCL: the fallback transport, and the line says so"
    detail = cfg["multi_gpu_check_detail"]
    # 128^3 on two ranks: the slabs run the levels 0..2, level 3 (one block across both slabs) is rank 0's
    assert detail["coarse_levels"]["levels"] == [3, 4] and len(detail["totals_per_level_blocks_verts_indices_tverts_tindices"]) == 4
    assert line["dry_run"] is True


def _levels(rng, sizes):
    from voxels_amd.binding import BLOCK_INFO_DTYPE, VERTEX_DTYPE, Level
    out = []
    for nb, nv, ni in sizes:
        infos = np.zeros(nb, BLOCK_INFO_DTYPE)
        infos["id"] = rng.randint(0, 1 << 31, nb)
        infos["n_tverts"] = rng.randint(0, 1 << 20, (nb, 6))
        infos["min_corner"] = rng.standard_normal((nb, 3))
        verts = np.zeros(nv, VERTEX_DTYPE)
        verts.view(np.uint8).reshape(nv, 48)[:, 40:] = rng.randint(0, 256, (nv, 8))
        for f, c in (("pos", 3), ("sec", 4), ("nrm", 3)):
            verts[f] = rng.standard_normal((nv, c))
        idx = rng.randint(0, 1 << 32, ni, dtype=np.uint64).astype(np.uint32)
        out.append(Level(infos, verts, idx, verts[: nv // 3].copy(), idx[: ni // 5].copy()))
    return out


def test_dump_outputs_is_exact_and_keeps_to_its_budget(tmp_path):
    """bench.py --dump-outputs' writer: every array as float32 / float64 columns that give back the exact values, whole when it
    all fits, else the block infos whole and the same seeded sample of every other array's rows (with their row numbers),
    within the budget and the same from call to call."""
    sys.path.insert(0, ROOT)
    import bench
    levels = _levels(np.random.RandomState(3), [(50, 4000, 9000), (20, 1500, 4000), (0, 0, 0)])

    def load(d):
        return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}

    def same(got, a):
        """`got` (as written) holds exactly the values of `a`, one row per element, its fields' components as columns."""
        want = a.astype(np.float64) if a.dtype.names is None else \
            np.concatenate([a[f].reshape(len(a), int(np.prod(a.dtype[f].shape))).astype(np.float64) for f in a.dtype.names], axis=1)
        return got.dtype in (np.float32, np.float64) and got.shape == want.shape and np.array_equal(got.astype(np.float64), want)
    bench.dump_outputs(str(tmp_path), levels)
    whole = load(str(tmp_path))
    assert np.array_equal(whole["counts"], [[50, 4000, 9000, 1333, 1800], [20, 1500, 4000, 500, 800], [0] * 5])
    for l, lv in enumerate(levels):
        for what in ("infos", "verts", "idx", "tverts", "tidx"):
            a = getattr(lv, what)
            # an array without elements is only its zero in counts.npy: every file written holds values
            assert same(whole["L%d_%s" % (l, what)], a) if len(a) else "L%d_%s" % (l, what) not in whole, (l, what)
    assert all(len(v) for v in whole.values())
    budget = 200000
    runs = []
    for k in range(2):
        d = tmp_path / ("sampled%d" % k)
        written = bench.dump_outputs(str(d), levels, budget=budget)
        assert written == sum(os.path.getsize(os.path.join(str(d), f)) for f in os.listdir(str(d))) <= budget
        runs.append(load(str(d)))
    assert runs[0].keys() == runs[1].keys() and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
    got = runs[0]
    assert same(got["L0_infos"], levels[0].infos) and same(got["L1_infos"], levels[1].infos)  # (the block infos whole)
    for l, lv in enumerate(levels[:2]):
        for what in ("verts", "idx", "tverts", "tidx"):
            rows = got["L%d_%s_rows" % (l, what)].astype(np.int64)
            assert 0 < len(rows) < len(getattr(lv, what)) and np.all(np.diff(rows) > 0)
            assert same(got["L%d_%s" % (l, what)], getattr(lv, what)[rows]), (l, what)


def test_bench_dump_outputs_on_cpu(tmp_path):
    """`bench.py --dump-outputs DIR` on the two-rank CPU dry run: each rank writes what its last timed step computed, the same
    bytes in a second run with the same arguments, and the ranks' meshes add up to the totals the line's self-check reports."""
    from voxels_amd import build
    path = build.build_emu()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29625", WORLD_SIZE="2", OMP_NUM_THREADS="2", VOXELS_HIP_LIBRARY=path)
    dumps, line = [], None
    for run in range(2):
        d = str(tmp_path / ("run%d" % run))
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "0", "--n", "128", "--levels", "3",
               "--dry-run-cpu", "--full", "--no-cpu-baseline", "--no-extra", "--no-isolated", "--dump-outputs", d]
        procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
        outs = [p.communicate(timeout=900) for p in procs]
        for r, (p, (so, se)) in enumerate(zip(procs, outs)):
            assert p.returncode == 0, "rank %d failed:\n%s" % (r, se[-3000:])
        line = json.loads([l for l in outs[0][0].splitlines() if l.startswith("{")][0])
        assert line["steps"] == 3 and line["dump_outputs"]["dir"] == d
        files = sorted(os.listdir(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
        dumps.append({f: np.load(os.path.join(d, f)) for f in files})
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][f], dumps[1][f]) for f in dumps[0])
    counts = [dumps[0]["rank%d_counts.npy" % r] for r in range(2)]
    for r in range(2):
        assert all(v.dtype in (np.float32, np.float64) for v in dumps[0].values())
        for l in range(len(counts[r])):
            names = ["rank%d_L%d_%s.npy" % (r, l, w) for w in ("infos", "verts", "idx", "tverts", "tidx")]
            assert [len(dumps[0][f]) if f in dumps[0] else 0 for f in names] == counts[r][l].tolist()
            assert all(f in dumps[0] for f, c in zip(names, counts[r][l]) if c)
    assert all(len(v) for v in dumps[0].values()), "every file written holds values"
    totals = line["config"]["multi_gpu_check_detail"]["totals_per_level_blocks_verts_indices_tverts_tindices"]
    assert (counts[0] + counts[1]).tolist() == [[float(x) for x in row] for row in totals[:len(counts[0])]]


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """A plain `bench.py` run (no --full) on one rank: it sets up, warms up, times the steps, writes --dump-outputs and prints
    the line - with the headline's keys and none of the figures --full adds - and what it dumps is what the --full run of the
    same arguments dumps."""
    from voxels_amd import build
    path = build.build_emu()
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", OMP_NUM_THREADS="2", VOXELS_HIP_LIBRARY=path)
    lines, dumps = {}, {}
    for mode in ("plain", "full"):
        d = str(tmp_path / mode)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "128", "--levels", "3",
               "--dry-run-cpu", "--no-cpu-baseline", "--no-extra", "--no-isolated", "--dump-outputs", d] + (["--full"] if mode == "full" else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, "%s run failed:\n%s" % (mode, r.stderr[-3000:])
        found = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(found) == 1, "ONE JSON line"
        lines[mode] = json.loads(found[0])
        dumps[mode] = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    plain, full = lines["plain"], lines["full"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
        assert key in plain, key
    assert plain["metric"] == full["metric"] == "Mvoxels/s polygonized (128^3 grid, 3 LOD levels)"
    assert plain["unit"] == "Mvoxels/s" and plain["higher_is_better"] is True and plain["dtype"] == "i8"
    assert abs(plain["value"] - 128 ** 3 / (plain["ms_per_step"] * 1e-3) / 1e6) < 0.01 * plain["value"]
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["dump_outputs"]["dir"] == str(tmp_path / "plain")
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    assert "roofline" not in plain and "cpu_baseline" not in plain and "parity_vs_reference" not in plain
    for key in ("stage_ms_serialized", "whole_execute", "e2e_ms", "cold", "steady_state_uncached", "edit", "extra", "multi_gpu_check"):
        assert key not in plain["config"], key
    assert "roofline" in full and full["config"]["e2e_ms"] and full["config"]["cold"]
    assert plain["config"]["active_blocks"] == full["config"]["active_blocks"]
    assert dumps["plain"].keys() == dumps["full"].keys() and all(np.array_equal(dumps["plain"][f], dumps["full"][f]) for f in dumps["plain"])
