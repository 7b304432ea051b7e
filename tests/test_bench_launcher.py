"""bench.py's own launcher (no GPU needed): `python bench.py --gpus N` without a launcher around it must start N ranks through
torch.distributed.run from a parent that never touches the GPU, pass its arguments on, and leave with the child's exit code."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(kw)
    return e


def test_gpus_n_builds_the_torchrun_command():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--dist-backend", "gloo",
                          "--force-device", "0", "--dry-launch"], env=_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    cmd = d["cmd"]
    assert d["would_launch"] == 2 and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0 and BENCH in cmd
    tail = cmd[cmd.index(BENCH) + 1:]
    assert tail == ["--gpus", "2", "--steps", "3", "--warmup", "1", "--dist-backend", "gloo", "--force-device", "0"]


def test_failed_ranks_give_a_nonzero_exit():
    """On a box without a GPU the ranks refuse to run; the self-launching parent must report that, not swallow it."""
    import torch
    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu", "--dist-backend", "gloo",
                          "--force-device", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert "needs an MI355X" in (out.stdout + out.stderr)


def test_a_launched_rank_does_not_relaunch():
    """Under a launcher (WORLD_SIZE set) bench.py is a rank: without a GPU it stops with the GPU message, it never spawns."""
    import torch
    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--no-cpu"], env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "needs an MI355X" in (out.stdout + out.stderr)


def test_pmc_traffic_takes_the_steady_state_step_kernel(tmp_path, monkeypatch):
    """The step kernel shows up in several instantiations in a counter pass (the pipeline's first launch carries only a
    mask pack, the drain's launches only tails and summaries): roofline.traffic quotes the one launched most, and
    nothing at all when the pass ran other kernel sources or another launch size."""
    import json
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    data = {"_meta": {"kernel_source_sha16": "abc", "points_per_launch": 16_000_000},
            "void lpf_step_t<4, 7u, unsigned char, false>": {"launches": 2, "hbm_bytes_per_launch": 38e6},
            "void lpf_step_t<8, 7u, unsigned char, false>": {"launches": 24, "hbm_bytes_per_launch": 516e6},
            "void lpf_step_t<4, 7u, unsigned int, false>": {"launches": 4, "hbm_bytes_per_launch": 9e6},
            "void lpf_k1_project_t<4, 7u, unsigned char>": {"launches": 24, "hbm_bytes_per_launch": 464e6}}
    (prof / bench.PMC_FILE).write_text(json.dumps(data))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_sha", lambda: "abc")
    assert bench.pmc_traffic(16_000_000, "lpf_step_t")[0] == 516e6
    assert bench.pmc_traffic(16_000_000, "lpf_k1_project_t")[0] == 464e6
    assert bench.pmc_traffic(2_000_000, "lpf_step_t")[0] is None
    monkeypatch.setattr(bench, "kernel_source_sha", lambda: "other")
    got, why = bench.pmc_traffic(16_000_000, "lpf_step_t")
    assert got is None and "re-run" in why


def _fake_step_outputs(F, n, M, B, seed=0):
    """outputs of one step as bench.make_outputs lays them out, filled as a finished step would fill them"""
    import numpy as np
    import torch
    from lidar_object_detection_amd._native import SUMMARY_DTYPE
    rng = np.random.default_rng(seed)
    sm = np.zeros(F, SUMMARY_DTYPE)
    valid = np.full(F * n, -7, np.int64)                       # -7: what lies beyond a frame's lists (never part of the output)
    inst = np.full(F * n, -7, np.int64)
    for f in range(F):
        nv = int(rng.integers(0, n))
        sm[f]["n_valid"] = nv
        valid[f * n:f * n + nv] = np.sort(rng.choice(n, nv, replace=False))
        cnt = rng.integers(0, n // (2 * M), M)
        sm[f]["inst_count"][:M] = cnt
        sm[f]["inst_off"][:M + 1] = np.concatenate([[0], np.cumsum(cnt)])
        inst[f * n:f * n + int(cnt.sum())] = rng.integers(0, n, int(cnt.sum()))
        sm[f]["best_box"][:M] = rng.integers(-1, B, M)
        sm[f]["best_cnt"][:M] = rng.integers(0, 50, M)
        sm[f]["n_labelled"] = int(rng.integers(1, n))
    uv = rng.integers(-2**31, 2**31, (F * n, 2), dtype=np.int64).astype(np.int32)
    lab = rng.integers(-2**31, 2**31, F * n, dtype=np.int64).astype(np.int32)
    return dict(uv=torch.from_numpy(uv), label_bits=torch.from_numpy(lab), valid_idx=torch.from_numpy(valid),
                inst_idx=torch.from_numpy(inst), count_mb=torch.from_numpy(rng.integers(0, 99, M * F * B).astype(np.int32)),
                summary=torch.from_numpy(np.frombuffer(sm.tobytes(), np.uint8).copy())), sm


def test_dump_outputs_writes_the_step_outputs(tmp_path, monkeypatch):
    """--dump-outputs (no GPU needed for the writer): float64 .npy files under the size limit, the same positions every time,
    sampled values equal to the outputs at those positions, nothing from beyond a frame's lists, full-array sums per frame."""
    import numpy as np
    import torch
    import bench
    F, n, M, B = 3, 5000, 4, 6
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    out, sm = _fake_step_outputs(F, n, M, B)
    bench.dump_outputs(torch, out, F, n, M, str(tmp_path / "a"))
    bench.dump_outputs(torch, out, F, n, M, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and all(x.endswith(".npy") for x in names)
    d = {x[:-4]: np.load(tmp_path / "a" / x) for x in names}
    for k, v in d.items():
        assert v.dtype == np.float64, k
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    uv, lab = out["uv"].numpy(), out["label_bits"].numpy().view(np.uint32)
    assert all(v.any() for v in d.values()), [k for k, v in d.items() if not v.any()]    # nothing in it is a constant zero
    assert not any(k.endswith("_pos") or k == "inst_overflow" for k in d)               # computed outputs only
    pos = bench.dump_sample_positions(F * n, "point")
    assert len(pos) == 1000 and np.all(np.diff(pos) > 0)
    assert np.array_equal(d["u_sample"], uv[pos, 0]) and np.array_equal(d["v_sample"], uv[pos, 1])
    assert np.array_equal(d["label_bits_sample"], lab[pos])
    valid = np.concatenate([out["valid_idx"].numpy()[f * n:f * n + sm[f]["n_valid"]] for f in range(F)])
    assert np.array_equal(d["valid_idx_sample"], valid[bench.dump_sample_positions(len(valid), "valid_idx")])
    inst = out["inst_idx"].numpy()
    lists = [inst[f * n + sm[f]["inst_off"][m]:f * n + sm[f]["inst_off"][m + 1]] for f in range(F) for m in range(M)]
    assert np.array_equal(d["inst_idx_sample"], np.concatenate(lists)[bench.dump_sample_positions(sum(map(len, lists)), "inst_idx")])
    assert -7 not in d["valid_idx_sample"] and -7 not in d["inst_idx_sample"]
    assert np.array_equal(d["frame_sum_u"], uv[:, 0].reshape(F, n).astype(np.int64).sum(1))
    assert np.array_equal(d["frame_sum_label_bits"], lab.reshape(F, n).astype(np.int64).sum(1))
    assert np.array_equal(d["frame_sum_valid_idx"], [valid_f.sum() for valid_f in np.split(valid, np.cumsum(sm["n_valid"])[:-1])])
    assert np.array_equal(d["n_valid"], sm["n_valid"]) and np.array_equal(d["inst_off"], sm["inst_off"][:, :M + 1])
    assert np.array_equal(d["best_box"], sm["best_box"][:, :M]) and np.array_equal(d["count_mb"], out["count_mb"].numpy())


def test_dump_outputs_refuses_overflowed_lists(tmp_path):
    """A step whose instance lists overflowed has no complete outputs: --dump-outputs stops instead of writing part of them."""
    import numpy as np
    import pytest
    import torch
    import bench
    from lidar_object_detection_amd._native import SUMMARY_DTYPE
    out, sm = _fake_step_outputs(2, 3000, 4, 5)
    sm[1]["inst_overflow"] = 1
    out["summary"] = torch.from_numpy(np.frombuffer(sm.tobytes(), np.uint8).copy())
    assert sm.dtype == SUMMARY_DTYPE
    with pytest.raises(SystemExit, match="overflowed"):
        bench.dump_outputs(torch, out, 2, 3000, 4, str(tmp_path / "d"))
    assert not os.path.exists(tmp_path / "d") or not os.listdir(tmp_path / "d")
