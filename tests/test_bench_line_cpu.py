"""bench.py's driver-facing line: short (< 4 KB), strict JSON, carries the contract's keys; `roofline.traffic` comes from the
PMC summaries committed under profiles/, not from a typed constant (BENCH_r04 `parsed` was null)."""
import json
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")
ROOF = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "launch_ms")


def _canned():
    """a full `result` as main() builds it: the largest one committed (20 KB as a line) + a few hostile additions"""
    with open(os.path.join(ROOT, "profiles", "r04b_default_bench.json")) as f:
        r = json.load(f)
    r["config"]["workload"] = "NS: 40 views x 256 ch x 480x640 fp32 maps (channels_last) -> grid 192x192x192, N=300"
    r["config"]["scenes_per_step"] = r["scenes_per_step"]
    r["kernels"]["x" * 300] = dict(ms_per_scene=1.0)
    r["conv_layers"] = r["conv_layers"] * 4
    r["train_S"] = dict(value=40.0, ms_per_step=25.0, note="n" * 5000)
    r["A"] = dict(value=240.0, ms_per_step=100.0, graph_nodes_per_scene=290, n_classes=17, n_reg_outs=8, workload="A" * 400,
                  windows_scenes_per_s=[240.0, 241.0, 239.0])
    r["dist"] = dict(world_size=8, backend="nccl", rank=0, per_rank_window_s=[[2.0] * 8] * 3)
    return r


def test_line_is_short_strict_json_with_the_contract_keys():
    r = _canned()
    text = bench.compact_line(r)
    assert len(text) < 4096 and "\n" not in text
    line = json.loads(text)
    for k in CONTRACT:
        assert k in line, k
    assert line["value"] == pytest.approx(r["value"], rel=1e-3)
    assert line["unit"] == "scenes/s" and line["higher_is_better"] is True and line["scaling"] == "weak"
    for roof in (line["roofline"], line["S"]["roofline"]):
        assert tuple(roof) == ROOF
        assert roof["bound"] in ("hbm", "mfma") and roof["unit"] in ("GB/s", "TFLOP/s")
        assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=2e-3)
    cb = line["cpu_baseline"]
    assert set(cb) >= {"value", "unit", "cores", "kind", "sample"} and cb["kind"] in ("port", "reference")
    assert len(cb["sample"]) <= 200
    assert isinstance(line["config"]["workload"], str) and len(line["config"]["workload"]) < 300
    assert "model" not in line["config"]
    for k in ("kernels", "conv_layers", "stage_ms"):
        assert k not in line and k not in line["S"]
    assert line["through_plugin"]["value"] and line["nchw_input"]["value"] and line["value_f32_conv"]
    assert line["A"] == dict(value=240.0, ms_per_step=100.0, graph_nodes_per_scene=290, n_reg_outs=8)      # BASELINE configs[2]
    assert line["detail"] == bench.DETAIL_NAME


def test_line_never_exceeds_the_limit_even_with_oversized_fields():
    r = _canned()
    r["config"]["workload"] = "w" * 3000
    r["config"]["level_rows"] = list(range(400))
    text = bench.compact_line(r)
    assert len(text) < 4096
    json.loads(text)


def test_nan_is_refused_not_printed():
    r = _canned()
    r["value"] = float("nan")
    with pytest.raises(ValueError):
        bench.compact_line(r)


def test_line_without_secondary_blocks():
    r = _canned()
    for k in ("S", "through_plugin", "nchw_input", "f32_conv", "value_f32_conv", "cpu_baseline", "dist", "train_S"):
        r.pop(k, None)
    line = json.loads(bench.compact_line(r))
    assert line["cpu_baseline"] is None and "S" not in line


def test_emit_writes_detail_and_prints_one_line(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    r = _canned()
    bench.emit(r)
    out = capsys.readouterr().out
    assert out.endswith("\n") and out.count("\n") == 1
    json.loads(out)
    with open(tmp_path / bench.DETAIL_NAME) as f:
        detail = json.load(f)
    assert "kernels" in detail and "conv_layers" in detail and detail["S"]["kernels"]


def test_roofline_traffic_is_read_from_the_committed_pmc_passes():
    import csv
    for wl in ("NS", "S"):
        for fam in ("dense", "conv"):
            got = bench.pmc_traffic(wl, fam)
            assert got is not None, (wl, fam, bench.PMC_TAG)
            total, src = got
            assert f"profiles/{bench.PMC_TAG}_{wl.lower()}_pmc_FETCH_SIZE.csv" in src
            # recompute by hand from the two files
            want = 0.0
            for counter, mult in (("FETCH_SIZE", 2.0), ("WRITE_SIZE", 1.0)):
                kb = n = 0
                with open(os.path.join(ROOT, "profiles", f"{bench.PMC_TAG}_{wl.lower()}_pmc_{counter}.csv"), newline="") as f:
                    for row in csv.DictReader(f):
                        if any(k in row["Kernel_Name"] for k in bench.PMC_KERNELS[fam]):
                            kb += float(row["Sum"])
                            n += int(row["Dispatches"])
                want += mult * kb * 1024 / n
            assert total == pytest.approx(want, rel=1e-12)
    # the dense kernel at NS: ~60 GB per launch against 19.86 GB algorithmic
    assert 40e9 < bench.pmc_traffic("NS", "dense")[0] < 80e9
    assert bench.pmc_traffic("NS", "dense", tag="no_such_round") is None


def _graph_workload(batch=False, bad=0):
    """what dump_outputs() reads of a graph-path workload after its last step: 2 scenes, 2 levels of 4 + 3 padded rows in
    the step buffers; the slot is a real StaticScene / StaticBatch (its detections() picks the live rows), its outputs
    hold another scene's block"""
    import types
    import torch
    from cnrma_amd import pipeline
    det = torch.full((2, 7, 6 + 18), float("nan"))
    for j in range(2):
        for r in range(7):
            det[j, r] = 100 * j + r + torch.arange(24) / 100
    valid = torch.tensor([[2, 1], [0, 3]], dtype=torch.int32)
    B = 2 if batch else 1
    out = dict(sizes=[4, 3], n_levels=2, status=torch.zeros(1, dtype=torch.int32), done=None,
               counts=torch.zeros(2 * B + B + 2 * 2 * B if batch else 7, dtype=torch.int32),
               bboxes=torch.zeros((B, 7, 6) if batch else (7, 6)), scores=torch.zeros((B, 7, 18) if batch else (7, 18)),
               valid=torch.zeros((B, 2) if batch else (2,), dtype=torch.int32))
    if batch:
        slot = object.__new__(pipeline.StaticBatch)
        slot.B, slot.device = B, torch.device("cpu")
    else:
        slot = object.__new__(pipeline.StaticScene)
    slot.out = out
    return types.SimpleNamespace(torch=torch, plugin=False, args=types.SimpleNamespace(eager=False), det=det, det_valid=valid,
                                 box_w=6, slots=[slot], sps=2, B=B, violations=lambda: bad)


@pytest.fixture
def cpu_readback(monkeypatch):
    """the dump on the CPU: no device to synchronise, host reads straight from the tensor"""
    import torch
    from cnrma_amd import _lib
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "read_ints", lambda t: t.reshape(-1).tolist())


@pytest.mark.parametrize("batch", [False, True])
def test_dump_outputs_writes_the_live_rows_of_the_last_step(tmp_path, cpu_readback, batch):
    import numpy as np
    wl = _graph_workload(batch)
    bench.dump_outputs(wl, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["bboxes.npy", "rows.npy", "scores.npy"]
    b, s, rows = (np.load(tmp_path / "out" / f"{k}.npy") for k in ("bboxes", "scores", "rows"))
    assert b.dtype == s.dtype == np.float32 and rows.dtype == np.float64
    assert rows.tolist() == [[2, 1], [0, 3]] and b.shape == (6, 6) and s.shape == (6, 18)
    live = [(0, 0), (0, 1), (0, 4), (1, 4), (1, 5), (1, 6)]            # (scene, padded row): level 0 at row 0, level 1 at row 4
    want = np.stack([wl.det[j, r].numpy() for j, r in live])
    assert np.array_equal(b, want[:, :6]) and np.array_equal(s, want[:, 6:])


def test_dump_outputs_keeps_the_first_scenes_within_the_size_limit(tmp_path, cpu_readback, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 24 * 4 + 16 + 1)     # scene 0 (3 rows) fits, scene 1 does not
    bench.dump_outputs(_graph_workload(), str(tmp_path / "out"))
    assert np.load(tmp_path / "out" / "rows.npy").tolist() == [[2, 1]]
    assert np.load(tmp_path / "out" / "bboxes.npy").shape == (3, 6)


def test_dump_outputs_refuses_a_run_that_violated_the_plan(tmp_path, cpu_readback):
    with pytest.raises(RuntimeError, match="violation"):
        bench.dump_outputs(_graph_workload(bad=1), str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
