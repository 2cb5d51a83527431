"""Guards the driver-facing contracts: bench.py's JSON line (the CI
driver parses these exact fields), the static web client's JS syntax,
and the pipeline-depth interface on the CPU tier."""

import json
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def test_bench_json_contract():
    """`python bench.py --cpu --steps 2` emits one JSON line with every
    field the driver consumes, with sane values."""
    p = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--cpu", "--steps", "2",
         "--warmup", "1", "--width", "320", "--height", "192"],
        capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    line = [l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in d, f"missing driver field {key}"
    assert d["metric"] == "encoded_fps_1080p60_h264"
    assert d["n_gpus"] == 1 and d["steps"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["data"] == "synthetic" and d["value"] > 0
    cfg = d["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism",
                "resolution", "latency_p50_ms", "latency_p95_ms"):
        assert key in cfg, f"missing config field {key}"
    assert cfg["resolution"] == "320x192"


BENCH_CPU = [sys.executable, str(REPO / "bench.py"), "--cpu", "--steps", "3",
             "--warmup", "1", "--width", "320", "--height", "192"]


def _bench_dump(out_dir, *extra):
    p = subprocess.run(BENCH_CPU + ["--dump-outputs", str(out_dir), *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    d = json.loads([l for l in p.stdout.strip().splitlines()
                    if l.startswith("{")][-1])
    import numpy as np
    return d, {f.stem: np.load(f) for f in sorted(out_dir.glob("*.npy"))}


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes the last timed frame's stripes as float
    .npy; the same arguments give the same outputs run to run, and
    --full changes neither the result line's fields nor the outputs."""
    import numpy as np
    d1, a = _bench_dump(tmp_path / "a")
    d2, b = _bench_dump(tmp_path / "b", "--full")
    assert set(a) == set(b) == {"bitstream", "stripes", "frame_id"}
    assert set(d1) == set(d2) and d1["steps"] == d2["steps"] == 3
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert np.array_equal(a[name], b[name]), name
    # warmup encodes frames 0..1, the 3 timed steps frames 2..4
    assert a["frame_id"].tolist() == [4.0]
    st = a["stripes"]
    assert st[:, 0].tolist() == [0.0, 64.0, 128.0]      # 192 rows / 64
    assert st[:, 1].tolist() == np.concatenate(
        [[0], np.cumsum(st[:-1, 2])]).tolist()
    bits = a["bitstream"]
    assert bits.size == int(st[:, 2].sum()) and bits.size > 0
    assert bits.min() >= 0 and bits.max() <= 255
    assert np.array_equal(bits, np.round(bits))
    # every stripe is an Annex-B stream: starts with a start code
    for off in st[:, 1].astype(int):
        assert bits[off:off + 3].tolist() in ([0, 0, 1], [0, 0, 0])


def test_bench_dump_outputs_budget(tmp_path):
    """An output past the byte budget is cut to a fixed seeded sample
    that fits it, with the sampled positions alongside."""
    import numpy as np
    sys.path.insert(0, str(REPO))
    import bench
    rng = np.random.default_rng(5)
    stripes = [(y, rng.integers(0, 256, 40000, dtype=np.uint8).tobytes())
               for y in (0, 64)]
    budget = 100_000
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), (7, stripes), budget=budget)
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= budget
    a = {f.stem: np.load(f) for f in files}
    idx = a["bitstream_index"].astype(int)
    assert 0 < idx.size < 80000 and np.all(np.diff(idx) > 0)
    raw = np.frombuffer(b"".join(p for _, p in stripes), dtype=np.uint8)
    assert np.array_equal(a["bitstream"], raw[idx].astype(np.float32))
    for f in files:
        assert np.array_equal(np.load(f), np.load(tmp_path / "b" / f.name))


node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node not available")
def test_web_client_js_syntax():
    """Every shipped static JS file parses (node --check)."""
    web = REPO / "selkies_amd" / "web"
    files = sorted(web.glob("*.js"))
    assert files
    for f in files:
        p = subprocess.run([node, "--check", str(f)],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, f"{f.name}: {p.stderr}"


def test_cpu_pipeline_ignores_depth():
    """pipeline_depth is a HIP-pipeline feature; the CPU pipelines take
    the same interface but stay synchronous — same outputs, flush is a
    no-op."""
    hipflux = pytest.importorskip("hipflux")
    if not hipflux.native_available():
        pytest.skip("native module not built")
    import numpy as np
    from hipflux import _native
    rng = np.random.default_rng(3)
    frames = [np.ascontiguousarray(
        rng.integers(0, 256, (128, 192, 4), dtype=np.uint8))
        for _ in range(4)]
    a = _native._pipeline_encode("cpu", frames, 192, 128, 26, 64, 1)
    b = _native._pipeline_encode("cpu", frames, 192, 128, 26, 64, 1,
                                 pipeline_depth=2)
    assert len(a) == len(b) == 4
    for fa, fb in zip(a, b):
        assert [(bytes(d), y) for d, y, *_ in fa] == \
               [(bytes(d), y) for d, y, *_ in fb]
