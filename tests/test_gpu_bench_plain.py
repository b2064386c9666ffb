"""bench.py's plain run on the GPU: it times --steps frames and prints the
headline line only; what else the bench measures waits for --full.  With
--dump-outputs the last timed step's frame and ray count are written, equal to
a render of the same frame through the package in another process (the inputs
are the bundled scene and a fixed seed: the same from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 136, 72, 8    # 17 x 9 tiles of 8 x 8: more than one block, an odd tile count


def test_plain_run_prints_the_headline_and_dumps_its_outputs(mcpt, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--width", str(W), "--height", str(H), "--spp", str(SPP), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(out) == 1, r.stdout
    line = json.loads(out[0])
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement, rays of the 3 steps / their wall time
    # (ms_per_step is rounded to 1e-3 ms; a step of this frame takes more than 0.1 ms)
    assert line["value"] == pytest.approx(line["rays_per_step"] / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    # nothing that takes a run of its own
    for k in ("roofline", "cpu_baseline", "other_pipeline", "extra_lines"):
        assert k not in line
    scene = mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))
    ref, st = scene.render(mcpt.RenderParams(width=W, height=H, spp=SPP, spp_chunk=32, pipeline="wavefront"))
    img = np.load(tmp_path / "out" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (H, W, 4)
    assert np.array_equal(img[..., :3], ref)
    rays = np.load(tmp_path / "out" / "rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [float(st["rays"])] and line["rays_per_step"] == st["rays"]
