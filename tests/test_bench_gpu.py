"""GPU: a plain `python bench.py --gpus 1` run does only what its headline needs (set up, warm up, time, print); what takes runs of
its own (in-run PMC passes, tokenizer / renderer rooflines, zero-tail cross-attention, wall-clock per video, CPU baseline) is --full only."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

FULL_ONLY = ("roofline_tokenizer", "roofline_render", "roofline_extras_error", "cross_attention_zero_tail", "video_wallclock", "cpu_baseline")


def test_plain_bench_run_prints_the_headline_without_the_full_extras(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--blocks", "4", "--latent", "8,32,48",
           "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["unit"] == "denoise-steps/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert (out["steps"], out["warmup"]) == (2, 1) and out["value"] > 0 and out["ms_per_step"] > 0 and out["output_finite"]
    assert abs(out["value"] * out["ms_per_step"] - 1e3) < 1e3 * 1e-2
    # from the timed steps' own hipEvent pairs (self-attention over 8 x 16 x 24 = 3 072 tokens: above the 2 048-key cut of `roofline`)
    assert out["roofline"]["launches"] > 0 and out["roofline_gemm"]["launches"] > 0
    for key in FULL_ONLY:
        assert key not in out, key
    assert "not run in this invocation" in out["outside_timed_region"]
    assert (tmp_path / "dump" / "latent.npy").exists() and out["dumped_outputs"]["arrays"]["latent"]["shape"] == [1, 16, 8, 32, 48]
