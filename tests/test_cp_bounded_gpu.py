"""GPU: a DiT denoise step under the three key-sharding context-parallel schedules with the logit-bound switch on == the non-CP step, 3 ranks sharing
cuda:0 over gloo (tools/cp_check.py, as tests/test_cp_carry_gpu.py runs it). The one-wave-per-SIMD kernel is forced (the check's 1 152 keys are below
the length at which "auto" picks it), so every self-attention launch of the CP step is a no-running-max kernel of g3_self_attn_fwd_bounded_cp_bf16:
plain, segmented, partial, carry-in, and on rank 1 - interior - with its own block skipped. Every rank prints the schedule that actually ran and
whether the bound was used, so a silent fallback cannot pass."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCHEDULES = ("gather_first", "local_first", "local_carry")


def _free_port() -> str:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_bounded_cp_step_matches_single_rank_three_ranks():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(ROOT / "tools" / "cp_check.py")]
    env = dict(os.environ, G3_CP_CHECK_KERNEL="w4b", G3_CP_CHECK_BOUNDED="1", G3_CP_CHECK_SCHEDULES=",".join(SCHEDULES))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT), env=env)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_check] OK" in r.stdout
    # (the ranks' prints may interleave on one line: the pattern is not anchored)
    lines = re.findall(r"rank (\d)/3: CP \(([a-z_]+)\) vs non-CP denoise step rel_l2=(\S+) max_abs=\S+ effective=([a-z_]+) effective_bounded=(True|False)", r.stdout)
    assert sorted((int(rk), sched) for rk, sched, _, _, _ in lines) == sorted((rk, s) for rk in range(3) for s in SCHEDULES), r.stdout[-3000:]
    for rk, sched, rel, eff, bounded in lines:
        assert eff == sched, f"rank {rk} ran {eff} for {sched}"
        assert bounded == "True", f"rank {rk}, {sched}: the logit bound was not used"
        assert float(rel) < 5e-3
