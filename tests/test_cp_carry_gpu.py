"""GPU: a DiT denoise step under the "local_carry" context-parallel schedule == the non-CP step, 3 ranks sharing cuda:0 over gloo
(tools/cp_check.py, as tests/test_cp_gpu.py runs it), so that rank 1 is interior: its remote keys sit on both sides of its own block and its
one carry launch per head group skips that block. Every rank prints the schedule that actually ran, so a silent fallback cannot pass."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _free_port() -> str:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_local_carry_step_matches_single_rank_three_ranks():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(ROOT / "tools" / "cp_check.py")]
    env = dict(os.environ, G3_CP_CHECK_SCHEDULES="local_carry")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT), env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_check] OK" in r.stdout
    # (the ranks' prints may interleave on one line: the pattern is not anchored and stops at the schedule name)
    lines = re.findall(r"rank (\d)/3: CP \(local_carry\) vs non-CP denoise step rel_l2=(\S+) max_abs=\S+ effective=([a-z_]+)", r.stdout)
    assert sorted(int(rk) for rk, _, _ in lines) == [0, 1, 2], r.stdout[-3000:]
    for rk, rel, eff in lines:
        assert eff == "local_carry", f"rank {rk} ran {eff}"
        assert float(rel) < 5e-3
