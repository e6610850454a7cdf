"""GPU: the frame-window self-attention under context parallelism with the real HIP kernels == the single-rank windowed step, 2 and then 4 ranks
sharing cuda:0 over gloo, and once more with ONE rank over RCCL (tools/cp_window_check.py; as tests/test_cp_gpu.py does for the dense schedules)."""
import os
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


def _run(ranks, env=None):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(ROOT / "tools" / "cp_window_check.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT), env=env)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cp_window_check] OK" in r.stdout
    assert r.stdout.count("effective=window_halo") == ranks


@pytest.mark.parametrize("ranks", [2, 4])
def test_window_halo_step_matches_the_single_rank_windowed_step(ranks):
    _run(ranks)


def test_window_halo_code_path_over_rccl_single_rank():
    """backend "nccl" (= RCCL) and ONE rank: the split-size all_to_all_single of the halo exchange, Work.wait() and the RCCL-stream / compute-stream
    hand-off through the real RCCL process group (a self-exchange: the whole sequence is the rank's own)."""
    _run(1, env=dict(os.environ, G3_CP_CHECK_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0"))
