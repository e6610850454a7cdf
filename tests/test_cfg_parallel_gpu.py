"""GPU: CFG-parallel with the real HIP kernels, ranks sharing cuda:0 over gloo (tools/cfg_check.py; RCCL itself needs one GPU per rank). The
CFG-parallel denoise step is held to BIT equality against code that exists without it: the single-rank step (2 ranks, cfg 2 x cp 1) and the plain
context-parallel two-call step (4 ranks, cfg 2 x cp 2, gather_first and local_first), plus the chunk's render / encode stages sharded over all 4 ranks."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _free_port() -> str:
    import socket
    with socket.socket() as s:  # hard-coded rendezvous ports collide on shared boxes
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _cfg_check(ranks: int) -> str:
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(ROOT / "tools" / "cfg_check.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[cfg_check] OK" in r.stdout
    assert ": False" not in r.stdout
    return r.stdout


def _said(out: str, rank: int, world: int, what: str) -> int:
    """How often rank `rank` printed the statement `what` (ranks write to one pipe: their lines can run into each other, the statements stay whole)."""
    return len(re.findall(rf"\[cfg_check\] rank {rank}/{world} \([^)]*\): {re.escape(what)}", out))


def test_cfg_parallel_two_ranks_equal_the_single_rank_step_bitwise():
    out = _cfg_check(2)
    for rank in (0, 1):
        for what in ("CFG-parallel step == single-rank two-call step: True", "CFG-parallel step == single-rank fused step: True",
                     "both ranks of the pair hold the same xt: True"):
            assert _said(out, rank, 2, what) == 1, (rank, what)


def test_cfg_parallel_four_ranks_equal_the_plain_context_parallel_step_bitwise():
    out = _cfg_check(4)
    for rank in range(4):
        for sched in ("gather_first", "local_first"):
            for what in (f"plain cp = 2 ({sched}) two-call step is deterministic: True", f"CFG-parallel ({sched}) step == plain cp = 2 two-call step: True",
                         f"CFG-parallel ({sched}) ran the requested schedule: True", f"CFG-parallel ({sched}) vs non-parallel full step rel_l2 < 5e-3: True",
                         f"both ranks of the pair hold the same xt ({sched}): True"):
                assert _said(out, rank, 4, what) == 1, (rank, what)
        for what in ("render sharded over 4 ranks (N=1, foreground_masking=False) == replicated: True",
                     "render sharded over 4 ranks (N=2, foreground_masking=True) == replicated: True",
                     "tokenizer encodes sharded (4 clips over 4 ranks) == replicated: True"):
            assert _said(out, rank, 4, what) == 1, (rank, what)
