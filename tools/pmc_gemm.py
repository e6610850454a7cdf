"""A few launches of the step's five block-GEMM shapes (B = 2: M = 2 x 56 320, and the operand-swapped V^T launch), for a rocprofv3 counter pass of its own:
  rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d <dir> -o p -- python tools/pmc_gemm.py [launches per shape]
then  python tools/pmc_summary.py <parent of dir> <out.csv> gemm_bf16 . Held clock = GRBM_GUI_ACTIVE / 8 / duration (the counter sums the 8 XCDs);
MFMA busy = SQ_VALU_MFMA_BUSY_CYCLES / (4 x SQ_WAVE_CYCLES) at one wave per SIMD. The kernels' names tell the classes apart only by epilogue
(<0>: q | k and V^T, <1>: MLP up, <2>: attention out and MLP down), so the script prints the order of its launches: the trace lists them in it."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd import _lib, ops  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda:0")
S, B, D = 56320, 2, 4096
M = S * B
h = torch.randn(M, D, device=dev).to(torch.bfloat16)
SHAPES = [("qk", M, 8192, 4096, 0), ("vt", D, S, 4096, 0), ("out", M, 4096, 4096, 2), ("w1", M, 16384, 4096, 1), ("w2", M, 4096, 16384, 2)]
for (name, m, n, k, epi) in SHAPES:
    if name == "vt":  # V^T[b] = W_v h[:, b]^T: a = W_v, w = the batch item's token rows (row stride B D), output rows of ceil64(S) tokens
        a = (torch.randn(m, k, device=dev) * 0.02).to(torch.bfloat16)
        w = h.view(S, B, D)[:, 0]
    else:
        a = h if k == D else torch.randn(m, k, device=dev).to(torch.bfloat16)
        w = (torch.randn(n, k, device=dev) * 0.02).to(torch.bfloat16)
    o = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
    kw = dict(gate=torch.randn(B, n, device=dev).to(torch.bfloat16), residual=torch.randn(m, n, device=dev).to(torch.bfloat16)) if epi == 2 else {}
    for _ in range(REPS):
        ops.gemm_nt(a, w, out=o, epilogue=epi, **kw)
    torch.cuda.synchronize()
    print(f"{REPS} x {name}: M={m} N={n} K={k} epilogue={epi} kernel={_lib.load().g3_gemm_kernel_name(m, n, k, epi).decode()}", flush=True)
    del a, w, o, kw
print("done")
