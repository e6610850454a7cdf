"""The benchmark's self-attention launch (S = 56 320, H = 32, RMS-normalised q / k, the DiT's logit bound) on both no-max kernels, N launches each, interleaved:
hipEvent time per launch and the rel-L2 between the two outputs. argv[1] = launches per arm (default 3; one more round warms up).
The figures of profiles/attn_mfma16_ab.txt sections 2 to 4, each pass a run of its own on the GPU box:
  python tools/attn_mfma16_pair.py 6
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o s -- python tools/attn_mfma16_pair.py 6      (kernel statistics, nothing else enabled)
  rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d <dir> -o p -- python tools/attn_mfma16_pair.py 2
clock = GRBM_GUI_ACTIVE / 8 / kernel duration of the same pass; MFMA-busy share = SQ_VALU_MFMA_BUSY_CYCLES / (4 SQ_WAVE_CYCLES)."""
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))  # the repository root
from gen3c_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
S, H = 56320, 32
g = torch.Generator(device=dev).manual_seed(1)
rms = lambda x: (x.view(S, H, 128) * torch.rsqrt(x.view(S, H, 128).pow(2).mean(-1, keepdim=True))).reshape(S, H * 128)
q = rms(torch.randn(S, H * 128, device=dev, generator=g)).to(torch.bfloat16)
k = rms(torch.randn(S, H * 128, device=dev, generator=g)).to(torch.bfloat16)
v = torch.randn(S, H * 128, device=dev, generator=g).to(torch.bfloat16)
vt = ops.transpose_v(v, S, 1, H)
bound = 128 / math.sqrt(128) * 1.03
outs = {}
times = {False: [], True: []}
for i in range(n + 1):  # first round = warm-up
    for flag in (False, True):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        outs[flag] = ops.self_attn_bounded(q, k, vt, S, S, 1, H, bound, mfma16=flag)
        e1.record()
        torch.cuda.synchronize()
        if i:
            times[flag].append(e0.elapsed_time(e1))
for flag in (False, True):
    t = times[flag]
    print(f"{'16x16x32 (w4c)' if flag else '32x32x16 (w4b)'}: launches {' '.join(f'{x:.2f}' for x in t)} ms, mean {sum(t) / len(t):.2f}")
d = float((outs[True].float() - outs[False].float()).norm() / outs[False].float().norm())
print(f"rel-L2 between the two kernels' outputs: {d:.3e}; finite: {bool(torch.isfinite(outs[True].float()).all())}")
