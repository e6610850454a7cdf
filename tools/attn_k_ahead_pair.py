"""The benchmark's self-attention launch (S = 56 320, H = 32, B = 1, RMS-normalised q / k, the DiT's bound) on flash_attn_fwd_w4c_nm_kernel of TWO libraries,
interleaved: this tree's and one built from another checkout (the parent commit of a schedule change). hipEvent time per launch, and whether the two
outputs are bitwise equal. The launch figures of profiles/attn_k_ahead_ab.txt, each pass a run of its own on the GPU box:
  python tools/attn_k_ahead_pair.py OTHER/gen3c_amd/lib/libgen3c_hip.so 6
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o s -- python tools/attn_k_ahead_pair.py OTHER/... 6 --only other   (and --only this)
  rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d <dir> -o p -- python tools/attn_k_ahead_pair.py OTHER/... 2 --only other
Both libraries name the kernel alike, so a profiler pass takes one library at a time (--only). clock = GRBM_GUI_ACTIVE / 8 / kernel duration of the same
pass; MFMA-busy share = SQ_VALU_MFMA_BUSY_CYCLES / (4 SQ_WAVE_CYCLES). argv: the other library, launches per arm (default 3; one more round warms up)."""
import ctypes as C
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))  # the repository root
from gen3c_amd import _lib, ops  # noqa: E402

this = _lib.load()
other = C.CDLL(str(Path(sys.argv[1]).resolve()))
for name, argtypes in _lib.SIGNATURES.items():
    if hasattr(other, name):
        getattr(other, name).argtypes = argtypes
        getattr(other, name).restype = _lib._RESTYPES.get(name, C.c_int)
n = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 3
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
arms = [(a, lib) for (a, lib) in (("other", other), ("this", this)) if only in (None, a)]
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
S, H = 56320, 32
g = torch.Generator(device=dev).manual_seed(1)
rms = lambda x: (x.view(S, H, 128) * torch.rsqrt(x.view(S, H, 128).pow(2).mean(-1, keepdim=True))).reshape(S, H * 128)
q = rms(torch.randn(S, H * 128, device=dev, generator=g)).to(torch.bfloat16)
k = rms(torch.randn(S, H * 128, device=dev, generator=g)).to(torch.bfloat16)
v = torch.randn(S, H * 128, device=dev, generator=g).to(torch.bfloat16)
vt = ops.transpose_v(v, S, 1, H)
ld = vt.shape[-1]
bound = 128 / math.sqrt(128) * 1.03
for _a, lib in arms:
    assert lib.g3_self_attn16_kernel_name(S, S, 1, H, bound, 11).decode() == "flash_attn_fwd_w4c_nm_kernel"
outs = {a: torch.empty_like(q) for a, _ in arms}
times = {a: [] for a, _ in arms}
for i in range(n + 1):  # first round = warm-up
    for a, lib in arms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib.g3_self_attn_fwd_bounded16_bf16(q.data_ptr(), H * 128, H * 128, 128, k.data_ptr(), H * 128, H * 128, 128, vt.data_ptr(), ld, H * 128 * ld, 128 * ld, 0, 0,
                                                 outs[a].data_ptr(), None, None, H * 128, H * 128, 128, S, S, 1, H, 128, 1.0 / math.sqrt(128), bound, 11, st)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, lib.g3_last_error()
        if i:
            times[a].append(e0.elapsed_time(e1))
for a, _ in arms:
    t = times[a]
    print(f"{a:5s} library: launches {' '.join(f'{x:.2f}' for x in t)} ms, mean {sum(t) / len(t):.3f}")
if only is None:
    print(f"outputs bitwise equal: {bool(torch.equal(outs['this'], outs['other']))}; finite: {bool(torch.isfinite(outs['this'].float()).all())}")
