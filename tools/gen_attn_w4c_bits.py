"""Records the bits flash_attn_fwd_w4c_nm_kernel writes today, for tests/test_attn_w4c_kahead_gpu.py: a change to the kernel's schedule (where its LDS-DMA
pieces sit, which tile they fetch) must leave every output bit where it was.

Run ONCE on the GPU, on a build of the commit whose bits are to be kept (the parent of the schedule change):
  python tools/gen_attn_w4c_bits.py [--root CHECKOUT] [--commit HASH] [--overwrite]
--root: the checkout whose library runs (default: this one); --commit: recorded in the file (default: git rev-parse HEAD of that checkout). Writes
tests/golden/attn_w4c_parent_bits.json of THIS checkout: per shape the SHA-256 of the output bytes and the first 64 output values. Refuses to overwrite an
existing file without --overwrite.

The inputs are made on the host by numpy.random.RandomState, with no reduction anywhere: entries uniform in [-1, 1] rounded to bf16, so |q|, |k| <= sqrt(128)
and the unit-weight logit bound holds. They are the same on every machine, and the test recomputes them from host_inputs() below."""
import argparse
import hashlib
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent.parent
GOLDEN = HERE / "tests" / "golden" / "attn_w4c_parent_bits.json"
HD = 128
B, H = 2, 2
D = H * HD
SQ = 320  # two query blocks, the second ragged
SKVS = (64, 128, 192, 256, 320, 384, 1024)  # 1 to 6 key tiles, and 16
BOUND = HD / math.sqrt(HD) * 1.03  # unit norm weights, with the margin the DiT passes


def host_inputs(Sq, Skv):
    """(fused q buffer [Sq*B, 3 D], fused k buffer [Skv*B, 3 D], v [Skv*B, D]) as bf16 CPU tensors; q = columns [0, D), k = columns [D, 2 D)"""
    rs = np.random.RandomState(1000 * Sq + Skv)
    draw = lambda rows, cols: torch.from_numpy(rs.uniform(-1.0, 1.0, size=(rows, cols)).astype(np.float32)).to(torch.bfloat16)
    return draw(Sq * B, 3 * D), draw(Skv * B, 3 * D), draw(Skv * B, D)


def output_record(out):
    """out: the [Sq*B, D] bf16 result (any device, any strides)"""
    flat = out.detach().to("cpu").contiguous().view(torch.int16).numpy().tobytes()
    return {"sha256": hashlib.sha256(flat).hexdigest(), "first64": [float(x) for x in out.detach().to("cpu").contiguous().flatten()[:64].float()]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--overwrite", action="store_true")
    a = ap.parse_args()
    if GOLDEN.exists() and not a.overwrite:
        sys.exit(f"{GOLDEN} exists: these are the parent's recorded bits; pass --overwrite to replace them")
    root = Path(a.root).resolve()
    commit = a.commit or subprocess.run(["git", "-C", str(root), "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    sys.path.insert(0, str(root))
    from gen3c_amd import _lib, ops
    assert Path(ops.__file__).resolve().is_relative_to(root), ops.__file__
    lib = _lib.load()
    dev = torch.device("cuda:0")
    shapes = {}
    for Skv in SKVS:
        name = lib.g3_self_attn16_kernel_name(SQ, Skv, B, H, float(BOUND), 11).decode()
        assert name == "flash_attn_fwd_w4c_nm_kernel", name
        qf, kf, v = (x.to(dev) for x in host_inputs(SQ, Skv))
        out = ops.self_attn_bounded(qf[:, :D], kf[:, D:2 * D], ops.transpose_v(v, Skv, B, H), SQ, Skv, B, H, BOUND, variant=11, mfma16=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        shapes[f"{SQ}x{Skv}"] = output_record(out)
        print(f"Sq={SQ} Skv={Skv}: {shapes[f'{SQ}x{Skv}']['sha256']}")
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    GOLDEN.write_text(json.dumps({"commit": commit, "kernel": "flash_attn_fwd_w4c_nm_kernel", "B": B, "H": H, "bound": BOUND, "shapes": shapes}, indent=1) + "\n")
    print(f"wrote {GOLDEN} (commit {commit})")


if __name__ == "__main__":
    main()
