"""tests/golden/align_edges.npz: the reference's own results on the edge inputs of tests/align_kernel_ref.py (sibling of gen_golden_align.py).
Per case: the inputs, torch.quantile(q = 0.1, 0.9) of both valid inverse-depth sets, and - where the fit is well conditioned - the reference's
camera_utils.align_depth output, rigid and non-rigid after 1 and 2 Adam steps (CPU, torch autograd).
Run in the build container (needs the reference checkout); the tests only read the committed .npz."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import ref_shims  # noqa: E402

ref_shims.install()
from cosmos_predict1.diffusion.inference.camera_utils import align_depth  # noqa: E402

from tests import align_kernel_ref as kr  # noqa: E402

t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
K, c2w, _, _ = kr.camera(kr.H, kr.W)
out = dict(K=K, c2w=c2w)
for name in kr.FIXTURE_CASES:
    src, tgt, mask = kr.build_case(name)
    out[f"{name}_source"], out[f"{name}_target"], out[f"{name}_mask"] = src, tgt, mask
    si, ti, sv, tv, _ = kr.inverses(src, tgt, mask)
    q = torch.tensor([0.1, 0.9])
    out[f"{name}_quantiles"] = np.stack([torch.quantile(t(si[sv]), q).numpy(), torch.quantile(t(ti[tv]), q).numpy()])  # [array][q]
    if name not in kr.FIT_CASES:
        continue
    with np.errstate(all="ignore"):
        out[f"{name}_rigid"] = align_depth(t(src), t(tgt), t(mask)).numpy()
        for iters in (1, 2):
            with torch.enable_grad():
                r = align_depth(t(src), t(tgt), t(mask), k=t(K), c2w=t(c2w), alignment_method="non_rigid", num_iters=iters, lambda_arap=0.1,
                                smoothing_kernel_size=3)
            out[f"{name}_non_rigid_{iters}"] = r.detach().numpy()
np.savez_compressed(kr.GOLD, **out)
for k, v in out.items():
    print(k, v.shape, v.dtype)
print(kr.GOLD, kr.GOLD.stat().st_size, "bytes")
