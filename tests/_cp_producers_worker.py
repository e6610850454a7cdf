"""Worker of tests/test_mxfp8_producers_gpu.py: ONE rank (torchrun, RCCL) drives the tiny MXFP8 DiT through the context-parallel branches of
forward() - gather_first (K | V projected ahead of Q) and local_first (one fused QKV projection) - with mxfp8_producers "fused", and requires
the output to be bitwise the single-rank output and bitwise the "separate" arm's under the same schedule. Prints "[cp_producers] OK"."""
import sys
from pathlib import Path

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gen3c_amd.parallel import init_distributed, parallel_state  # noqa: E402
from tests._mxfp8_tiny_dit import _inputs, _net, _run  # noqa: E402


def main():
    torch.cuda.set_device(0)
    init_distributed("nccl")
    parallel_state.initialize_model_parallel(context_parallel_size=dist.get_world_size())
    dev = torch.device("cuda:0")
    inp = _inputs()
    net = _net(dev, "mxfp8", producers="fused")
    single = _run(net, inp, dev)
    net.enable_context_parallel(parallel_state.get_context_parallel_group())
    good = True
    for sched in ("gather_first", "local_first"):
        net._cp_attn.configure(head_groups=2, schedule=sched)
        out = {}
        for producers in ("separate", "fused"):
            net.set_mxfp8_producers(producers)
            out[producers] = _run(net, inp, dev)
        same_arm, same_single = torch.equal(out["fused"], out["separate"]), torch.equal(out["fused"], single)
        print(f"[cp_producers] {sched}: fused == separate {same_arm}; fused == single-rank fused {same_single}", flush=True)
        good = good and same_arm and same_single
    dist.destroy_process_group()
    if not good:
        sys.exit(1)
    print("[cp_producers] OK", flush=True)


if __name__ == "__main__":
    main()
