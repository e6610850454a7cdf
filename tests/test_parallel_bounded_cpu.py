"""CPU (gloo, world 3 so that rank 1 is interior): ContextParallelAttention's `bounded` switch. With it on and a positive logit bound every attention
launch of the key-sharding schedules - gather_first, local_first, local_carry - goes through the backend's "attention_bounded_cp" with the key ranges
and the skip the unbounded launches have; off, with a bound of 0 or with a backend that lacks the callable the launches are today's. The HIP kernels
cannot run here: the backend callables are an fp64 oracle that records its calls. Column 0 of every head group of K holds the key's position, so a
call's key range is read from the keys it was handed."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_parallel_head_cpu import _oracle_backend, _part, _v_rows

WORLD, SL, B, H, G = 3, 64, 2, 6, 2  # 3 heads per group for the key-sharding schedules; head_parallel: 2 heads per rank, one per group
S = SL * WORLD
BOUND = 3.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranges(pos):
    """sorted key positions -> [(begin, end), ...]"""
    out = []
    for p in pos:
        if out and out[-1][1] == p:
            out[-1][1] = p + 1
        else:
            out.append([p, p + 1])
    return tuple((a, b) for a, b in out)


def _recording_backend(calls, with_bounded=True):
    """the oracle backend of tests/test_parallel_head_cpu.py with every attention callable recording (name, Sq, Skv, H, partial, carry, kv_skip, key ranges)"""
    be = _oracle_backend(with_exchange=True, calls=None)

    def run(name, q, k, vt, Sq, Skv, Bq, Hq, out=None, carry=None, kv_skip=None, partial=False):
        v = _v_rows(vt, Bq, Hq)
        k4 = k.reshape(-1, Bq, Hq * 128)
        if kv_skip is not None:
            b0, n = kv_skip
            keep = [i for i in range(k4.shape[0]) if not (b0 <= i < b0 + n)]
            k4, v = k4[keep], v[keep]
        assert k4.shape[0] == Skv == v.shape[0], (name, k4.shape, Skv)
        pos = [int(round(float(x) * S)) for x in k4[:, 0, 0]]
        calls.append((name, Sq, Skv, Hq, bool(partial), carry is not None, kv_skip, _ranges(pos)))
        o, lse = _part(q, k4.reshape(-1, Hq * 128), v, Sq, Bq, Hq)
        if carry is not None:
            oc, lc = carry[0].double(), carry[1].double()
            m = torch.maximum(lc, lse)
            wc, wk = torch.exp2(lc - m), torch.exp2(lse - m)
            rows = lambda w: w.permute(2, 0, 1).reshape(Sq * Bq, Hq).repeat_interleave(128, dim=1)
            o = (rows(wc) * oc + rows(wk) * o) / rows(wc + wk)
            lse = m + torch.log2(wc + wk)
        if partial:
            if out is None:
                out = torch.empty(Sq * Bq, Hq * 128, dtype=torch.float32)
            out.copy_(o.float())
            return out, lse.float().contiguous()
        if out is None:
            out = torch.empty(Sq * Bq, Hq * 128, dtype=q.dtype)
        out.copy_(o.to(out.dtype))
        return out

    be["attention"] = lambda q, k, vt, Sq, Skv, Bq, Hq, out, variant=0: run("attention", q, k, vt, Sq, Skv, Bq, Hq, out=out)
    be["attention_partial"] = lambda q, k, vt, Sq, Skv, Bq, Hq, variant=0: run("attention_partial", q, k, vt, Sq, Skv, Bq, Hq, partial=True)
    be["attention_carry"] = lambda q, k, vt, Sq, Skv, Bq, Hq, out=None, carry=None, kv_skip=None, partial=False, variant=0: run(
        "attention_carry", q, k, vt, Sq, Skv, Bq, Hq, out=out, carry=carry, kv_skip=kv_skip, partial=partial)
    plain_bounded = be["attention_bounded"]

    def attention_bounded(q, k, vt, Sq, Skv, Bq, Hq, logit_bound, out, variant=0):
        calls.append(("attention_bounded", Sq, Skv, Hq))
        return plain_bounded(q, k, vt, Sq, Skv, Bq, Hq, logit_bound, out, variant=variant)

    be["attention_bounded"] = attention_bounded
    if with_bounded:
        def bounded_cp(q, k, vt, Sq, Skv, Bq, Hq, logit_bound, out=None, carry=None, kv_skip=None, partial=False, variant=0):
            assert logit_bound == BOUND
            return run("attention_bounded_cp", q, k, vt, Sq, Skv, Bq, Hq, out=out, carry=carry, kv_skip=kv_skip, partial=partial)
        be["attention_bounded_cp"] = bounded_cp
    return be


def _expected(schedule, rank, names):
    """the launches of one layer on `rank`: (name, Sq, Skv, heads, partial, carry, kv_skip, key ranges), phase 1 of all groups first"""
    Hg = H // G
    own = ((rank * SL, (rank + 1) * SL),)
    before, after = ((0, rank * SL),), (((rank + 1) * SL, S),)
    remote = tuple(r for r in (before[0], after[0]) if r[1] > r[0])
    if schedule == "gather_first":
        return [(names["attention"], SL, S, Hg, False, False, None, ((0, S),))] * G
    if schedule == "local_first":
        ph2 = [(names["attention_partial"], SL, r[1] - r[0], Hg, True, False, None, (r,)) for r in remote]
        return [(names["attention_partial"], SL, SL, Hg, True, False, None, own)] * G + ph2 * G
    skip = (rank * SL, SL) if 0 < rank < WORLD - 1 else None
    return ([(names["attention_carry"], SL, SL, Hg, True, False, None, own)] * G
            + [(names["attention_carry"], SL, S - SL, Hg, False, True, skip, remote)] * G)


PLAIN = dict(attention="attention", attention_partial="attention_partial", attention_carry="attention_carry")
BOUNDED = dict.fromkeys(PLAIN, "attention_bounded_cp")


def _worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from gen3c_amd import parallel
    parallel.init_distributed("gloo")
    parallel.parallel_state.initialize_model_parallel(context_parallel_size=world)
    group = parallel.parallel_state.get_context_parallel_group()
    try:
        g = torch.Generator().manual_seed(0)
        D = H * 128
        q, k, v = (torch.randn(S * B, D, generator=g) for _ in range(3))
        for grp in range(G):  # the key's position, in column 0 of every head group (and of head_parallel's per-rank head blocks: unused there)
            k[:, grp * (D // G)] = torch.arange(S).repeat_interleave(B).float() / S
        rows = slice(rank * SL * B, (rank + 1) * SL * B)
        ref, _ = _part(q[rows], k, v.reshape(S, B, H, 128), SL, B, H)
        ql, kl, vl = q[rows], k[rows], v[rows]

        def run(schedule, bounded, bound, with_bounded=True, via_configure=False):
            calls = []
            be = _recording_backend(calls, with_bounded)
            if via_configure:
                cpa = parallel.ContextParallelAttention(group, head_groups=G, backend=be, schedule=schedule).configure(bounded=bounded)
            else:
                cpa = parallel.ContextParallelAttention(group, head_groups=G, backend=be, schedule=schedule, bounded=bounded)
            out = cpa(ql, kl, vl, SL, B, H, logit_bound=bound)
            torch.testing.assert_close(out, ref.float(), rtol=1e-5, atol=1e-5)
            return cpa, calls

        for i, schedule in enumerate(("gather_first", "local_first", "local_carry")):
            cpa, calls = run(schedule, True, BOUND, via_configure=bool(i % 2))
            assert cpa.effective["schedule"] == schedule and cpa.effective_bounded is True, (cpa.effective, cpa.effective_bounded)
            assert set(cpa.effective) == {"schedule", "kernel", "head_groups"}  # bench.py copies this dict: no new key
            assert calls == _expected(schedule, rank, BOUNDED), (schedule, rank, calls)
            today = None
            for bounded, bound, with_bounded in ((False, BOUND, True), (True, 0.0, True), (True, BOUND, False), (False, 0.0, False)):
                cpa, calls = run(schedule, bounded, bound, with_bounded)
                assert cpa.effective["schedule"] == schedule and cpa.effective_bounded is False
                assert calls == _expected(schedule, rank, PLAIN), (schedule, rank, bounded, bound, with_bounded, calls)
                today = today or calls
                assert calls == today
        # head_parallel: the bound alone selects its bounded launch, the switch changes nothing
        for bounded in (False, True):
            for bound in (BOUND, 0.0):
                cpa, calls = run("head_parallel", bounded, bound)
                assert cpa.effective["schedule"] == "head_parallel" and cpa.effective_bounded is False
                assert [c[:4] for c in calls] == [("attention_bounded" if bound else "attention", S, S, 1)] * 2, calls  # one launch per group, all keys
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write("ok")
    finally:
        dist.destroy_process_group()


def test_bounded_switch_world_three(tmp_path):
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(WORLD))


def test_default_backend_offers_the_bounded_callable():
    from gen3c_amd import parallel
    be = parallel._default_backend()
    assert callable(be["attention_bounded_cp"]) and callable(be["attention_bounded"])


def test_cp_logit_bound_env_reaches_the_switch(monkeypatch):
    """G3_CP_LOGIT_BOUND=1 is read in dit.enable_context_parallel next to G3_CP_CONFIG (no GPU work: an unbuilt network object, only the CP plumbing);
    the default is off; the command lines carry --cp_logit_bound."""
    import argparse
    from gen3c_amd import parallel
    from gen3c_amd.cli_common import add_common_args
    from gen3c_amd.dit import VideoExtendGeneralDIT
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 4)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 1)
    net = VideoExtendGeneralDIT.__new__(VideoExtendGeneralDIT)
    net._tables = {}
    monkeypatch.delenv("G3_CP_LOGIT_BOUND", raising=False)
    monkeypatch.delenv("G3_CP_CONFIG", raising=False)
    VideoExtendGeneralDIT.enable_context_parallel(net, object())
    assert net._cp_attn.bounded is False and net._cp_attn.effective_bounded is False and net._cp_attn.schedule == "local_first"
    monkeypatch.setenv("G3_CP_LOGIT_BOUND", "0")
    VideoExtendGeneralDIT.enable_context_parallel(net, object())
    assert net._cp_attn.bounded is False
    monkeypatch.setenv("G3_CP_LOGIT_BOUND", "1")
    monkeypatch.setenv("G3_CP_CONFIG", "2,w4b,local_carry")
    VideoExtendGeneralDIT.enable_context_parallel(net, object())
    assert net._cp_attn.bounded is True and net._cp_attn.schedule == "local_carry" and net._cp_attn.kernel == "w4b" and net._cp_attn.head_groups == 2
    ap = add_common_args(argparse.ArgumentParser())
    assert ap.parse_args([]).cp_logit_bound is False and ap.parse_args(["--cp_logit_bound"]).cp_logit_bound is True
    assert parallel.ContextParallelAttention.__init__.__defaults__[-1] is False  # bounded=False
