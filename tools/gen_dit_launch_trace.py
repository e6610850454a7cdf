"""Records tests/golden/dit_launch_trace_parent.json: the C calls the Python front end (gen3c_amd/ops.py, gen3c_amd/dit.py) makes for every case of
tests/test_dit_launch_trace_cpu.py, dry-run on the CPU (tests/dit_launch_trace.py). It is recorded ONCE, from the commit before the front end
was folded, with that commit's own ops.py / dit.py and library:

  git worktree add ../parent <parent commit>         (and build its library: python -m gen3c_amd.build inside it)
  python tools/gen_dit_launch_trace.py --tree ../parent

--tree: where `gen3c_amd` is imported from (default: this tree); the cases and the recorder always come from this tree's tests/.
Distinct rows are stored once; a case holds indices into them (and, where kernel timers were on, their (kind, meta) pairs)."""
import argparse
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", type=Path, default=ROOT)
    ap.add_argument("--out", type=Path, default=ROOT / "tests" / "golden" / "dit_launch_trace_parent.json")
    args = ap.parse_args()
    sys.path.insert(0, str(args.tree.resolve()))
    import gen3c_amd
    from gen3c_amd import dit, ops, parallel, sparse_attn  # noqa: F401  (everything the cases import, from --tree)
    sys.path.remove(str(args.tree.resolve()))
    sys.path.insert(0, str(ROOT))
    assert Path(gen3c_amd.__file__).resolve().parent.parent == args.tree.resolve(), gen3c_amd.__file__
    from tests import test_dit_launch_trace_cpu as cases

    rows, index, out = [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in cases.CASES:
            undo = []

            def patch(obj, attr, value):
                undo.append((obj, attr, getattr(obj, attr)))
                setattr(obj, attr, value)
            try:
                got = cases.run_case(name, patch, tmp)
            finally:
                for obj, attr, value in reversed(undo):
                    setattr(obj, attr, value)
            ids = []
            for row in got["rows"]:
                key = json.dumps(row)
                if key not in index:
                    index[key] = len(rows)
                    rows.append(row)
                ids.append(index[key])
            out[name] = dict(got, rows=ids)
            print(f"{len(ids):5d} calls  {name}")
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
    one = lambda v: json.dumps(v, separators=(",", ":"))
    note = "see tests/test_dit_launch_trace_cpu.py. Recorded by tools/gen_dit_launch_trace.py from the commit before the front end was folded; not regenerated since"
    text = ('{\n "note": ' + one(note) + ',\n "rows": [\n  ' + ",\n  ".join(one(r) for r in rows) + '\n ],\n "cases": {\n  ' +
            ",\n  ".join(one(n) + ": " + one(c) for n, c in out.items()) + "\n }\n}\n")  # one row, one case per line
    assert json.loads(text) == dict(note=note, rows=rows, cases=out)
    args.out.write_text(text)
    print(f"{len(rows)} distinct rows, {len(text)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
