"""CPU dry run of the Python front end (gen3c_amd/ops.py, gen3c_amd/dit.py): inside `traced()` the library is a recording proxy, ops._dev a dtype
check + data_ptr() and ops._stream 0, so CPU tensors go through every wrapper and the list of C calls they WOULD make comes back - nothing is
launched. Shared by tests/test_dit_launch_trace_cpu.py and tools/gen_dit_launch_trace.py.

A row is [symbol, item per argument], typed from _lib.SIGNATURES: scalars as they are (floats as Python floats), a pointer as "null" or "p<i>" with
i the index of its first appearance within that call (null-ness and aliasing such as `out is residual`, independent of the allocator), a ctypes
array as "array<n>"."""
import contextlib
import ctypes as C

import torch

from gen3c_amd import _lib, ops

# answered by the real library: host-only queries and the dry runs, which dereference no pointer
HOST_ONLY = frozenset("""g3_get_option g3_set_option g3_last_error g3_self_attn_window_q_rows g3_self_attn_window_tiles g3_self_attn_window_cp_tiles
    g3_attn_ranges_check g3_self_attn_ranges_max g3_attn_profile_members g3_attn_profile_chunks g3_attn_profile_workspace_bytes g3_attn_plan_bf16
    g3_attn_plan16_bf16 g3_attn_window_plan_bf16 g3_attn_window_cp_plan_bf16 g3_attn_ranges_plan_bf16""".split())


def _item(ctype, arg, seen: dict):
    if isinstance(arg, C.Array):
        return f"array{len(arg)}"
    if ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer):
        if isinstance(arg, C.c_void_p):
            arg = arg.value
        if not arg:
            return "null"
        key = arg if isinstance(arg, int) else id(getattr(arg, "_obj", arg))  # (byref(x): the object pointed to)
        return f"p{seen.setdefault(key, len(seen))}"
    return float(arg) if ctype is C.c_float else int(arg)


class _Recorder:
    """Stands in for the loaded library: HOST_ONLY symbols are the real ones, every other one is recorded and answered G3_OK without being called."""

    def __init__(self, real):
        self._real, self.rows = real, []

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self._real, name)
        types = _lib.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(types), f"{name}: {len(args)} arguments for {len(types)} parameters"
            seen = {}
            self.rows.append([name] + [_item(t, a, seen) for t, a in zip(types, args)])
            return _lib.G3_OK
        return call


def _dev(t, name, dtype=torch.bfloat16):
    if t.dtype != dtype:
        raise _lib.Gen3cHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


@contextlib.contextmanager
def traced():
    """with traced() as rows: ... - `rows` fills with the calls made inside the block, and stays as it is once the block is left."""
    rec = _Recorder(_lib.load())
    saved = (_lib.load, ops._dev, ops._stream)
    _lib.load, ops._dev, ops._stream = (lambda: rec), _dev, (lambda: 0)
    try:
        yield rec.rows
    finally:
        _lib.load, ops._dev, ops._stream = saved
        rec.rows = []  # (a kernel timer collected later still destroys its events through `rec`)
