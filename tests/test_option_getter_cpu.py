"""CPU: g3_get_option reads the value of a switch that is in force in the library, whoever set it - the one source of truth behind
dit._SELF_ATTN_MFMA16 = "auto" (the 16x16x32 self-attention kernel only where the library chooses the attention kernel itself)."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_get_option_sees_every_setter():
    from gen3c_amd import _lib, dit, ops
    lib = _lib.load()
    try:
        assert ops.option("attn_variant") == 0 and dit._self_attn_mfma16()
        ops.set_option("attn_variant", 11)
        assert ops.option("attn_variant") == 11 and not dit._self_attn_mfma16()
        assert lib.g3_set_option(b"attn_variant", 4) == 0  # a direct call, as the tools make it
        assert ops.option("attn_variant") == 4 and not dit._self_attn_mfma16()
    finally:
        lib.g3_set_option(b"attn_variant", 0)
    assert dit._self_attn_mfma16()
    v = C.c_int(-1)
    assert lib.g3_get_option(b"no_such_option", C.byref(v)) != 0 and lib.g3_last_error() == b"g3_get_option: unknown option no_such_option"
    with pytest.raises(_lib.Gen3cHipError):
        ops.option("no_such_option")


def test_get_option_sees_the_environment_variable():
    code = "from gen3c_amd import dit, ops; print(ops.option('attn_variant'), dit._self_attn_mfma16())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, G3_ATTN_VARIANT="11"), capture_output=True, text=True, check=True).stdout
    assert out.split() == ["11", "False"], out
