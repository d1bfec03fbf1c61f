"""CPU tier of the engine switches (the device tier is test_engine_switches_gpu.py).

literalkg_amd/ops.py reads its process-wide switches from the environment once, at import.  Each case below imports the
module in a fresh child Python with ONE variable set (no GPU is needed for the import) and reads back the module constants
and the three predicates every dispatch above the kernels hangs on:

    tall_ok(20000, 32, (32, 2, 12))     the tall engine / the fused gate
    _wants_rowmax(20000)                producers emit row maxima for it
    fused_layer_ok(20000, 32, (32,))    the one-launch layer forward

LKG_GEMM_ENGINE and LKG_WGRAD_ENGINE accept the names of ops.GEMM_ENGINES / ops.WGRAD_ENGINES (surrounding whitespace
stripped); anything else ends the import with a ValueError that names the variable, the value and the accepted list -- a typo
used to switch the tall engine, the fused gate and the fused layer off without a word.  The four boolean / mode variables keep
the parsing they have: the values each accepts today are pinned as they are."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARS = ("LKG_GEMM_ENGINE", "LKG_WGRAD_ENGINE", "LKG_FOLD_F32", "LKG_NARROW_LAYER", "LKG_FUSED_LAYER", "LKG_CHECK_STRUCTURES")
CHILD = """
import json
from literalkg_amd import ops
print(json.dumps(dict(engine=ops._ENGINE, wgrad=ops._WGRAD_ENGINE, fold_f64=ops.FOLD_F64, narrow=ops.NARROW_LAYER,
                      fused=ops.FUSED_LAYER, check=ops.CHECK_STRUCTURES, tall_ok=ops.tall_ok(20000, 32, (32, 2, 12)),
                      wants_rowmax=ops._wants_rowmax(20000), fused_layer_ok=ops.fused_layer_ok(20000, 32, (32,)))))
"""
DEFAULTS = dict(engine="f16x2", wgrad="longk", fold_f64=True, narrow=True, fused="auto", check=False, tall_ok=True,
                wants_rowmax=True, fused_layer_ok=True)


def child(**env_set):
    """(exit code, the child's JSON line or None, stderr) of one import with exactly ``env_set`` of the switches set"""
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env.update(env_set)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p.stderr


def expect(env_set, **changed):
    code, got, err = child(**env_set)
    assert code == 0 and got is not None, (env_set, code, err[-2000:])
    assert got == dict(DEFAULTS, **changed), (env_set, got)


def test_defaults():
    expect({})


# the table of DESIGN.md 3.6v: engine name -> (tall_ok, _wants_rowmax, fused_layer_ok)
GEMM = {"f16x2": (True, True, True), "f16x2-all": (True, True, True), "bf16x3": (False, False, False), "f32": (False, False, False)}


@pytest.mark.parametrize("value", list(GEMM) + [" f16x2-all\t"])
def test_gemm_engine_accepted(value):
    name = value.strip()
    tall, rowmax, layer = GEMM[name]
    expect({"LKG_GEMM_ENGINE": value}, engine=name, tall_ok=tall, wants_rowmax=rowmax, fused_layer_ok=layer)


@pytest.mark.parametrize("value", ["longk", "bf16x3", "bf16x3 "])
def test_wgrad_engine_accepted(value):
    expect({"LKG_WGRAD_ENGINE": value}, wgrad=value.strip())        # (no predicate reads it: _FusedGate.backward and gemm_engine do)


@pytest.mark.parametrize("var,accepted", [("LKG_GEMM_ENGINE", ("f16x2", "f16x2-all", "bf16x3", "f32")),
                                          ("LKG_WGRAD_ENGINE", ("longk", "bf16x3"))])
@pytest.mark.parametrize("value", ["nonsense", "F32", "f16x2,"])
def test_unknown_engine_name_is_refused_at_import(var, accepted, value):
    code, got, err = child(**{var: value})
    assert code != 0 and got is None, (var, value, got)
    last = err.strip().splitlines()[-1]
    assert last.startswith("ValueError") and var in last and repr(value) in last, err[-2000:]
    assert all(a in last for a in accepted), last


@pytest.mark.parametrize("var,value,changed", [
    # LKG_FOLD_F32: the float64 fold unless set to anything but "" / "0"
    ("LKG_FOLD_F32", "", {}), ("LKG_FOLD_F32", "0", {}), ("LKG_FOLD_F32", "1", dict(fold_f64=False)),
    ("LKG_FOLD_F32", "yes", dict(fold_f64=False)),
    # LKG_NARROW_LAYER: on unless "" / "0"
    ("LKG_NARROW_LAYER", "", dict(narrow=False)), ("LKG_NARROW_LAYER", "0", dict(narrow=False)), ("LKG_NARROW_LAYER", "1", {}),
    ("LKG_NARROW_LAYER", "yes", {}),
    # LKG_FUSED_LAYER: stripped, lower-cased; "" / auto, 0 / off, 1 / on; anything else is "auto"
    ("LKG_FUSED_LAYER", "", {}), ("LKG_FUSED_LAYER", "auto", {}), ("LKG_FUSED_LAYER", "0", dict(fused=False)),
    ("LKG_FUSED_LAYER", "off", dict(fused=False)), ("LKG_FUSED_LAYER", "1", dict(fused=True)),
    ("LKG_FUSED_LAYER", " ON ", dict(fused=True)), ("LKG_FUSED_LAYER", "nonsense", {}),
    # LKG_CHECK_STRUCTURES: off unless set to anything but "" / "0" (tests/conftest.py sets it to 1 for the test tiers)
    ("LKG_CHECK_STRUCTURES", "", {}), ("LKG_CHECK_STRUCTURES", "0", {}), ("LKG_CHECK_STRUCTURES", "1", dict(check=True)),
    ("LKG_CHECK_STRUCTURES", "yes", dict(check=True)),
])
def test_the_other_switches_parse_as_they_do_today(var, value, changed):
    expect({var: value}, **changed)
