"""The shell entry points reproduce, bit for bit, the output buffers recorded in tests/golden/shell_digests.json (tools/shell_digests.py: the
case list, how a record is made and what a digest covers).  The record was made with the library of the commit before the shell kernels were
rebuilt from shared phases; a later change that means to keep their bits leaves it alone."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("shell_digests", os.path.join(ROOT, "tools", "shell_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shell_entry_points_reproduce_the_recorded_digests():
    tool = _tool()
    with open(os.path.join(ROOT, "tests", "golden", "shell_digests.json")) as f:
        want = json.load(f)
    assert want and not [k for k, v in want.items() if v.startswith("refused")]
    assert sorted(want) == sorted(n for n, _ in tool.cases())          # the record covers the case list, nothing else
    got = tool.digests()
    bad = tool.compare(got, want)
    assert not bad, f"{len(bad)} of {len(want)} cases differ, the first: {bad[:8]}"
