"""CPU: smalltts_amd.api keeps every name it had before its code moved into options.py and plans.py, and those two modules stay
importable without torch.

tests/golden/api_names.txt is dir(smalltts_amd.api) of the commit before the split, without dunder names and imported modules."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "api_names.txt")) as f:
    NAMES = f.read().split()


def test_the_list_is_the_one_that_was_recorded():
    assert len(NAMES) == 95 and len(set(NAMES)) == 95
    assert {"Takes", "as_repair", "frames_of_groups", "_Batch", "_ENGINES", "_validated", "check_takes_sv"} <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_every_name_still_resolves_on_api(name):
    from smalltts_amd import api
    assert hasattr(api, name), f"smalltts_amd.api lost {name!r}"


def test_moved_names_are_the_same_objects():
    from smalltts_amd import api, options, plans
    for mod in (options, plans):
        for n in NAMES:
            assert not hasattr(mod, n) or getattr(api, n) is getattr(mod, n), n
    assert api.Takes is options.Takes and api.word_times is plans.word_times and api._frames is plans._frames


@pytest.mark.parametrize("module", ["smalltts_amd.options", "smalltts_amd.plans"])
def test_options_and_plans_import_without_torch(module):
    code = (f"import sys, {module}\n"
            "heavy = [m for m in ('torch', 'smalltts_amd.engine', 'smalltts_amd.api') if m in sys.modules]\n"
            "assert not heavy, heavy\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]


def test_a_delivery_is_made_without_torch_too():
    code = ("import sys\nfrom smalltts_amd.options import Delivery, as_delivery\n"
            "assert as_delivery((16000, 'mulaw')).ratio == (2, 3)\n"
            "assert 'torch' not in sys.modules and 'smalltts_amd.engine' not in sys.modules\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]
