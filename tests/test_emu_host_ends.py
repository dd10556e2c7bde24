"""The two host ends of the boundary call under the emulator (tests/host_ends_cases.py): the product's own marshalling, final
pass and helper kernels run on the CPU, one subprocess per case as in tests/test_emu.py, each against the plain-C restatement."""
import os
import subprocess
import sys

import pytest

import host_ends_cases as hc
from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def _through_emulator(lib, call, env=None, timeout=900):
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import host_ends_cases as hc\n"
        "print(hc.%s)\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), lib, call)
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_emulated_host_ends_match_the_restatement(emu_lib, name):   # noqa: F811
    _through_emulator(emu_lib, "run_case(%r)" % name)


def test_emulated_host_ends_with_two_samples_in_flight(emu_lib):   # noqa: F811
    _through_emulator(emu_lib, "run_multi()")


@pytest.mark.parametrize("label", [k for k, _, _ in hc.INVALID])
def test_emulated_invalid_base_is_refused_with_the_reference_message(emu_lib, label):   # noqa: F811
    _through_emulator(emu_lib, "run_invalid(%r)" % label)
